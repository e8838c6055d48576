// The exact per-channel Wasserstein (sorted) option of a W2 style layer (st_plan_set_w2_marginal, losses.StyleLossW2Marginal):
// the W2 distance between the exact one-dimensional marginals of the tap and of the style's tap - the sliced Wasserstein loss
// of Heitz et al. taken along the channel axes, the exact form of Risser et al.'s histogram loss.  On a tap F [C][N] and a
// target T [C][N] with non-decreasing rows, pi_c the stable ascending order of row c:
//   term = w sum_c sum_k (f_c,pi_c(k) - T_c,k)^2 / (C N)        dF_c,pi_c(k) = w (2 / (C N)) (f_c,pi_c(k) - T_c,k)
// The hot path is a segmented stable sort of the rows on composite 64-bit keys: the order-preserving integer image of f + 0.0f
// (-0.0 sorts as +0.0) in the high word, the pixel index in the low word.  Keys are unique, so every comparison sort gives the
// one stable order and two runs give the same bits.
//   chunk_sort_kernel<K>      one workgroup sorts K keys of a row in LDS (bitonic network: its control flow is the same for
//                             every input, NaNs included); the row's last chunk is padded in LDS only, with the all-ones key,
//                             which no element has (N <= 2^32 - 1: an index is at most 2^32 - 2)
//   merge_pass_kernel         ceil(log2(runs)) passes between two buffers: an element's slot in the merged pair of runs is its
//                             position in its own run plus the count of smaller keys in the sibling run (a bounded binary
//                             search); a run without a sibling is copied.  The first buffer written is chosen by the parity
//                             of the pass count, so the result always ends in buffer A.
//   unpack_keys_kernel        sorted values and / or the permutation from the keys (st_op_channel_sort, Plan.quantiles)
//   resample_rows_kernel      the target: a quantile function [C][n_in] at n_out midpoints, u in double, the lerp in fp32
//   marginal_residual_kernel  walks the sorted keys against T: the gradient through the permutation (one owner per element,
//                             written - a content term of the same layer adds after it), sum d^2 as per-block fp32 partials,
//                             a ticket, and the last block's index-order sum in double with the weighted term
//   scale_by_scalar_kernel    grad = upstream[0] unit_grad (the module's backward)
// No floating-point atomics and no data-dependent loop bounds anywhere.
#include <algorithm>
#include <cstdint>

#include "../../include/st_amd.h"
#include "st_common.h"

namespace st {

namespace {

typedef unsigned long long u64;

constexpr int kSortThreads = 512;
constexpr int kTileElems = 1024;                  // elements of a row per workgroup of the streaming kernels: 4 per thread
constexpr u64 kPadKey = ~0ull;

__device__ __forceinline__ u64 make_key(float f, unsigned int index) {
    unsigned int u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0u;                 // f + 0.0f: -0.0 compares equal to +0.0, the index alone orders them
    u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
    return ((u64)u << 32) | index;
}
__device__ __forceinline__ float key_value(u64 key) {
    unsigned int u = (unsigned int)(key >> 32);
    u ^= (u >> 31) ? 0x80000000u : 0xffffffffu;
    return __uint_as_float(u);
}

// workgroup blockIdx.x = row * runs + run sorts elements [run K, min((run + 1) K, n)) of its row
template <int K>
__global__ __launch_bounds__(kSortThreads) void chunk_sort_kernel(const float* __restrict__ feat, long long n, int runs,
                                                                  u64* __restrict__ out) {
    __shared__ u64 keys[K];
    const long long row = blockIdx.x / (unsigned)runs, base = (long long)(blockIdx.x % (unsigned)runs) * K;
    const float* src = feat + row * n;
    for (int t = threadIdx.x; t < K; t += kSortThreads) {
        const long long i = base + t;
        keys[t] = i < n ? make_key(src[i], (unsigned int)i) : kPadKey;
    }
    __syncthreads();
    for (int k = 2; k <= K; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < K / 2; t += kSortThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));       // the pair's lower element: bit j clear
                const u64 a = keys[i], b = keys[i + j];
                const bool ascending = (i & k) == 0;
                if ((a > b) == ascending) {
                    keys[i] = b;
                    keys[i + j] = a;
                }
            }
            __syncthreads();
        }
    }
    u64* dst = out + row * n;
    for (int t = threadIdx.x; t < K; t += kSortThreads) {
        const long long i = base + t;
        if (i < n) dst[i] = keys[t];
    }
}

// workgroup blockIdx.x = row * tiles + tile; runs of `run` keys (the row's last one shorter) merge in pairs
__global__ __launch_bounds__(256) void merge_pass_kernel(const u64* __restrict__ src, u64* __restrict__ dst, long long n, long long run,
                                                         int tiles) {
    const long long row = blockIdx.x / (unsigned)tiles, first = (long long)(blockIdx.x % (unsigned)tiles) * kTileElems;
    const u64* s = src + row * n;
    u64* d = dst + row * n;
#pragma unroll
    for (int e = 0; e < kTileElems / 256; ++e) {
        const long long i = first + e * 256 + threadIdx.x;
        if (i >= n) continue;
        const u64 key = s[i];
        const long long r = i / run, start = r * run, sib_start = (r ^ 1) * run;
        if (sib_start >= n) {                     // the odd run at the row's end: carried across
            d[i] = key;
            continue;
        }
        long long lo = 0, hi = n - sib_start < run ? n - sib_start : run;
        while (lo < hi) {                         // at most 33 rounds: the keys of the sibling run that are smaller (none is equal)
            const long long mid = (lo + hi) >> 1;
            if (s[sib_start + mid] < key) lo = mid + 1; else hi = mid;
        }
        d[(start < sib_start ? start : sib_start) + (i - start) + lo] = key;
    }
}

__global__ __launch_bounds__(256) void unpack_keys_kernel(const u64* __restrict__ keys, long long count, float* __restrict__ sorted_out,
                                                          unsigned int* __restrict__ perm_out) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
        const u64 key = keys[i];
        if (sorted_out) sorted_out[i] = key_value(key);
        if (perm_out) perm_out[i] = (unsigned int)key;
    }
}

// out[c][i] = lerp(q_c, u), u = clamp((i + 1/2) n_in / n_out - 1/2, 0, n_in - 1) in double: order statistic k sits at (k + 1/2) / n_in
__global__ __launch_bounds__(256) void resample_rows_kernel(const float* __restrict__ q, long long n_in, long long n_out, int tiles,
                                                            float* __restrict__ out) {
#pragma clang fp contract(off)
    const long long row = blockIdx.x / (unsigned)tiles, first = (long long)(blockIdx.x % (unsigned)tiles) * kTileElems;
    const float* s = q + row * n_in;
    float* d = out + row * n_out;
#pragma unroll
    for (int e = 0; e < kTileElems / 256; ++e) {
        const long long i = first + e * 256 + threadIdx.x;
        if (i >= n_out) continue;
        double u = ((double)i + 0.5) * (double)n_in / (double)n_out - 0.5;
        u = u > 0.0 ? u : 0.0;
        u = u < (double)(n_in - 1) ? u : (double)(n_in - 1);
        const long long i0 = (long long)u, i1 = i0 + 1 < n_in ? i0 + 1 : n_in - 1;
        const float t = (float)(u - (double)i0);
        const float a = s[i0], b = s[i1];
        d[i] = t == 0.f ? a : a + t * (b - a);
    }
}

struct MarginalFinish {
    double weight = 1.0, count = 1.0;   // w and C N
    float coef = 0.f;                   // w 2 / (C N), rounded once
    float* loss_out = nullptr;
};

// a grid-stride loop over the C N sorted keys; element e of row e / n belongs to pixel (low word of its key)
__global__ __launch_bounds__(256) void marginal_residual_kernel(const u64* __restrict__ keys, const float* __restrict__ target, long long n,
                                                                long long count, float* __restrict__ grad, float* __restrict__ partials,
                                                                LastBlock lb, MarginalFinish fin) {
#pragma clang fp contract(off)
    __shared__ float scratch[4];
    __shared__ bool is_last;
    __shared__ double sums[256];
    float acc = 0.f;
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < count; e += (long long)gridDim.x * 256) {
        const u64 key = keys[e];
        const float d = key_value(key) - target[e];
        grad[(e / n) * n + (long long)(unsigned int)key] = fin.coef * d;
        acc += d * d;
    }
    acc = block_sum_256(acc, scratch);
    const float part[1] = {acc};
    if (!last_block_arrives(lb, &is_last, partials + blockIdx.x, part)) return;
    // the last block: thread t adds partials [t per, (t + 1) per) in index order, thread 0 the 256 sums in thread order
    const int blocks = (int)gridDim.x, per = (blocks + 255) / 256;
    double mine = 0.0;
    for (int i = threadIdx.x * per; i < blocks && i < ((int)threadIdx.x + 1) * per; ++i) mine += (double)partials[i];
    sums[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int i = 0; i < 256; ++i) total += sums[i];
        fin.loss_out[0] = (float)(fin.weight * total / fin.count);
    }
}

__global__ __launch_bounds__(256) void scale_by_scalar_kernel(const float* __restrict__ x, const float* __restrict__ scalar, long long count,
                                                              float* __restrict__ out) {
    const float a = scalar[0];
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += (long long)gridDim.x * 256) out[i] = a * x[i];
}

Option& chunk_option() {
    static Option opt("ST_SORT_CHUNK", 4096);
    return opt;
}

long long tiles_of(long long n) { return (n + kTileElems - 1) / kTileElems; }

// rows above 65535 ride in the grid's x dimension with the chunks / tiles; what does not fit it is refused, not wrapped
int check_sort_shape(const char* who, int channels, long long n) {
    ST_REQUIRE(channels >= 1 && n >= 1 && n <= 0xffffffffll, "%s: %d rows of %lld elements: at least one row of 1 to 2^32 - 1 elements", who,
               channels, n);
    ST_REQUIRE((long long)channels * std::max(tiles_of(n), (n + 4095) / 4096) <= 0x7fffffffll,
               "%s: %d rows of %lld elements need more than 2^31 - 1 workgroups in one launch", who, channels, n);
    return 0;
}

unsigned stream_blocks(long long count) { return (unsigned)std::min<long long>(kMarginalBlocks, (count + 1023) / 1024); }

}  // namespace

int sort_chunk() { return chunk_option().get() == 8192 ? 8192 : 4096; }

long long marginal_scratch_bytes(int channels, long long n) {
    const long long keys = (((long long)channels * n * 8 + 255) / 256) * 256;
    return kMarginalHeaderBytes + 2 * keys;
}

MarginalScratch marginal_scratch_of(void* scratch, int channels, long long n) {
    char* base = static_cast<char*>(scratch);
    const long long keys = (((long long)channels * n * 8 + 255) / 256) * 256;
    MarginalScratch m;
    m.ticket = reinterpret_cast<unsigned int*>(base);
    m.partials = reinterpret_cast<float*>(base + 256);
    m.keys_a = reinterpret_cast<unsigned long long*>(base + kMarginalHeaderBytes);
    m.keys_b = reinterpret_cast<unsigned long long*>(base + kMarginalHeaderBytes + keys);
    return m;
}

int launch_channel_sort(const float* feat, int channels, long long n, const MarginalScratch& m, hipStream_t s) {
    if (check_sort_shape("launch_channel_sort", channels, n)) return 1;
    const int chunk = sort_chunk();
    const long long runs = (n + chunk - 1) / chunk;
    int passes = 0;
    while (((long long)chunk << passes) < n) ++passes;
    u64* src = (passes & 1) ? m.keys_b : m.keys_a;      // ... so that the last pass writes keys_a
    u64* dst = (passes & 1) ? m.keys_a : m.keys_b;
    const dim3 grid((unsigned)(channels * runs));
    if (chunk == 8192)
        hipLaunchKernelGGL(chunk_sort_kernel<8192>, grid, dim3(kSortThreads), 0, s, feat, n, (int)runs, src);
    else
        hipLaunchKernelGGL(chunk_sort_kernel<4096>, grid, dim3(kSortThreads), 0, s, feat, n, (int)runs, src);
    ST_LAUNCH_CHECK();
    const int tiles = (int)tiles_of(n);
    for (int pass = 0; pass < passes; ++pass) {
        hipLaunchKernelGGL(merge_pass_kernel, dim3((unsigned)(channels * (long long)tiles)), dim3(256), 0, s, src, dst, n,
                           (long long)chunk << pass, tiles);
        ST_LAUNCH_CHECK();
        std::swap(src, dst);
    }
    return 0;
}

int launch_unpack_keys(const unsigned long long* keys, long long count, float* sorted_out, unsigned int* perm_out, hipStream_t s) {
    hipLaunchKernelGGL(unpack_keys_kernel, dim3(stream_blocks(count)), dim3(256), 0, s, keys, count, sorted_out, perm_out);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_resample_quantiles(const float* q, int channels, long long n_in, long long n_out, float* out, hipStream_t s) {
    if (check_sort_shape("launch_resample_quantiles", channels, n_in) || check_sort_shape("launch_resample_quantiles", channels, n_out))
        return 1;
    if (n_in == n_out) {                      // a copy, bit for bit
        ST_HIP(hipMemcpyAsync(out, q, (size_t)channels * n_in * sizeof(float), hipMemcpyDeviceToDevice, s));
        return 0;
    }
    const int tiles = (int)tiles_of(n_out);
    hipLaunchKernelGGL(resample_rows_kernel, dim3((unsigned)(channels * (long long)tiles)), dim3(256), 0, s, q, n_in, n_out, tiles, out);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_marginal_residual(const MarginalScratch& m, const float* target, int channels, long long n, float weight, float* grad,
                             float* loss_out, hipStream_t s) {
    const long long count = (long long)channels * n;
    MarginalFinish fin;
    fin.weight = (double)weight;
    fin.count = (double)count;
    fin.coef = (float)((double)weight * 2.0 / (double)count);
    fin.loss_out = loss_out;
    hipLaunchKernelGGL(marginal_residual_kernel, dim3(stream_blocks(count)), dim3(256), 0, s, m.keys_a, target, n, count, grad, m.partials,
                       last_block(m.ticket), fin);
    ST_LAUNCH_CHECK();
    return 0;
}

int marginal_head_run(const float* feat, int channels, long long n, const float* target, void* scratch, float weight, float* grad,
                      float* loss_out, hipStream_t s) {
    const MarginalScratch m = marginal_scratch_of(scratch, channels, n);
    if (launch_channel_sort(feat, channels, n, m, s)) return 1;
    return launch_marginal_residual(m, target, channels, n, weight, grad, loss_out, s);
}

}  // namespace st

using namespace st;

extern "C" {

int st_op_sort_chunk(void) { return sort_chunk(); }

long long st_op_sort_scratch_bytes(int channels, long long n) {
    if (channels < 1 || n < 1) return 0;
    return marginal_scratch_bytes(channels, n);
}

int st_op_channel_sort(const float* feat, int channels, long long n, void* scratch, float* sorted_out, unsigned int* perm_out,
                       void* stream) {
    ST_REQUIRE(feat && scratch, "st_op_channel_sort: null argument");
    ST_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 255) == 0, "st_op_channel_sort: scratch must be 256-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const MarginalScratch m = marginal_scratch_of(scratch, channels, n);
    if (launch_channel_sort(feat, channels, n, m, s)) return 1;
    if (!sorted_out && !perm_out) return 0;
    return launch_unpack_keys(m.keys_a, (long long)channels * n, sorted_out, perm_out, s);
}

int st_op_resample_quantiles(const float* q, int channels, long long n_in, long long n_out, float* out, void* stream) {
    ST_REQUIRE(q && out, "st_op_resample_quantiles: null argument");
    return launch_resample_quantiles(q, channels, n_in, n_out, out, static_cast<hipStream_t>(stream));
}

int st_op_w2_marginal_loss(const float* feat, int channels, long long n, const float* target, void* scratch, float* unit_grad_out,
                           float* loss_out, void* stream) {
    ST_REQUIRE(feat && target && scratch && unit_grad_out && loss_out, "st_op_w2_marginal_loss: null argument");
    ST_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 255) == 0, "st_op_w2_marginal_loss: scratch must be 256-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (check_sort_shape("st_op_w2_marginal_loss", channels, n)) return 1;
    ST_HIP(hipMemsetAsync(scratch, 0, 16, s));
    return marginal_head_run(feat, channels, n, target, scratch, 1.f, unit_grad_out, loss_out, s);
}

int st_op_w2_marginal_loss_backward(const float* unit_grad, long long count, const float* upstream, float* grad, void* stream) {
    ST_REQUIRE(unit_grad && upstream && grad && count >= 1, "st_op_w2_marginal_loss_backward: null argument or empty tensor");
    hipLaunchKernelGGL(scale_by_scalar_kernel, dim3(stream_blocks(count)), dim3(256), 0, static_cast<hipStream_t>(stream), unit_grad, upstream,
                       count, grad);
    ST_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
