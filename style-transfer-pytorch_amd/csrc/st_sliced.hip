// The sliced Wasserstein option of a W2 style layer (st_plan_set_style_sliced, losses.StyleLossSliced): the W2 distance between
// the projections of the tap and of the style's feature vectors onto P random unit directions, new directions at every closure
// (Heitz et al., "A Sliced Wasserstein Loss for Neural Texture Synthesis").  On a tap F [C][N], directions R [P][C] with unit
// rows and a target T [P][N] with non-decreasing rows, Y = R F and pi_p the stable ascending order of row p of Y:
//   term = w sum_p sum_k (Y_p,pi_p(k) - T_p,k)^2 / (P N)        dF = w (2 / (P N)) R^T G,   G_p,pi_p(k) = Y_p,pi_p(k) - T_p,k
// The expensive pieces are the project's own: the 1x1 step (st_conv1x1.hip in fp16x3, st_conv.hip in fp32) for both products,
// the segmented sort, the quantile resample and the residual pass (st_sort.hip) on P rows.  New here:
//   sliced_directions_kernel  a wave per row: C standard normals from a counter-based hash of (seed, entry, epoch, p, c) through
//                             Box-Muller, their norm summed in double in a fixed order (lane-strided, then a butterfly), the row
//                             divided by it and written to R [P][C] and R^T [C][P] in the same launch
//   sliced_blend_kernel       T = a q, or T += a q: the style images' resampled quantile functions blended in image order, one
//                             owner per element
// and the host sequences: a style image's share of the target (project, sort, unpack, resample, blend) and the head (project,
// sort + residual into G, the bound on max |G| by the integer atomicMax pass the trunk uses, back-project).
// No floating-point atomics and no data-dependent loop bounds anywhere.
#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "../../include/st_amd.h"
#include "st_common.h"

namespace st {

namespace {

typedef unsigned long long u64;

// splitmix64's finaliser: a bijection of 64-bit words
__host__ __device__ __forceinline__ u64 mix64(u64 z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// the key of one direction set: every (seed, entry, epoch) its own stream
u64 sliced_key(u64 seed, int entry, u64 epoch) {
    u64 k = mix64(seed ^ 0x9e3779b97f4a7c15ull);
    k = mix64(k ^ (u64)(unsigned int)(entry + 1));
    return mix64(k ^ epoch);
}

// element (p, c): one hash word, two uniforms, one normal
__device__ __forceinline__ float sliced_normal(u64 key, unsigned int p, unsigned int c) {
    const u64 h = mix64(key ^ (((u64)p << 32) | c));
    const float u1 = ((float)(unsigned int)(h >> 41) + 0.5f) * 1.1920928955078125e-7f;        // (top 23 bits + 1/2) 2^-23, in (0, 1)
    const float u2 = (float)((unsigned int)h >> 8) * 5.9604644775390625e-8f;                  // bits 31..8 times 2^-24, in [0, 1)
    return sqrtf(-2.f * __logf(u1)) * __builtin_amdgcn_cosf(u2);                               // v_cos_f32 takes revolutions: cos(2 pi u2)
}

// workgroup b: rows 4 b .. 4 b + 3, a wave each
__global__ __launch_bounds__(256) void sliced_directions_kernel(u64 key, int proj, int channels, float* __restrict__ r,
                                                                float* __restrict__ rt) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= proj) return;
    double acc = 0.0;
    for (int c = lane; c < channels; c += 64) {
        const double z = (double)sliced_normal(key, (unsigned int)p, (unsigned int)c);
        acc += z * z;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    const double inv = 1.0 / sqrt(acc);
    for (int c = lane; c < channels; c += 64) {
        const float v = (float)((double)sliced_normal(key, (unsigned int)p, (unsigned int)c) * inv);
        r[(size_t)p * channels + c] = v;
        rt[(size_t)c * proj + p] = v;
    }
}

__global__ __launch_bounds__(256) void sliced_blend_kernel(const float* __restrict__ q, long long count, float a, int accumulate,
                                                           float* __restrict__ target) {
#pragma clang fp contract(off)
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
        const float v = a * q[i];
        target[i] = accumulate ? target[i] + v : v;
    }
}

long long round256(long long bytes) { return ((bytes + 255) / 256) * 256; }

constexpr long long kBoundBytes = (long long)kAmaxWordUints * 4;

// ST_SLICED_FP32 = 1: both products on the exact fp32 MFMA whatever bounds are given (A/B runs)
bool force_fp32() {
    static Option opt("ST_SLICED_FP32", 0);
    return opt.get() != 0;
}

}  // namespace

int sliced_check_shape(const char* who, int channels, int proj, long long n) {
    ST_REQUIRE(channels >= 32 && channels % 32 == 0, "%s: %d channels: a positive multiple of 32", who, channels);
    ST_REQUIRE(proj >= 64 && proj <= 512 && proj % 64 == 0, "%s: %d projections: a multiple of 64 in [64, 512]", who, proj);
    ST_REQUIRE(pixels_in_range(n), "%s: rows of %lld elements: 1 to 2^24 - 1", who, n);      // (kMaxPixels, st_common.h)
    return 0;
}

int launch_sliced_directions(unsigned long long seed, int entry, unsigned long long epoch, int proj, int channels, float* r, float* rt,
                             hipStream_t s) {
    hipLaunchKernelGGL(sliced_directions_kernel, dim3((unsigned)(proj / 4)), dim3(256), 0, s, sliced_key(seed, entry, epoch), proj, channels,
                       r, rt);
    ST_LAUNCH_CHECK();
    return 0;
}

long long sliced_scratch_bytes(int proj, long long n) {
    return 3 * kBoundBytes + 2 * round256((long long)proj * n * 4) + marginal_scratch_bytes(proj, n);
}

SlicedScratch sliced_scratch_of(void* scratch, int proj, long long n) {
    char* base = static_cast<char*>(scratch);
    const long long rows = round256((long long)proj * n * 4);
    SlicedScratch sc;
    sc.in_bound = reinterpret_cast<unsigned int*>(base);
    sc.r_bound = reinterpret_cast<unsigned int*>(base + kBoundBytes);
    sc.g_bound = reinterpret_cast<unsigned int*>(base + 2 * kBoundBytes);
    sc.y = reinterpret_cast<float*>(base + 3 * kBoundBytes);
    sc.g = reinterpret_cast<float*>(base + 3 * kBoundBytes + rows);
    sc.sort = base + 3 * kBoundBytes + 2 * rows;
    return sc;
}

int sliced_product(const float* in, int cin, int cout, long long npix, const float* w, const float* wt, const unsigned int* in_bound,
                   const unsigned int* w_bound, float* out, hipStream_t s) {
    ConvProblem c{};
    c.in = in; c.wgt = w; c.out = out; c.cin = cin; c.cout = cout; c.height = 1; c.width = (int)npix; c.taps = 1;
    if (in_bound && w_bound && !force_fp32()) {
        c.planes = 2; c.elem = 1; c.amax_word = const_cast<unsigned int*>(in_bound); c.wgt_amax = w_bound;
    }
    const char* fp32_env = option_env("ST_CONV1X1_FP32");
    if (!conv1x1_split_applies(c) || (fp32_env && atoi(fp32_env) != 0)) {        // the exact kernel reads its weights as [Cin][Cout]
        c.planes = 0; c.elem = 0; c.amax_word = nullptr; c.wgt_amax = nullptr;
        c.wgt = wt;
    }
    return launch_conv(c, s);
}

int sliced_target_add(const float* feat, int channels, long long m, const float* r, const float* rt, int proj, long long n_out,
                      const SlicedScratch& sc, const unsigned int* feat_bound, const unsigned int* r_bound, float* target, int accumulate,
                      float weight, hipStream_t s) {
    if (sliced_product(feat, channels, proj, m, r, rt, feat_bound, r_bound, sc.y, s)) return 1;
    const MarginalScratch ms = marginal_scratch_of(sc.sort, proj, m);
    if (launch_channel_sort(sc.y, proj, m, ms, s)) return 1;
    if (launch_unpack_keys(ms.keys_a, (long long)proj * m, sc.g, nullptr, s)) return 1;
    const float* q = sc.g;
    if (m != n_out) {
        if (launch_resample_quantiles(sc.g, proj, m, n_out, sc.y, s)) return 1;
        q = sc.y;
    }
    const long long count = (long long)proj * n_out;
    const unsigned blocks = (unsigned)std::min<long long>(1024, (count + 1023) / 1024);
    hipLaunchKernelGGL(sliced_blend_kernel, dim3(blocks), dim3(256), 0, s, q, count, weight, accumulate, target);
    ST_LAUNCH_CHECK();
    return 0;
}

int sliced_head_run(const float* feat, int channels, long long n, const float* r, const float* rt, int proj, const float* target,
                    const SlicedScratch& sc, const unsigned int* feat_bound, const unsigned int* r_bound, float weight, float* grad,
                    float* loss_out, hipStream_t s) {
    if (sliced_product(feat, channels, proj, n, r, rt, feat_bound, r_bound, sc.y, s)) return 1;
    if (marginal_head_run(sc.y, proj, n, target, sc.sort, weight, sc.g, loss_out, s)) return 1;
    const bool f16 = feat_bound && r_bound && !force_fp32();
    if (f16) {              // max |G| as the trunk measures an operand: integer atomicMax on the bit image, no host read
        ST_HIP(hipMemsetAsync(sc.g_bound, 0, (size_t)kBoundBytes, s));
        if (launch_amax(sc.g, (long long)proj * n, sc.g_bound, 0, s)) return 1;
    }
    return sliced_product(sc.g, proj, channels, n, rt, r, f16 ? sc.g_bound : nullptr, r_bound, grad, s);
}

}  // namespace st

using namespace st;

extern "C" {

int st_op_sliced_directions(unsigned long long seed, int entry, unsigned long long epoch, int projections, int channels, float* r_out,
                            float* rt_out, void* stream) {
    ST_REQUIRE(r_out && rt_out, "st_op_sliced_directions: null argument");
    ST_REQUIRE(entry >= 0, "st_op_sliced_directions: entry %d: not negative", entry);
    if (sliced_check_shape("st_op_sliced_directions", channels, projections, 1)) return 1;
    return launch_sliced_directions(seed, entry, epoch, projections, channels, r_out, rt_out, static_cast<hipStream_t>(stream));
}

long long st_op_sliced_scratch_bytes(int channels, int projections, long long n) {
    if (channels < 1 || projections < 1 || n < 1) return 0;
    return sliced_scratch_bytes(projections, n);
}

// the bounds of a standalone call: max |feat| and max |R| measured into the scratch's words
static int measure_op_bounds(const float* feat, long long feat_count, const float* r, long long r_count, const SlicedScratch& sc,
                             hipStream_t s) {
    ST_HIP(hipMemsetAsync(sc.in_bound, 0, (size_t)(3 * kBoundBytes), s));
    return launch_amax(feat, feat_count, sc.in_bound, 0, s) || launch_amax(r, r_count, sc.r_bound, 0, s);
}

int st_op_sliced_target(const float* feat, int channels, long long m, const float* r, const float* rt, int projections, long long n_out,
                        void* scratch, float* target, int accumulate, float weight, void* stream) {
    ST_REQUIRE(feat && r && rt && scratch && target, "st_op_sliced_target: null argument");
    ST_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 255) == 0, "st_op_sliced_target: scratch must be 256-byte aligned");
    if (sliced_check_shape("st_op_sliced_target", channels, projections, m) ||
        sliced_check_shape("st_op_sliced_target", channels, projections, n_out))
        return 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const SlicedScratch sc = sliced_scratch_of(scratch, projections, std::max(m, n_out));
    if (measure_op_bounds(feat, (long long)channels * m, r, (long long)projections * channels, sc, s)) return 1;
    return sliced_target_add(feat, channels, m, r, rt, projections, n_out, sc, sc.in_bound, sc.r_bound, target, accumulate != 0, weight, s);
}

int st_op_sliced_project(const float* feat, int channels, long long n, const float* r, const float* rt, int projections, void* scratch,
                         float* y_out, void* stream) {
    ST_REQUIRE(feat && r && rt && scratch && y_out, "st_op_sliced_project: null argument");
    ST_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 255) == 0, "st_op_sliced_project: scratch must be 256-byte aligned");
    if (sliced_check_shape("st_op_sliced_project", channels, projections, n)) return 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const SlicedScratch sc = sliced_scratch_of(scratch, projections, n);
    if (measure_op_bounds(feat, (long long)channels * n, r, (long long)projections * channels, sc, s)) return 1;
    return sliced_product(feat, channels, projections, n, r, rt, sc.in_bound, sc.r_bound, y_out, s);
}

int st_op_sliced_loss(const float* feat, int channels, long long n, const float* r, const float* rt, int projections, const float* target,
                      void* scratch, float* unit_grad_out, float* loss_out, void* stream) {
    ST_REQUIRE(feat && r && rt && target && scratch && unit_grad_out && loss_out, "st_op_sliced_loss: null argument");
    ST_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 255) == 0, "st_op_sliced_loss: scratch must be 256-byte aligned");
    if (sliced_check_shape("st_op_sliced_loss", channels, projections, n)) return 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const SlicedScratch sc = sliced_scratch_of(scratch, projections, n);
    if (measure_op_bounds(feat, (long long)channels * n, r, (long long)projections * channels, sc, s)) return 1;
    ST_HIP(hipMemsetAsync(sc.sort, 0, 16, s));
    return sliced_head_run(feat, channels, n, r, rt, projections, target, sc, sc.in_bound, sc.r_bound, 1.f, unit_grad_out, loss_out, s);
}

int st_op_sliced_loss_backward(const float* unit_grad, long long count, const float* upstream, float* grad, void* stream) {
    ST_REQUIRE(unit_grad && upstream && grad && count >= 1, "st_op_sliced_loss_backward: null argument or empty tensor");
    return st_op_w2_marginal_loss_backward(unit_grad, count, upstream, grad, stream);
}

}  // extern "C"
