// The nearest-neighbour feature-matching option of a W2 style layer (st_plan_set_style_nearest, losses.StyleLossNearest): every
// feature vector of the tap is pulled towards the closest feature vector of the style - the MRF / neural-neighbour family of style
// losses (Li & Wand's CNNMRF, Kolkin et al.'s NNST) in its L2 form, the one-sided Chamfer distance from the tap to the style set.
// On a tap F [C][N] with columns f_i and style vectors S [C][M] with columns s_k:
//   k*(i) = argmin_k |f_i - s_k|^2 = argmax_k (<f_i, s_k> - |s_k|^2 / 2), ties: the lowest k
//   term  = w sum_i |f_i - s_k*(i)|^2 / (C N)            dF_ci = w (2 / (C N)) (f_ci - s_c,k*(i))
// The hot path is the M x C by C x N product of the search.  It is conv1x1_f16_kernel's staging and MFMA loop (st_conv1x1.hip:
// both operands scaled by a power of two under their bounds and split into two fp16 planes WHILE THEY ARE STAGED, three
// v_mfma_f32_32x32x16_f16 products, fp32 accumulation) with W = S^T and b = -|s|^2 / 2 - but the epilogue writes no score: the
// accumulators keep one pixel per lane and 16 style vectors per register block, so the arg-max over k is a per-lane running
// (score, k).  Nothing of size N x M exists anywhere.
//   nearest_transpose_kernel  S [C][M] -> S^T [M_pad][C], zero rows in the padding (the setter, once)
//   nearest_bias_kernel       bias_k = -|s_k|^2 / 2 summed in double in channel order, rounded to fp32; -inf in the padding, so
//                             padding never wins against a finite score
//   nearest_search_kernel     a workgroup owns 128 pixels and a contiguous range of k tiles (128 style vectors each).  Per k tile
//                             it runs the chunk loop over C - the tap's chunks are staged again for every k tile: at C = 512 the
//                             two planes of a 128-pixel tile are 256 KB and do not fit the LDS, and the tap is L2-resident - and
//                             folds the tile's scores into the running (score, k) in ascending k with "greater"; the two
//                             half-wave row groups are folded with one cross-lane exchange under "greater, or equal and lower k";
//                             one (score, k) per pixel and split is written
//   nearest_finish_kernel     merges a pixel's splits in split order by the same rule, gathers s_k* as a contiguous row of S^T,
//                             writes dF (one owner per element, WRITTEN - a content term of the same layer adds after it;
//                             coalesced through LDS) and the index array, and reduces the term by per-block fp32 partials, a
//                             ticket and the last block's index-order sum in double
//   nearest_merge_kernel      the search entry's ending: the merge alone, indices and best scores
//   nearest_scale_kernel      grad = upstream[0] unit_grad (the module's backward)
// Cosine and centred-cosine matching (st_plan_set_nearest_metric; include/st_amd.h fixes the semantics) is the same search on
// unit rows: W = s^^T with s^_k = (s_k - mu) / sqrt(|s_k - mu|^2 + eps), b_k = -<mu, s^_k>, mu = 0 or the style set's mean.
//   cosine_mean_kernel            mu in double in ascending k, rounded once (the setter, once)
//   cosine_rows_kernel            s^^T [M_pad][C] and b, formed in double and rounded once; zero rows and -inf in the padding
//   nearest_cosine_finish_kernel  a workgroup owns 64 pixels and ALL their channels: it merges the splits, gathers s^_k*, recomputes
//                                 p_i = <f_i - mu, s^_k*> and |f_i - mu|^2 in fp32 in a fixed channel order (first read of the
//                                 tap), writes dF = (w / N) (-s^_k* / r_i + p_i g_i / r_i^3) (second read) and the indices, and
//                                 reduces sum_i (1 - p_i / r_i) as nearest_finish_kernel does
// No floating-point atomics: two runs give the same bits, indices included.  No loop's trip count depends on a comparison of
// values, so every launch ends on any input; an index is clamped into [0, M) before it is used as an address.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/st_amd.h"
#include "st_common.h"

namespace st {

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
constexpr int PT = 40;                    // LDS row pitch in halfs (st_conv1x1.hip)
constexpr int KC = kNearestChunk;         // channels per chunk
constexpr int CM = 4;                     // 32-row blocks of S^T per k tile
constexpr int TK = kNearestKTile;         // style vectors per k tile
constexpr int TPX = kNearestPixelTile;    // pixels per workgroup: 4 waves side by side, 32 pixels each
constexpr int FPX = 64;                   // finish kernel: pixels per workgroup ...
constexpr int FCH = 4;                    // ... and chunks of 32 channels
static_assert(TK == 32 * CM && KC == 32 && TPX == 128, "the staging maps below are written for these");

__device__ __forceinline__ void split_scaled(const float (&v)[8], float scale, _Float16* p0, _Float16* p1) {
    f16x8 h0, h1;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = v[e] * scale;
        const _Float16 a = (_Float16)x;
        h0[e] = a;
        h1[e] = (_Float16)(x - (float)a);
    }
    *reinterpret_cast<f16x8*>(p0) = h0;
    *reinterpret_cast<f16x8*>(p1) = h1;
}

// "greater, or equal and lower k": the order in which every pair of candidates is compared
__device__ __forceinline__ bool candidate_wins(float score, int k, float best, int best_k) {
    return score > best || (score == best && k < best_k);
}

// blockIdx.x: the pixel tile, blockIdx.y: the split, which owns k tiles [y tiles_per_split, min((y + 1) tiles_per_split, ktiles))
__global__ __launch_bounds__(256, 2) void nearest_search_kernel(const float* __restrict__ feat, const float* __restrict__ st_t,
                                                                const float* __restrict__ bias, int cin, long long npix, int ktiles,
                                                                int tiles_per_split, const unsigned int* __restrict__ feat_bound,
                                                                const unsigned int* __restrict__ s_bound, float* __restrict__ part_score,
                                                                int* __restrict__ part_k, int vec_ok) {
    __shared__ __attribute__((aligned(16))) _Float16 lds_x[2][TPX * PT];   // [plane][pixel][ci]
    __shared__ __attribute__((aligned(16))) _Float16 lds_w[2][TK * PT];    // [plane][k][ci]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const long long px0 = (long long)blockIdx.x * TPX;
    const int ea = scale_exp(amax_read(feat_bound)), ew = scale_exp(amax_read(s_bound));
    const float sa = pow2f(ea), sw = pow2f(ew), ua = pow2f(-ea), uw = pow2f(-ew);

    // staging maps: the tap (4 pixels at 4*pg, channels 8*cg..+7, threads 0..127), S^T (rows pg and pg + 64, channels 8*cg..+7)
    const int cg = tid & 3, pg = tid >> 2;
    const bool xact = pg < TPX / 4;
    f32x4 xr[8], wr[CM];

    auto load_chunk = [&](int kt, int k0) {
        if (xact) {
            const long long px = px0 + 4 * pg;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float* p = feat + (size_t)(k0 + cg * 8 + c) * npix + px;
                if (vec_ok && px + 3 < npix) {
                    xr[c] = *reinterpret_cast<const f32x4*>(p);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) xr[c][e] = (px + e < npix) ? p[e] : 0.f;
                }
            }
        }
#pragma unroll
        for (int h = 0; h < CM / 2; ++h) {
            const float* w = st_t + ((size_t)kt * TK + h * 64 + pg) * cin + k0 + cg * 8;
            wr[2 * h] = *reinterpret_cast<const f32x4*>(w);
            wr[2 * h + 1] = *reinterpret_cast<const f32x4*>(w + 4);
        }
    };
    auto store_chunk = [&]() {
        if (xact) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float v[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) v[c] = xr[c][j];
                const int off = (4 * pg + j) * PT + cg * 8;
                split_scaled(v, sa, &lds_x[0][off], &lds_x[1][off]);
            }
        }
#pragma unroll
        for (int h = 0; h < CM / 2; ++h) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = wr[2 * h + (e >> 2)][e & 3];
            const int off = (h * 64 + pg) * PT + cg * 8;
            split_scaled(v, sw, &lds_w[0][off], &lds_w[1][off]);
        }
    };

    float best = -INFINITY;
    int best_k = 0x7fffffff;
    const int nchunks = cin / KC;
    const int kt_first = blockIdx.y * tiles_per_split;
    const int kt_end = min(ktiles, kt_first + tiles_per_split);
    for (int kt = kt_first; kt < kt_end; ++kt) {
        f32x16 acc[CM];
#pragma unroll
        for (int m = 0; m < CM; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
        __syncthreads();                          // the former tile's last chunk has been read by every wave
        load_chunk(kt, 0);
        store_chunk();
        __syncthreads();
        for (int ch = 0; ch < nchunks; ++ch) {
            const bool more = ch + 1 < nchunks;
            if (more) load_chunk(kt, (ch + 1) * KC);
#pragma unroll
            for (int kb = 0; kb < KC / 16; ++kb) {
                const int row = wave * 32 + l31;
                const f16x8 b0 = *reinterpret_cast<const f16x8*>(&lds_x[0][row * PT + kb * 16 + 8 * half]);
                const f16x8 b1 = *reinterpret_cast<const f16x8*>(&lds_x[1][row * PT + kb * 16 + 8 * half]);
#pragma unroll
                for (int m = 0; m < CM; ++m) {
                    const f16x8 a0 = *reinterpret_cast<const f16x8*>(&lds_w[0][(m * 32 + l31) * PT + kb * 16 + 8 * half]);
                    const f16x8 a1 = *reinterpret_cast<const f16x8*>(&lds_w[1][(m * 32 + l31) * PT + kb * 16 + 8 * half]);
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, acc[m], 0, 0, 0);
                }
            }
            if (more) {
                __syncthreads();
                store_chunk();
                __syncthreads();
            }
        }
        // acc[m][r]: k = kt TK + m*32 + (r&3) + 8*(r>>2) + 4*half (ascending in m, r), pixel = px0 + wave*32 + l31
#pragma unroll
        for (int m = 0; m < CM; ++m) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = kt * TK + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const float score = acc[m][r] * ua * uw + bias[k];
                if (score > best) {
                    best = score;
                    best_k = k;
                }
            }
        }
    }
    // the other half-wave holds the same pixel's interleaved rows
    const float other = __shfl_xor(best, 32, 64);
    const int other_k = __shfl_xor(best_k, 32, 64);
    if (candidate_wins(other, other_k, best, best_k)) {
        best = other;
        best_k = other_k;
    }
    const long long px = px0 + wave * 32 + l31;
    if (half == 0 && px < npix) {
        part_score[(size_t)blockIdx.y * npix + px] = best;
        part_k[(size_t)blockIdx.y * npix + px] = best_k;
    }
}

// [32][32] tiles: S [C][M] read along k, S^T [M_pad][C] written along c; rows k >= m are zero
__global__ __launch_bounds__(256) void nearest_transpose_kernel(const float* __restrict__ s, int cin, long long m, float* __restrict__ st_t) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long long k0 = (long long)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = c0 + ty + 8 * j;
        const long long k = k0 + tx;
        tile[ty + 8 * j][tx] = k < m ? s[(size_t)c * m + k] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long k = k0 + ty + 8 * j;
        st_t[(size_t)k * cin + c0 + tx] = tile[tx][ty + 8 * j];
    }
}

__global__ __launch_bounds__(256) void nearest_bias_kernel(const float* __restrict__ st_t, int cin, long long m, long long m_pad,
                                                           float* __restrict__ bias) {
    const long long k = blockIdx.x * 256ll + threadIdx.x;
    if (k >= m_pad) return;
    if (k >= m) {
        bias[k] = -INFINITY;
        return;
    }
    double sum = 0.0;
    for (int c = 0; c < cin; ++c) {
        const double v = (double)st_t[(size_t)k * cin + c];
        sum += v * v;
    }
    bias[k] = (float)(-0.5 * sum);
}

// a pixel's splits in split order under the same rule; the index is clamped into [0, m) (a NaN's leftovers: never an address out
// of bounds)
__device__ __forceinline__ float merge_splits(const float* __restrict__ part_score, const int* __restrict__ part_k, int splits,
                                              long long npix, long long m, long long px, int* k_out) {
    float best = part_score[px];
    int k = part_k[px];
    for (int sp = 1; sp < splits; ++sp) {
        const float score = part_score[(size_t)sp * npix + px];
        const int ks = part_k[(size_t)sp * npix + px];
        if (candidate_wins(score, ks, best, k)) {
            best = score;
            k = ks;
        }
    }
    *k_out = k < 0 ? 0 : ((long long)k >= m ? (int)(m - 1) : k);
    return best;
}

// the search entry's own ending: indices and best scores, no gradient
__global__ __launch_bounds__(256) void nearest_merge_kernel(const float* __restrict__ part_score, const int* __restrict__ part_k, int splits,
                                                            long long npix, long long m, int* __restrict__ idx_out,
                                                            float* __restrict__ score_out) {
    const long long px = blockIdx.x * 256ll + threadIdx.x;
    if (px >= npix) return;
    int k;
    const float best = merge_splits(part_score, part_k, splits, npix, m, px, &k);
    idx_out[px] = k;
    if (score_out) score_out[px] = best;
}

struct NearestFinish {
    double weight = 1.0, count = 1.0;   // w and C N
    float coef = 0.f;                   // w 2 / (C N), rounded once
    float* loss_out = nullptr;
};

// blockIdx.x = pixel tile * cgroups + channel group: FPX pixels, FCH chunks of 32 channels
__global__ __launch_bounds__(256) void nearest_finish_kernel(const float* __restrict__ feat, const float* __restrict__ st_t,
                                                             const float* __restrict__ part_score, const int* __restrict__ part_k,
                                                             int splits, long long npix, int cin, long long m, int cgroups,
                                                             int* __restrict__ idx_out, float* __restrict__ score_out,
                                                             float* __restrict__ grad, float* __restrict__ partials, LastBlock lb,
                                                             NearestFinish fin) {
#pragma clang fp contract(off)
    __shared__ int ksel[FPX];
    __shared__ float tile[32][FPX + 1];
    __shared__ float scratch[4];
    __shared__ bool is_last;
    __shared__ double sums[256];
    const int tid = threadIdx.x;
    const long long px0 = (long long)(blockIdx.x / (unsigned)cgroups) * FPX;
    const int cgrp = blockIdx.x % (unsigned)cgroups;
    if (tid < FPX) {
        const long long px = px0 + tid;
        int k = 0;
        if (px < npix) {
            const float best = merge_splits(part_score, part_k, splits, npix, m, px, &k);
            if (cgrp == 0) {
                idx_out[px] = k;
                if (score_out) score_out[px] = best;
            }
        }
        ksel[tid] = k;
    }
    __syncthreads();
    float acc = 0.f;
    const int nchunks = cin / KC;
    for (int ch = cgrp * FCH; ch < nchunks && ch < (cgrp + 1) * FCH; ++ch) {
        const int c0 = ch * KC;
        {   // gather: thread (pixel tid >> 2, quarter tid & 3) reads 8 consecutive channels of its pixel's row of S^T
            const int p = tid >> 2, q = tid & 3;
            const float* row = st_t + (size_t)ksel[p] * cin + c0 + q * 8;
            const f32x4 lo = *reinterpret_cast<const f32x4*>(row), hi = *reinterpret_cast<const f32x4*>(row + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                tile[q * 8 + e][p] = lo[e];
                tile[q * 8 + 4 + e][p] = hi[e];
            }
        }
        __syncthreads();
        const long long px = px0 + (tid & 63);
        if (px < npix) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int cl = (tid >> 6) + 4 * e;
                const size_t at = (size_t)(c0 + cl) * npix + px;
                const float d = feat[at] - tile[cl][tid & 63];
                grad[at] = fin.coef * d;
                acc += d * d;
            }
        }
        __syncthreads();
    }
    acc = block_sum_256(acc, scratch);
    const float part[1] = {acc};
    if (!last_block_arrives(lb, &is_last, partials + blockIdx.x, part)) return;
    // the last block: thread t adds partials [t per, (t + 1) per) in index order, thread 0 the 256 sums in thread order
    const long long blocks = gridDim.x, per = (blocks + 255) / 256;
    double mine = 0.0;
    for (long long i = tid * per; i < blocks && i < (tid + 1) * per; ++i) mine += (double)partials[i];
    sums[tid] = mine;
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (int i = 0; i < 256; ++i) total += sums[i];
        fin.loss_out[0] = (float)(fin.weight * total / fin.count);
    }
}

__global__ __launch_bounds__(256) void nearest_scale_kernel(const float* __restrict__ x, const float* __restrict__ scalar, long long count,
                                                            float* __restrict__ out) {
    const float a = scalar[0];
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += (long long)gridDim.x * 256) out[i] = a * x[i];
}

// ---- cosine and centred-cosine matching (st_plan_set_nearest_metric): the prepare kernels and the finish pass ----
constexpr int CPX = 64;                   // cosine finish: pixels per workgroup, which owns ALL their channels
constexpr int CTP = 68;                   // pitch of its gathered tile in floats: rows stay 16-byte aligned
constexpr double kCosEps = 1e-8;          // kNearestCosineEps where the sums are double

// mu_c = (1/M) sum_k s_ck, in double in ascending k, rounded once (0 for the plain cosine and in the padding behind C).  One wave
// per channel: 64 coalesced loads, then every lane adds the 64 values in lane order
__global__ __launch_bounds__(64) void cosine_mean_kernel(const float* __restrict__ s, int cin, long long m, int centered,
                                                         float* __restrict__ mu) {
    const int c = blockIdx.x, lane = threadIdx.x;
    if (!centered || c >= cin) {
        if (lane == 0) mu[c] = 0.f;
        return;
    }
    double sum = 0.0;
    for (long long k0 = 0; k0 < m; k0 += 64) {
        const float v = k0 + lane < m ? s[(size_t)c * m + k0 + lane] : 0.f;
        const int cnt = (int)min(64ll, m - k0);
        for (int j = 0; j < cnt; ++j) sum += (double)__shfl(v, j, 64);
    }
    if (lane == 0) mu[c] = (float)(sum / (double)m);
}

// thread = style vector k: |s_k - mu|^2 in double in channel order, then s^_k = (s_k - mu) / sqrt(|s_k - mu|^2 + eps) rounded once
// (a zero vector stays zero), transposed through LDS into rows of s^T, and b_k = -<mu, s^_k> from the ROUNDED s^_k and mu, in
// double in channel order, rounded once.  Padding rows are zero and their bias -inf.  The grid covers M_pad
__global__ __launch_bounds__(64) void cosine_rows_kernel(const float* __restrict__ s, const float* __restrict__ mu, int cin, long long m,
                                                         float* __restrict__ st_t, float* __restrict__ bias) {
    __shared__ float tile[64][33];
    const int lane = threadIdx.x;
    const long long k0 = blockIdx.x * 64ll, k = k0 + lane;
    const bool live = k < m;
    double nrm = 0.0;
    for (int c = 0; c < cin; ++c) {
        const double d = live ? (double)s[(size_t)c * m + k] - (double)mu[c] : 0.0;
        nrm += d * d;
    }
    const double root = sqrt(nrm + kCosEps);
    double b = 0.0;
    for (int c0 = 0; c0 < cin; c0 += 32) {
        for (int j = 0; j < 32; ++j) {
            const double mc = (double)mu[c0 + j];
            const float v = live ? (float)(((double)s[(size_t)(c0 + j) * m + k] - mc) / root) : 0.f;
            b += mc * (double)v;
            tile[lane][j] = v;
        }
        __syncthreads();
        for (int r = lane >> 5; r < 64; r += 2) st_t[(size_t)(k0 + r) * cin + c0 + (lane & 31)] = tile[r][lane & 31];
        __syncthreads();
    }
    bias[k] = live ? (float)(0.0 - b) : -INFINITY;
}

struct CosineFinish {
    double weight = 1.0, count = 1.0;   // w and N
    float coef = 0.f;                   // w / N, rounded once
    float* loss_out = nullptr;
};

// blockIdx.x: a tile of CPX pixels, ALL channels - a gradient element needs p_i = <g_i, s^_k*> and |g_i|^2 over all C, so the tap
// and the gathered rows are read twice (the tap is L2-resident): once for the two sums, once for dF.
// Thread (row = tid >> 4, quad = tid & 15) owns pixels 4 quad .. 4 quad + 3 and channels row, row + 16 of every 32-channel chunk:
// it adds its channels in ascending order, then the 16 rows' sums are added in row order - the 16-byte and the scalar path do the
// same arithmetic in the same order, so a pixel's sums depend on C alone.
__global__ __launch_bounds__(256) void nearest_cosine_finish_kernel(const float* __restrict__ feat, const float* __restrict__ st_t,
                                                                    const float* __restrict__ mu, const float* __restrict__ part_score,
                                                                    const int* __restrict__ part_k, int splits, long long npix, int cin,
                                                                    long long m, int* __restrict__ idx_out, float* __restrict__ grad,
                                                                    float* __restrict__ partials, LastBlock lb, CosineFinish fin, int vec_ok) {
#pragma clang fp contract(off)
    __shared__ int ksel[CPX];
    __shared__ __attribute__((aligned(16))) float tile[32][CTP];
    __shared__ float psum[16][CPX], qsum[16][CPX];
    __shared__ float pfin[CPX], ifin[CPX];
    __shared__ float scratch[4];
    __shared__ bool is_last;
    __shared__ double sums[256];
    const int tid = threadIdx.x;
    const long long px0 = (long long)blockIdx.x * CPX;
    if (tid < CPX) {
        const long long px = px0 + tid;
        int k = 0;
        if (px < npix) {
            merge_splits(part_score, part_k, splits, npix, m, px, &k);
            idx_out[px] = k;
        }
        ksel[tid] = k;
    }
    __syncthreads();
    const int quad = tid & 15, row = tid >> 4;
    const long long px = px0 + 4 * quad;
    const bool wide = vec_ok && px + 3 < npix;
    const int nchunks = cin / KC;
    // thread (pixel tid >> 2, quarter tid & 3) reads 8 consecutive channels of its pixel's row of s^T
    auto gather = [&](int c0) {
        const int gp = tid >> 2, gq = tid & 3;
        const float* src = st_t + (size_t)ksel[gp] * cin + c0 + gq * 8;
        const f32x4 lo = *reinterpret_cast<const f32x4*>(src), hi = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            tile[gq * 8 + e][gp] = lo[e];
            tile[gq * 8 + 4 + e][gp] = hi[e];
        }
    };
    auto load4 = [&](const float* at) {
        f32x4 v;
        if (wide) {
            v = *reinterpret_cast<const f32x4*>(at);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (px + e < npix) ? at[e] : 0.f;
        }
        return v;
    };
    float p[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
    for (int ch = 0; ch < nchunks; ++ch) {
        const int c0 = ch * KC;
        gather(c0);
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int cl = row + 16 * e;
            const f32x4 f = load4(feat + (size_t)(c0 + cl) * npix + px);
            const float mc = mu[c0 + cl];
            const f32x4 sv = *reinterpret_cast<const f32x4*>(&tile[cl][4 * quad]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float g = f[j] - mc;
                p[j] += g * sv[j];
                q[j] += g * g;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        psum[row][4 * quad + j] = p[j];
        qsum[row][4 * quad + j] = q[j];
    }
    __syncthreads();
    float acc = 0.f;
    if (tid < CPX) {
        float ps = 0.f, qs = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            ps += psum[r][tid];
            qs += qsum[r][tid];
        }
        const float r = sqrtf(qs + kNearestCosineEps);
        pfin[tid] = ps;
        ifin[tid] = 1.f / r;
        if (px0 + tid < npix) acc = 1.f - ps / r;
    }
    __syncthreads();
    float ir[4], a[4];                    // 1 / r and p / r^3
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        ir[j] = ifin[4 * quad + j];
        a[j] = pfin[4 * quad + j] * ir[j] * ir[j] * ir[j];
    }
    for (int ch = 0; ch < nchunks; ++ch) {
        const int c0 = ch * KC;
        gather(c0);
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int cl = row + 16 * e;
            float* out = grad + (size_t)(c0 + cl) * npix + px;
            const f32x4 f = load4(feat + (size_t)(c0 + cl) * npix + px);
            const float mc = mu[c0 + cl];
            const f32x4 sv = *reinterpret_cast<const f32x4*>(&tile[cl][4 * quad]);
            f32x4 d;
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j] = fin.coef * (a[j] * (f[j] - mc) - sv[j] * ir[j]);
            if (wide) {
                *reinterpret_cast<f32x4*>(out) = d;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (px + j < npix) out[j] = d[j];
            }
        }
        __syncthreads();
    }
    acc = block_sum_256(acc, scratch);
    const float part[1] = {acc};
    if (!last_block_arrives(lb, &is_last, partials + blockIdx.x, part)) return;
    // the last block: thread t adds partials [t per, (t + 1) per) in index order, thread 0 the 256 sums in thread order
    const long long blocks = gridDim.x, per = (blocks + 255) / 256;
    double mine = 0.0;
    for (long long i = tid * per; i < blocks && i < (tid + 1) * per; ++i) mine += (double)partials[i];
    sums[tid] = mine;
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (int i = 0; i < 256; ++i) total += sums[i];
        fin.loss_out[0] = (float)(fin.weight * total / fin.count);
    }
}

long long round_up(long long v, long long to) { return (v + to - 1) / to * to; }

long long finish_blocks(int channels, long long n) {
    return ((n + FPX - 1) / FPX) * ((channels / KC + FCH - 1) / FCH);
}

}  // namespace

long long nearest_m_pad(long long m) { return round_up(m, TK); }

// The split count depends on the shape alone: a split owns at least kNearestMinTiles k tiles, and there are at most as many
// splits as give the chip about 1024 workgroups with the pixel tiles (64 at the most).
int nearest_splits(long long n, long long m, int* tiles_per_split) {
    const long long ktiles = nearest_m_pad(m) / TK, ptiles = (n + TPX - 1) / TPX;
    const long long max_splits = std::min<long long>(64, std::max<long long>(1, 1024 / ptiles));
    const long long per = std::max<long long>(kNearestMinTiles, (ktiles + max_splits - 1) / max_splits);
    if (tiles_per_split) *tiles_per_split = (int)per;
    return (int)((ktiles + per - 1) / per);
}

int nearest_check_shape(const char* who, int channels, long long n, long long m) {
    ST_REQUIRE(channels >= KC && channels % KC == 0, "%s: %d channels: a multiple of %d (the search kernel's K chunk)", who, channels, KC);
    ST_REQUIRE(n >= 1 && m >= 1, "%s: %lld pixels against %lld style vectors: at least one of each", who, n, m);
    ST_REQUIRE(nearest_m_pad(m) <= 0x7fffff00ll && (n + TPX - 1) / TPX <= 0x7fffffffll && finish_blocks(channels, n) <= 0x7fffffffll,
               "%s: %lld pixels against %lld style vectors of %d channels do not fit one launch", who, n, m, channels);
    return 0;
}

long long nearest_prepared_floats(int channels, long long m) {
    const long long m_pad = nearest_m_pad(m);
    return kAmaxWordUints + m_pad + m_pad * channels;
}

NearestPrepared nearest_prepared_of(float* prepared, int channels, long long m) {
    NearestPrepared pr;
    pr.m = m;
    pr.m_pad = nearest_m_pad(m);
    pr.bound = reinterpret_cast<unsigned int*>(prepared);
    pr.bias = prepared + kAmaxWordUints;
    pr.st_t = pr.bias + pr.m_pad;
    pr.mu = pr.st_t + pr.m_pad * channels;      // inside the buffer only for nearest_cosine_prepared_floats; L2 never reads it
    return pr;
}

long long nearest_scratch_floats(int channels, long long n, long long m) {
    const long long splits = nearest_splits(n, m, nullptr);
    return 64 + kAmaxWordUints + round_up(finish_blocks(channels, n), 64) + 2 * round_up(splits * n, 64);
}

NearestScratch nearest_scratch_of(float* scratch, int channels, long long n, long long m) {
    NearestScratch sc;
    sc.splits = nearest_splits(n, m, &sc.tiles_per_split);
    sc.ticket = reinterpret_cast<unsigned int*>(scratch);
    sc.bound = reinterpret_cast<unsigned int*>(scratch + 64);
    sc.partials = scratch + 64 + kAmaxWordUints;
    sc.part_score = sc.partials + round_up(finish_blocks(channels, n), 64);
    sc.part_k = reinterpret_cast<int*>(sc.part_score + round_up((long long)sc.splits * n, 64));
    return sc;
}

int launch_nearest_prepare(const float* vectors, int channels, long long m, const NearestPrepared& pr, hipStream_t s) {
    if (nearest_check_shape("launch_nearest_prepare", channels, 1, m)) return 1;
    ST_REQUIRE((reinterpret_cast<uintptr_t>(pr.st_t) & 15) == 0, "launch_nearest_prepare: the prepared buffer is not 16-byte aligned");
    hipLaunchKernelGGL(nearest_transpose_kernel, dim3((unsigned)(pr.m_pad / 32), (unsigned)(channels / 32)), dim3(256), 0, s, vectors,
                       channels, m, pr.st_t);
    ST_LAUNCH_CHECK();
    hipLaunchKernelGGL(nearest_bias_kernel, dim3((unsigned)((pr.m_pad + 255) / 256)), dim3(256), 0, s, pr.st_t, channels, m, pr.m_pad, pr.bias);
    ST_LAUNCH_CHECK();
    ST_HIP(hipMemsetAsync(pr.bound, 0, kAmaxWordUints * sizeof(unsigned int), s));
    return launch_amax(pr.st_t, pr.m_pad * channels, pr.bound, 0, s);
}

int launch_nearest_search(const float* feat, int channels, long long n, const NearestPrepared& pr, const NearestScratch& sc,
                          const unsigned int* feat_bound, hipStream_t s) {
    if (nearest_check_shape("launch_nearest_search", channels, n, pr.m)) return 1;
    if (!feat_bound) {          // a tensor no trunk kernel wrote: cleared and measured first, as the standalone heads do
        ST_HIP(hipMemsetAsync(sc.bound, 0, kAmaxWordUints * sizeof(unsigned int), s));
        if (launch_amax(feat, (long long)channels * n, sc.bound, 0, s)) return 1;
        feat_bound = sc.bound;
    }
    const int vec_ok = n % 4 == 0 && (reinterpret_cast<uintptr_t>(feat) & 15) == 0;
    const dim3 grid((unsigned)((n + TPX - 1) / TPX), (unsigned)sc.splits);
    hipLaunchKernelGGL(nearest_search_kernel, grid, dim3(256), 0, s, feat, pr.st_t, pr.bias, channels, n, (int)(pr.m_pad / TK),
                       sc.tiles_per_split, feat_bound, pr.bound, sc.part_score, sc.part_k, vec_ok);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_nearest_finish(const float* feat, int channels, long long n, const NearestPrepared& pr, const NearestScratch& sc, float weight,
                          int* idx_out, float* score_out, float* grad, float* loss_out, hipStream_t s) {
    const double count = (double)channels * (double)n;
    NearestFinish fin;
    fin.weight = (double)weight;
    fin.count = count;
    fin.coef = (float)((double)weight * 2.0 / count);
    fin.loss_out = loss_out;
    const int cgroups = (channels / KC + FCH - 1) / FCH;
    hipLaunchKernelGGL(nearest_finish_kernel, dim3((unsigned)finish_blocks(channels, n)), dim3(256), 0, s, feat, pr.st_t, sc.part_score,
                       sc.part_k, sc.splits, n, channels, pr.m, cgroups, idx_out, score_out, grad, sc.partials, last_block(sc.ticket), fin);
    ST_LAUNCH_CHECK();
    return 0;
}

int nearest_head_run(const float* feat, int channels, long long n, const NearestPrepared& pr, const NearestScratch& sc,
                     const unsigned int* feat_bound, float weight, int* idx_out, float* score_out, float* grad, float* loss_out,
                     hipStream_t s) {
    if (launch_nearest_search(feat, channels, n, pr, sc, feat_bound, s)) return 1;
    return launch_nearest_finish(feat, channels, n, pr, sc, weight, idx_out, score_out, grad, loss_out, s);
}

long long nearest_cosine_prepared_floats(int channels, long long m) { return nearest_prepared_floats(channels, m) + round_up(channels, 64); }

long long nearest_cosine_scratch_floats(int channels, long long n, long long m) { return nearest_scratch_floats(channels, n, m); }

int launch_nearest_cosine_prepare(const float* vectors, int channels, long long m, int centered, const NearestPrepared& pr, hipStream_t s) {
    if (nearest_check_shape("launch_nearest_cosine_prepare", channels, 1, m)) return 1;
    ST_REQUIRE((reinterpret_cast<uintptr_t>(pr.st_t) & 15) == 0, "launch_nearest_cosine_prepare: the prepared buffer is not 16-byte aligned");
    hipLaunchKernelGGL(cosine_mean_kernel, dim3((unsigned)round_up(channels, 64)), dim3(64), 0, s, vectors, channels, m, centered, pr.mu);
    ST_LAUNCH_CHECK();
    hipLaunchKernelGGL(cosine_rows_kernel, dim3((unsigned)(pr.m_pad / 64)), dim3(64), 0, s, vectors, pr.mu, channels, m, pr.st_t, pr.bias);
    ST_LAUNCH_CHECK();
    ST_HIP(hipMemsetAsync(pr.bound, 0, kAmaxWordUints * sizeof(unsigned int), s));
    return launch_amax(pr.st_t, pr.m_pad * channels, pr.bound, 0, s);
}

int nearest_cosine_head_run(const float* feat, int channels, long long n, const NearestPrepared& pr, const NearestScratch& sc,
                            const unsigned int* feat_bound, float weight, int* idx_out, float* grad, float* loss_out, hipStream_t s) {
    if (launch_nearest_search(feat, channels, n, pr, sc, feat_bound, s)) return 1;
    CosineFinish fin;
    fin.weight = (double)weight;
    fin.count = (double)n;
    fin.coef = (float)((double)weight / (double)n);
    fin.loss_out = loss_out;
    const int vec_ok = n % 4 == 0 && ((reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(grad)) & 15) == 0;
    hipLaunchKernelGGL(nearest_cosine_finish_kernel, dim3((unsigned)((n + CPX - 1) / CPX)), dim3(256), 0, s, feat, pr.st_t, pr.mu,
                       sc.part_score, sc.part_k, sc.splits, n, channels, pr.m, idx_out, grad, sc.partials, last_block(sc.ticket), fin, vec_ok);
    ST_LAUNCH_CHECK();
    return 0;
}

}  // namespace st

using namespace st;

extern "C" {

int st_op_nearest_k_chunk(void) { return kNearestChunk; }
int st_op_nearest_pixel_tile(void) { return kNearestPixelTile; }
int st_op_nearest_k_tile(void) { return kNearestKTile; }

int st_op_nearest_splits(long long n, long long m) {
    if (n < 1 || m < 1) return 0;
    return nearest_splits(n, m, nullptr);
}

long long st_op_nearest_prepared_floats(int channels, long long m) {
    if (channels < 1 || m < 1) return 0;
    return nearest_prepared_floats(channels, m);
}

long long st_op_nearest_scratch_floats(int channels, long long n, long long m) {
    if (channels < 1 || n < 1 || m < 1) return 0;
    return nearest_scratch_floats(channels, n, m);
}

int st_op_nearest_prepare(const float* vectors, int channels, long long m, float* prepared, void* stream) {
    ST_REQUIRE(vectors && prepared, "st_op_nearest_prepare: null argument");
    ST_REQUIRE((reinterpret_cast<uintptr_t>(prepared) & 255) == 0, "st_op_nearest_prepare: prepared must be 256-byte aligned");
    if (nearest_check_shape("st_op_nearest_prepare", channels, 1, m)) return 1;
    return launch_nearest_prepare(vectors, channels, m, nearest_prepared_of(prepared, channels, m), static_cast<hipStream_t>(stream));
}

int st_op_nearest_search(const float* feat, int channels, long long n, const float* prepared, long long m, float* scratch, int* idx_out,
                         float* score_out, void* stream) {
    ST_REQUIRE(feat && prepared && scratch && idx_out, "st_op_nearest_search: null argument");
    ST_REQUIRE((reinterpret_cast<uintptr_t>(prepared) & 255) == 0, "st_op_nearest_search: prepared must be 256-byte aligned");
    ST_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 255) == 0, "st_op_nearest_search: scratch must be 256-byte aligned");
    if (nearest_check_shape("st_op_nearest_search", channels, n, m)) return 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const NearestPrepared pr = nearest_prepared_of(const_cast<float*>(prepared), channels, m);
    const NearestScratch sc = nearest_scratch_of(scratch, channels, n, m);
    if (launch_nearest_search(feat, channels, n, pr, sc, nullptr, s)) return 1;
    hipLaunchKernelGGL(nearest_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, sc.part_score, sc.part_k, sc.splits, n, pr.m,
                       idx_out, score_out);
    ST_LAUNCH_CHECK();
    return 0;
}

int st_op_nearest_loss(const float* feat, int channels, long long n, const float* prepared, long long m, float* scratch, int* idx_out,
                       float* unit_grad_out, float* loss_out, void* stream) {
    ST_REQUIRE(feat && prepared && scratch && idx_out && unit_grad_out && loss_out, "st_op_nearest_loss: null argument");
    ST_REQUIRE((reinterpret_cast<uintptr_t>(prepared) & 255) == 0, "st_op_nearest_loss: prepared must be 256-byte aligned");
    ST_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 255) == 0, "st_op_nearest_loss: scratch must be 256-byte aligned");
    if (nearest_check_shape("st_op_nearest_loss", channels, n, m)) return 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    ST_HIP(hipMemsetAsync(scratch, 0, 16, s));
    return nearest_head_run(feat, channels, n, nearest_prepared_of(const_cast<float*>(prepared), channels, m),
                            nearest_scratch_of(scratch, channels, n, m), nullptr, 1.f, idx_out, nullptr, unit_grad_out, loss_out, s);
}

long long st_op_nearest_cosine_prepared_floats(int channels, long long m) {
    if (channels < 1 || m < 1) return 0;
    return nearest_cosine_prepared_floats(channels, m);
}

long long st_op_nearest_cosine_scratch_floats(int channels, long long n, long long m) {
    if (channels < 1 || n < 1 || m < 1) return 0;
    return nearest_cosine_scratch_floats(channels, n, m);
}

int st_op_nearest_cosine_prepare(const float* vectors, int channels, long long m, int centered, float* prepared, void* stream) {
    ST_REQUIRE(vectors && prepared, "st_op_nearest_cosine_prepare: null argument");
    ST_REQUIRE(centered == 0 || centered == 1, "st_op_nearest_cosine_prepare: centered %d: 0 (cosine) or 1 (centered_cosine)", centered);
    ST_REQUIRE((reinterpret_cast<uintptr_t>(prepared) & 255) == 0, "st_op_nearest_cosine_prepare: prepared must be 256-byte aligned");
    if (nearest_check_shape("st_op_nearest_cosine_prepare", channels, 1, m)) return 1;
    ST_REQUIRE_PIXELS("st_op_nearest_cosine_prepare (style vectors)", m);
    return launch_nearest_cosine_prepare(vectors, channels, m, centered, nearest_prepared_of(prepared, channels, m),
                                         static_cast<hipStream_t>(stream));
}

int st_op_nearest_cosine_loss(const float* feat, int channels, long long n, const float* prepared, long long m, float* scratch, int* idx_out,
                              float* unit_grad_out, float* loss_out, void* stream) {
    ST_REQUIRE(feat && prepared && scratch && idx_out && unit_grad_out && loss_out, "st_op_nearest_cosine_loss: null argument");
    ST_REQUIRE((reinterpret_cast<uintptr_t>(prepared) & 255) == 0, "st_op_nearest_cosine_loss: prepared must be 256-byte aligned");
    ST_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 255) == 0, "st_op_nearest_cosine_loss: scratch must be 256-byte aligned");
    if (nearest_check_shape("st_op_nearest_cosine_loss", channels, n, m)) return 1;
    ST_REQUIRE_PIXELS("st_op_nearest_cosine_loss", n);
    ST_REQUIRE_PIXELS("st_op_nearest_cosine_loss (style vectors)", m);
    hipStream_t s = static_cast<hipStream_t>(stream);
    ST_HIP(hipMemsetAsync(scratch, 0, 16, s));
    return nearest_cosine_head_run(feat, channels, n, nearest_prepared_of(const_cast<float*>(prepared), channels, m),
                                   nearest_scratch_of(scratch, channels, n, m), nullptr, 1.f, idx_out, unit_grad_out, loss_out, s);
}

int st_op_nearest_loss_backward(const float* unit_grad, long long count, const float* upstream, float* grad, void* stream) {
    ST_REQUIRE(unit_grad && upstream && grad && count >= 1, "st_op_nearest_loss_backward: null argument or empty tensor");
    hipLaunchKernelGGL(nearest_scale_kernel, dim3((unsigned)std::min<long long>(1024, (count + 1023) / 1024)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), unit_grad, upstream, count, grad);
    ST_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
