// StyleLossW2 with both covariances restricted to their diagonals (st_plan_set_w2_diagonal, losses.StyleLossW2Diag): for two
// Gaussians with diagonal covariances W2^2 = sum_c (mu - mu_t)^2 + sum_c (sigma - sigma_t)^2, the mean / standard-deviation
// loss of Li et al., "Demystifying Neural Style Transfer".  On a tap F [C][npix] with pixel weights m_p, M = sum m_p:
//   mu_c = sum_p m_p f_cp / M,  q_c = sum_p m_p f_cp^2 / M,  v_c = max(q_c - mu_c^2, 0) + eps,  sigma_c = sqrt(v_c)
//   term = w (sum_c (mu_c - mut_c)^2 + sum_c (sigma_c - sigmat_c)^2) / C
//   dF_cp = w (m_p / M) ((2 / C) (mu_c - mut_c) + 2 g_c (f_cp - mu_c)),  g_c = (1 - sigmat_c / sigma_c) / C  (0 where sigma_c = 0)
// The variance term is (sigma - sigma_t)^2 and not v + v_t - 2 sqrt(v v_t): at the target it is exactly 0 with an exactly zero
// gradient.  No C x C work anywhere: two memory-bound launches per head.
//   channel_stats_kernel        one read of the tap: per (channel, split) workgroup two fp32 partials, sum m f and sum m f^2; the
//                               last block by ticket (LastBlock, st_common.h) adds each channel's partials in split order in
//                               double and forms mu, v, sigma, the term's two sums in channel order and, per channel,
//                               a_c = 2 w g_c / M and b_c = w (2 / C) (mu_c - mut_c) / M - a_c mu_c
//   channel_affine_grad_kernel  one read and one write (ACC: and one more read): g_cp = (a_c f_cp + b_c) m_p
// No floating-point atomics, and the split count is a function of the shape alone: two runs give the same bits.  The same code
// serves fp16x3 and fp32 plans; no bound word is read or committed (run_tap_backward's seeding commits the seed's).
#include <algorithm>
#include <cstdint>

#include "../../include/st_amd.h"
#include "st_common.h"

namespace st {

namespace {

constexpr long long kStatsSplitPixels = 4096;     // a split holds about this many pixels: 16 per thread ...
constexpr int kStatsMaxSplits = 64;               // ... until 64 splits per channel, which then grow

template <bool MASKED>
__global__ __launch_bounds__(256) void channel_stats_kernel(const float* __restrict__ feat, const float* __restrict__ sqrt_mask,
                                                            int channels, long long npix, int splits, int vec,
                                                            float* __restrict__ partials, LastBlock lb, ChannelStatsFinish fin) {
#pragma clang fp contract(off)
    __shared__ float scratch[4];
    __shared__ bool is_last;
    __shared__ double dm_sh[256], ds_sh[256];
    const int c = (int)blockIdx.x / splits, k = (int)blockIdx.x % splits;
    const float* row = feat + (long long)c * npix;
    float s1 = 0.f, s2 = 0.f;
    if (vec) {                        // 16-byte accesses: npix % 4 == 0, so every channel row starts on a 16-byte boundary
        const long long n4 = npix >> 2, chunk = (n4 + splits - 1) / splits;
        const long long lo = (long long)k * chunk, hi = lo + chunk < n4 ? lo + chunk : n4;
        const f32x4* f4 = reinterpret_cast<const f32x4*>(row);
        const f32x4* m4 = reinterpret_cast<const f32x4*>(sqrt_mask);
        for (long long i = lo + threadIdx.x; i < hi; i += 256) {
            const f32x4 f = f4[i];
            f32x4 r;
            if (MASKED) r = m4[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float mf = MASKED ? (r[e] * r[e]) * f[e] : f[e];
                s1 += mf;
                s2 += mf * f[e];
            }
        }
    } else {
        const long long chunk = (npix + splits - 1) / splits;
        const long long lo = (long long)k * chunk, hi = lo + chunk < npix ? lo + chunk : npix;
        for (long long i = lo + threadIdx.x; i < hi; i += 256) {
            const float f = row[i];
            float mf = f;
            if (MASKED) { const float r = sqrt_mask[i]; mf = (r * r) * f; }
            s1 += mf;
            s2 += mf * f;
        }
    }
    s1 = block_sum_256(s1, scratch);
    s2 = block_sum_256(s2, scratch);
    const float mine[2] = {s1, s2};   // [c][split][2]
    if (!last_block_arrives(lb, &is_last, partials + 2 * blockIdx.x, mine)) return;
    // the last block: a thread per channel, 256 channels at a time; thread 0 adds their contributions in channel order
    double t_mean = 0.0, t_std = 0.0;
    for (int base = 0; base < channels; base += 256) {
        const int ch = base + (int)threadIdx.x;
        double dm = 0.0, ds = 0.0;
        if (ch < channels) {
            double a1 = 0.0, a2 = 0.0;
            for (int i = 0; i < splits; ++i) {
                a1 += (double)partials[2 * (ch * splits + i)];
                a2 += (double)partials[2 * (ch * splits + i) + 1];
            }
            const double mu = a1 / fin.norm, q = a2 / fin.norm;
            if (fin.mean_out) fin.mean_out[ch] = (float)mu;
            if (fin.srm_out) fin.srm_out[ch] = (float)q;
            if (fin.mean_t) {
                const double var = q - mu * mu;
                const double sg = sqrt((var > 0.0 ? var : 0.0) + (double)fin.eps);
                const double dmu = mu - (double)fin.mean_t[ch], st = (double)fin.std_t[ch];
                const double dsg = sg - st;
                dm = dmu * dmu;
                ds = dsg * dsg;
                const double w = (double)fin.weight;
                const double g = sg > 0.0 ? (1.0 - st / sg) / (double)channels : 0.0;
                const double a = 2.0 * w * g / fin.norm;
                fin.coeffs[ch] = (float)a;
                fin.coeffs[channels + ch] = (float)(w * (2.0 / (double)channels) * dmu / fin.norm - a * mu);
            }
        }
        dm_sh[threadIdx.x] = dm;
        ds_sh[threadIdx.x] = ds;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int count = channels - base < 256 ? channels - base : 256;
            for (int i = 0; i < count; ++i) {
                t_mean += dm_sh[i];
                t_std += ds_sh[i];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && fin.loss_out) fin.loss_out[0] = (float)((double)fin.weight * (t_mean + t_std) / (double)channels);
}

// one workgroup column per channel (blockIdx.y), a grid-stride loop over its pixels: one owner per element
template <bool MASKED, bool ACC>
__global__ __launch_bounds__(256) void channel_affine_grad_kernel(const float* __restrict__ feat, const float* __restrict__ sqrt_mask,
                                                                  const float* __restrict__ coeffs, const float* __restrict__ upstream,
                                                                  int channels, long long npix, int vec, float* __restrict__ grad) {
#pragma clang fp contract(off)
    const int c = (int)blockIdx.y;
    float a = coeffs[c], b = coeffs[channels + c];
    if (upstream) {
        const float u = upstream[0];
        a *= u;
        b *= u;
    }
    const float* row = feat + (long long)c * npix;
    float* out = grad + (long long)c * npix;
    if (vec) {
        const long long n4 = npix >> 2;
        const f32x4* f4 = reinterpret_cast<const f32x4*>(row);
        const f32x4* m4 = reinterpret_cast<const f32x4*>(sqrt_mask);
        f32x4* g4 = reinterpret_cast<f32x4*>(out);
        for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
            const f32x4 f = f4[i];
            f32x4 r, g;
            if (MASKED) r = m4[i];
            if (ACC) g = g4[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = a * f[e] + b;
                if (MASKED) v = v * (r[e] * r[e]);
                g[e] = ACC ? g[e] + v : v;
            }
            g4[i] = g;
        }
    } else {
        for (long long i = blockIdx.x * 256ll + threadIdx.x; i < npix; i += (long long)gridDim.x * 256) {
            float v = a * row[i] + b;
            if (MASKED) { const float r = sqrt_mask[i]; v = v * (r * r); }
            out[i] = ACC ? out[i] + v : v;
        }
    }
}

__global__ __launch_bounds__(256) void diag_target_kernel(const float* __restrict__ mean, const float* __restrict__ srm, int n, float eps,
                                                          float* __restrict__ mean_t, float* __restrict__ std_t) {
#pragma clang fp contract(off)
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    const double mu = (double)mean[c];
    const double var = (double)srm[(long long)c * n + c] - mu * mu;
    mean_t[c] = mean[c];
    std_t[c] = (float)sqrt((var > 0.0 ? var : 0.0) + (double)eps);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the shapes both launches take: a 1-D grid of channels x splits, and a channel per grid row
int check_shape(const char* who, int channels, long long npix) {
    ST_REQUIRE(channels >= 1 && channels <= 65535 && npix >= 1 && (long long)channels * kStatsMaxSplits < (1ll << 30),
               "%s: %d channels of %lld pixels: 1 to 65535 channels of at least one pixel", who, channels, npix);
    ST_REQUIRE_PIXELS(who, npix);
    return 0;
}

}  // namespace

int channel_stats_splits(long long npix) {
    return (int)std::min<long long>(kStatsMaxSplits, std::max<long long>(1, (npix + kStatsSplitPixels - 1) / kStatsSplitPixels));
}

long long channel_stats_scratch_floats(int channels, long long npix) { return 4 + 2ll * channels * channel_stats_splits(npix); }

int launch_channel_stats(const float* feat, const float* sqrt_mask, int channels, long long npix, float* scratch,
                         const ChannelStatsFinish& fin, hipStream_t s) {
    if (check_shape("launch_channel_stats", channels, npix)) return 1;
    const int splits = channel_stats_splits(npix);
    const int vec = (npix & 3) == 0 && aligned16(feat) && (!sqrt_mask || aligned16(sqrt_mask));
    const LastBlock lb = last_block(reinterpret_cast<unsigned int*>(scratch));
    const dim3 grid((unsigned)(channels * splits));
    if (sqrt_mask)
        hipLaunchKernelGGL(channel_stats_kernel<true>, grid, dim3(256), 0, s, feat, sqrt_mask, channels, npix, splits, vec, scratch + 4, lb, fin);
    else
        hipLaunchKernelGGL(channel_stats_kernel<false>, grid, dim3(256), 0, s, feat, sqrt_mask, channels, npix, splits, vec, scratch + 4, lb, fin);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_channel_affine_grad(const float* feat, const float* sqrt_mask, const float* coeffs, const float* upstream, int channels,
                               long long npix, float* grad, int accumulate, hipStream_t s) {
    if (check_shape("launch_channel_affine_grad", channels, npix)) return 1;
    const int vec = (npix & 3) == 0 && aligned16(feat) && aligned16(grad) && (!sqrt_mask || aligned16(sqrt_mask));
    const long long items = vec ? npix >> 2 : npix;
    const dim3 grid((unsigned)std::min<long long>(64, (items + 255) / 256), (unsigned)channels);
#define ST_AFFINE_GRAD(MASKED, ACC)                                                                                                 \
    hipLaunchKernelGGL((channel_affine_grad_kernel<MASKED, ACC>), grid, dim3(256), 0, s, feat, sqrt_mask, coeffs, upstream, channels, \
                       npix, vec, grad)
    if (sqrt_mask) {
        if (accumulate) ST_AFFINE_GRAD(true, true); else ST_AFFINE_GRAD(true, false);
    } else {
        if (accumulate) ST_AFFINE_GRAD(false, true); else ST_AFFINE_GRAD(false, false);
    }
#undef ST_AFFINE_GRAD
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_diag_target(const float* mean, const float* srm, int n, float eps, float* mean_t, float* std_t, hipStream_t s) {
    hipLaunchKernelGGL(diag_target_kernel, dim3((n + 255) / 256), dim3(256), 0, s, mean, srm, n, eps, mean_t, std_t);
    ST_LAUNCH_CHECK();
    return 0;
}

}  // namespace st

using namespace st;

extern "C" {

long long st_op_channel_stats_scratch_floats(int channels, long long npix) {
    if (channels < 1 || npix < 1) return 0;
    return channel_stats_scratch_floats(channels, npix);
}

int st_op_channel_moments(const float* feat, int channels, long long npix, float* scratch, float* mean_out, float* srm_diag_out,
                          void* stream) {
    ST_REQUIRE(feat && scratch && mean_out && srm_diag_out, "st_op_channel_moments: null argument");
    if (check_shape("st_op_channel_moments", channels, npix)) return 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    ChannelStatsFinish fin;
    fin.norm = (double)npix;
    fin.mean_out = mean_out;
    fin.srm_out = srm_diag_out;
    ST_HIP(hipMemsetAsync(scratch, 0, 4 * sizeof(float), s));
    return launch_channel_stats(feat, nullptr, channels, npix, scratch, fin, s);
}

int st_op_w2_diag_loss(const float* feat, int channels, long long npix, const float* mean_t, const float* std_t, float eps,
                       float* scratch, float* coeffs_out, float* loss_out, void* stream) {
    ST_REQUIRE(feat && mean_t && std_t && scratch && coeffs_out && loss_out, "st_op_w2_diag_loss: null argument");
    ST_REQUIRE(eps >= 0.f, "st_op_w2_diag_loss: eps %g is negative", (double)eps);
    hipStream_t s = static_cast<hipStream_t>(stream);
    ChannelStatsFinish fin;
    fin.mean_t = mean_t;
    fin.std_t = std_t;
    fin.eps = eps;
    fin.weight = 1.f;
    fin.norm = (double)npix;
    fin.coeffs = coeffs_out;
    fin.loss_out = loss_out;
    ST_HIP(hipMemsetAsync(scratch, 0, 4 * sizeof(float), s));
    return launch_channel_stats(feat, nullptr, channels, npix, scratch, fin, s);
}

int st_op_w2_diag_loss_backward(const float* feat, int channels, long long npix, const float* coeffs, const float* upstream,
                                float* grad, void* stream) {
    ST_REQUIRE(feat && coeffs && upstream && grad, "st_op_w2_diag_loss_backward: null argument");
    return launch_channel_affine_grad(feat, nullptr, coeffs, upstream, channels, npix, grad, 0, static_cast<hipStream_t>(stream));
}

}  // extern "C"
