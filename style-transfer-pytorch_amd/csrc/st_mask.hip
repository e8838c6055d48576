// Spatial masks for the style statistics (st_plan_set_style_mask): stylize only a part of the picture, or take the style
// from only a part of a style image.  The style loss depends on a tap F [C][N] only through (mean, srm), so a mask m in
// [0, 1] per pixel enters as WEIGHTED moments at the tap's resolution,
//   mean_m = sum_p m_p f_p / M,   srm_m = sum_p m_p f_p f_p^T / M,   M = sum_p m_p,
// in the place of StyleLossW2.get_target(input) (style_transfer.py:175-181) and of F F^T / N in StyleLoss.forward (:141-142),
// and as the weighted form of the heads' gradient step, dF = (Ssym F + b 1^T) diag(m) with M in the place of N in (Ssym, b).
// Targets, eps, weights, the Newton-Schulz chains and the Lyapunov backward never see it.
//
// The pyramid: a tap behind k poolings takes level k of the mask, the plain mean of the 2 x 2 cells of level k - 1 at floor
// sizes (avg_pool2d(m, 2) - the geometry of the trunk's pools whatever the pooling mode).  The plan keeps s = sqrt(m) per
// level: the Gram kernels put s on BOTH operands (st_gram.hip, MASKED), so they keep their symmetry, tile pairs, fp16x3 bound
// (s <= 1) and split sums, and no masked copy of a tap exists.  M_k is read back ONCE, by the setter (a cold path that
// validates the mask with the same read); the closures get it as a kernel argument.
//
// Here: the pyramid kernel, the pointwise kernel of the gradient step, and the two entry points.
#include <cmath>

#include "st_plan.h"

namespace st {
namespace {

// Level `lev` (blockIdx.y) of the pyramid.  Floor sizes: every cell of level k covers a 2^k x 2^k block of the mask that lies
// inside it, so a thread folds its cell from the mask itself - ((a + b) + (c + d)) / 4 per 2 x 2, level by level, in registers -
// and no level waits for another.  Sums: a thread's cells in grid-stride order, the workgroup's 256 in a fixed tree, the
// workgroups' partials by pyramid_finish_kernel in index order; double, which the few cells of a deep level deserve.
struct PyramidShape {
    int h[kMaskLevels], w[kMaskLevels];
    float* out[kMaskLevels];
};

template <int LEV>
__device__ __forceinline__ float pyramid_cell(const float* __restrict__ mask, int W, int y, int x) {
    if constexpr (LEV == 0) {
        return mask[(size_t)y * W + x];
    } else {
        const float a = pyramid_cell<LEV - 1>(mask, W, 2 * y, 2 * x), b = pyramid_cell<LEV - 1>(mask, W, 2 * y, 2 * x + 1);
        const float c = pyramid_cell<LEV - 1>(mask, W, 2 * y + 1, 2 * x), d = pyramid_cell<LEV - 1>(mask, W, 2 * y + 1, 2 * x + 1);
        return ((a + b) + (c + d)) * 0.25f;
    }
}

__global__ __launch_bounds__(256) void mask_pyramid_kernel(const float* __restrict__ mask, PyramidShape sh,
                                                           double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double red[4][256];
    const int lev = blockIdx.y;
    const int h = sh.h[lev], w = sh.w[lev], W = sh.w[0];
    const long long cells = (long long)h * w;
    float* __restrict__ out = sh.out[lev];
    double sum = 0.0, lo = 2.0, hi = -1.0, nans = 0.0;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < cells; i += (long long)gridDim.x * 256) {
        const int y = (int)(i / w), x = (int)(i % w);
        float v;
        switch (lev) {
            case 0: v = pyramid_cell<0>(mask, W, y, x); break;
            case 1: v = pyramid_cell<1>(mask, W, y, x); break;
            case 2: v = pyramid_cell<2>(mask, W, y, x); break;
            case 3: v = pyramid_cell<3>(mask, W, y, x); break;
            default: v = pyramid_cell<4>(mask, W, y, x); break;
        }
        out[i] = sqrtf(v);
        if (v != v) {
            nans += 1.0;
        } else {
            sum += (double)v;
            lo = (double)v < lo ? (double)v : lo;
            hi = (double)v > hi ? (double)v : hi;
        }
    }
    red[0][threadIdx.x] = sum;
    red[1][threadIdx.x] = lo;
    red[2][threadIdx.x] = hi;
    red[3][threadIdx.x] = nans;
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step) {
            const int o = threadIdx.x + step;
            red[0][threadIdx.x] += red[0][o];
            red[1][threadIdx.x] = red[1][o] < red[1][threadIdx.x] ? red[1][o] : red[1][threadIdx.x];
            red[2][threadIdx.x] = red[2][o] > red[2][threadIdx.x] ? red[2][o] : red[2][threadIdx.x];
            red[3][threadIdx.x] += red[3][o];
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) partials[((size_t)lev * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = red[threadIdx.x][0];
}

// stats[0..4] = the levels' sums, [5] min, [6] max, [7] NaN count of level 0 (the mask itself)
__global__ __launch_bounds__(64) void pyramid_finish_kernel(const double* __restrict__ partials, int blocks,
                                                            double* __restrict__ stats) {
    const int t = threadIdx.x;
    if (t < kMaskLevels) {
        double s = 0.0;
        for (int b = 0; b < blocks; ++b) s += partials[((size_t)t * blocks + b) * 4];
        stats[t] = s;
    } else if (t < kMaskLevels + 3) {
        const int what = t - kMaskLevels + 1;              // 1 min, 2 max, 3 NaNs - of level 0
        double r = partials[what];
        for (int b = 1; b < blocks; ++b) {
            const double v = partials[(size_t)b * 4 + what];
            r = what == 1 ? (v < r ? v : r) : what == 2 ? (v > r ? v : r) : r + v;
        }
        stats[t] = r;
    }
}

// buf [c][npix] flat: element i lies in pixel column i % npix.  16-byte groups of the FLAT buffer (always aligned, whatever
// npix is: a group may run over a row's end, its pixel index wraps), then the count % 4 elements behind them one at a time.
__global__ __launch_bounds__(256) void mask_columns_kernel(float* __restrict__ buf, const float* __restrict__ sqrt_mask,
                                                           long long count, long long npix) {
#pragma clang fp contract(off)
    const long long n4 = count / 4;
    const long long first = blockIdx.x * 256ll + threadIdx.x, stride = (long long)gridDim.x * 256;
    f32x4* buf4 = reinterpret_cast<f32x4*>(buf);
    for (long long i = first; i < n4; i += stride) {
        f32x4 v = buf4[i];
        long long px = (4 * i) % npix;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float sm = sqrt_mask[px];
            v[e] *= sm * sm;
            px = px + 1 == npix ? 0 : px + 1;
        }
        buf4[i] = v;
    }
    for (long long i = 4 * n4 + first; i < count; i += stride) {
        const float sm = sqrt_mask[i % npix];
        buf[i] *= sm * sm;
    }
}

}  // namespace

int launch_mask_pyramid(const float* mask, const int* h, const int* w, float* const* sqrt_level, double* partials, double* stats,
                        hipStream_t s) {
    PyramidShape sh{};
    for (int k = 0; k < kMaskLevels; ++k) {
        ST_REQUIRE(h[k] >= 1 && w[k] >= 1 && sqrt_level[k], "mask pyramid: level %d is empty", k);
        ST_REQUIRE(k == 0 || (h[k] == h[k - 1] / 2 && w[k] == w[k - 1] / 2), "mask pyramid: level %d is not the floor half of level %d", k, k - 1);
        sh.h[k] = h[k];
        sh.w[k] = w[k];
        sh.out[k] = sqrt_level[k];
    }
    hipLaunchKernelGGL(mask_pyramid_kernel, dim3(kMaskPyramidBlocks, kMaskLevels), dim3(256), 0, s, mask, sh, partials);
    ST_LAUNCH_CHECK();
    hipLaunchKernelGGL(pyramid_finish_kernel, dim3(1), dim3(64), 0, s, partials, kMaskPyramidBlocks, stats);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_mask_columns(float* buf, const float* sqrt_mask, int channels, long long npix, hipStream_t s) {
    ST_REQUIRE(buf && sqrt_mask && channels > 0 && npix > 0, "mask columns: bad argument");
    const long long count = (long long)channels * npix;
    long long blocks = (std::max(count / 4, count % 4) + 255) / 256;
    blocks = std::min(std::max(blocks, 1ll), (long long)kStreamBlocks);
    hipLaunchKernelGGL(mask_columns_kernel, dim3((unsigned)blocks), dim3(256), 0, s, buf, sqrt_mask, count, npix);
    ST_LAUNCH_CHECK();
    return 0;
}

}  // namespace st

using namespace st;

extern "C" {

int st_plan_set_style_mask(st_plan* p, const float* mask, void* stream) {
    ST_REQUIRE(p, "st_plan_set_style_mask: null plan");
    ST_REQUIRE(!p->strip, "st_plan_set_style_mask: strip plans take no style mask (a level's sum would span the ranks)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!mask) {
        if (p->style_mask) {
            p->style_mask = false;
            invalidate_graph(p);
        }
        return 0;
    }
    constexpr size_t kPartials = (size_t)kMaskLevels * kMaskPyramidBlocks * 4;
    if (!p->mask_stats) {
        p->mask_h[0] = p->H;
        p->mask_w[0] = p->W;
        for (int k = 1; k < kMaskLevels; ++k) {
            p->mask_h[k] = p->pool[k - 1].h;
            p->mask_w[k] = p->pool[k - 1].w;
        }
        for (int k = 0; k < kMaskLevels; ++k)
            if (plan_alloc(p, &p->mask_sqrt[k], (size_t)p->mask_h[k] * p->mask_w[k])) return 1;
        float* mem = nullptr;
        if (plan_alloc(p, &mem, 2 * (kPartials + 8))) return 1;
        p->mask_stats = reinterpret_cast<double*>(mem);
    }
    // the levels are overwritten whether or not the mask is then accepted: no mask is in force until it is
    p->style_mask = false;
    invalidate_graph(p);
    if (launch_mask_pyramid(mask, p->mask_h, p->mask_w, p->mask_sqrt, p->mask_stats, p->mask_stats + kPartials, s)) return 1;
    double stats[8];
    ST_HIP(hipMemcpyAsync(stats, p->mask_stats + kPartials, sizeof(stats), hipMemcpyDeviceToHost, s));
    ST_HIP(hipStreamSynchronize(s));
    ST_REQUIRE(stats[7] == 0.0, "st_plan_set_style_mask: the mask holds %.0f NaN value(s): a mask's values lie in [0, 1]", stats[7]);
    ST_REQUIRE(stats[5] >= 0.0 && stats[6] <= 1.0, "st_plan_set_style_mask: the mask's values span [%g, %g]: a mask's values lie in [0, 1]",
               stats[5], stats[6]);
    for (int k = 0; k < kMaskLevels; ++k) {
        ST_REQUIRE(stats[k] > 0.0,
                   "st_plan_set_style_mask: the mask's level %d (%d x %d, behind %d poolings) sums to 0: the style layers at that "
                   "level would have no pixel to take their statistics from", k, p->mask_h[k], p->mask_w[k], k);
        p->mask_sum[k] = stats[k];
    }
    p->style_mask = true;
    return 0;
}

int st_plan_style_mask(const st_plan* p, int level, const float** sqrt_mask, int* h, int* w, double* sum) {
    ST_REQUIRE(p, "st_plan_style_mask: null plan");
    ST_REQUIRE(p->style_mask, "st_plan_style_mask: no style mask is set on this plan (st_plan_set_style_mask)");
    ST_REQUIRE(level >= 0 && level < kMaskLevels, "st_plan_style_mask: level %d out of range (0 .. %d)", level, kMaskLevels - 1);
    if (sqrt_mask) *sqrt_mask = p->mask_sqrt[level];
    if (h) *h = p->mask_h[level];
    if (w) *w = p->mask_w[level];
    if (sum) *sum = p->mask_sum[level];
    return 0;
}

}  // extern "C"
