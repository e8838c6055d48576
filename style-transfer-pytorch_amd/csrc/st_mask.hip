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
//
// Style regions (st_plan_set_style_regions): R <= kMaxRegions masks with a style each - Gatys et al.'s guided transfer, the
// formulas above once per region.  Region r has a pyramid of its own (this file's kernel, one call per region: a given mask
// yields the bits it yields as a style mask), one target per listed style layer and a weight rho_r; the term of (region r,
// entry j) is entry j's module on region r's weighted moments against region r's target, times style_weight[j] rho_r.  An
// entry's term is the fp32 sum of its regions' terms in region order (sum_region_terms_kernel), and the tap's gradient
// sum_r (Ssym_r F + b_r 1^T) diag(m_r) is accumulated in region order: region 0 writes the seed and is multiplied by m_0 as a
// style mask is, region r >= 1 writes its 1x1 step into one scratch buffer and mask_columns_add_kernel adds m_r times it onto
// the seed - one owner per element, no atomics, so two closures give equal bits.  The closure's part is st_taps.hip's.
//
// Weight maps for the content and TV terms (st_plan_set_content_mask / st_plan_set_tv_mask): the same pyramid kernel with the
// levels stored as they are - all five for the content map, level 0 alone for the TV map (a bit-exact copy) - and validated by
// the same read-back.  The weighted terms themselves are st_pointwise.hip's kernels, launched by st_taps.hip.
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

// root == 0 (the content and TV weight maps, below): the level itself is stored in the place of its square root.
__global__ __launch_bounds__(256) void mask_pyramid_kernel(const float* __restrict__ mask, PyramidShape sh,
                                                           double* __restrict__ partials, int root) {
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
        out[i] = root ? sqrtf(v) : v;
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
// (levels: how many the pyramid kernel ran; the sums of the others are 0)
__global__ __launch_bounds__(64) void pyramid_finish_kernel(const double* __restrict__ partials, int blocks,
                                                            double* __restrict__ stats, int levels) {
    const int t = threadIdx.x;
    if (t < kMaskLevels) {
        double s = 0.0;
        for (int b = 0; t < levels && b < blocks; ++b) s += partials[((size_t)t * blocks + b) * 4];
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

// dst [c][npix] += sqrt_mask^2 * src per pixel column, with mask_columns_kernel's structure.  HBM-bound: two reads and one write
// of the tap (the level of the mask stays in L2), so the grid is capped at kStreamBlocks workgroups striding over the buffer.
__global__ __launch_bounds__(256) void mask_columns_add_kernel(float* __restrict__ dst, const float* __restrict__ src,
                                                               const float* __restrict__ sqrt_mask, long long count, long long npix) {
#pragma clang fp contract(off)
    const long long n4 = count / 4;
    const long long first = blockIdx.x * 256ll + threadIdx.x, stride = (long long)gridDim.x * 256;
    f32x4* dst4 = reinterpret_cast<f32x4*>(dst);
    const f32x4* src4 = reinterpret_cast<const f32x4*>(src);
    for (long long i = first; i < n4; i += stride) {
        f32x4 v = dst4[i];
        const f32x4 a = src4[i];
        long long px = (4 * i) % npix;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float sm = sqrt_mask[px];
            v[e] = v[e] + (sm * sm) * a[e];
            px = px + 1 == npix ? 0 : px + 1;
        }
        dst4[i] = v;
    }
    for (long long i = 4 * n4 + first; i < count; i += stride) {
        const float sm = sqrt_mask[i % npix];
        dst[i] = dst[i] + (sm * sm) * src[i];
    }
}

// the entries' terms from their regions' terms, in region order; one region: the bits as the head wrote them
__global__ __launch_bounds__(64) void sum_region_terms_kernel(const float* __restrict__ region_terms, int regions, int n_style,
                                                              float* __restrict__ out) {
#pragma clang fp contract(off)
    const int j = threadIdx.x;
    if (j >= n_style) return;
    float t = region_terms[j];
    for (int r = 1; r < regions; ++r) t = t + region_terms[(size_t)r * n_style + j];
    out[j] = t;
}

}  // namespace

int launch_mask_pyramid(const float* mask, const int* h, const int* w, float* const* sqrt_level, double* partials, double* stats,
                        hipStream_t s, bool store_root, int levels) {
    ST_REQUIRE(levels >= 1 && levels <= kMaskLevels, "mask pyramid: %d levels", levels);
    PyramidShape sh{};
    for (int k = 0; k < levels; ++k) {
        ST_REQUIRE(h[k] >= 1 && w[k] >= 1 && sqrt_level[k], "mask pyramid: level %d is empty", k);
        ST_REQUIRE(k == 0 || (h[k] == h[k - 1] / 2 && w[k] == w[k - 1] / 2), "mask pyramid: level %d is not the floor half of level %d", k, k - 1);
        sh.h[k] = h[k];
        sh.w[k] = w[k];
        sh.out[k] = sqrt_level[k];
    }
    hipLaunchKernelGGL(mask_pyramid_kernel, dim3(kMaskPyramidBlocks, levels), dim3(256), 0, s, mask, sh, partials, store_root ? 1 : 0);
    ST_LAUNCH_CHECK();
    hipLaunchKernelGGL(pyramid_finish_kernel, dim3(1), dim3(64), 0, s, partials, kMaskPyramidBlocks, stats, levels);
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

int launch_mask_columns_add(float* dst, const float* src, const float* sqrt_mask, int channels, long long npix, hipStream_t s) {
    ST_REQUIRE(dst && src && sqrt_mask && channels > 0 && npix > 0, "mask columns add: bad argument");
    const long long count = (long long)channels * npix;
    long long blocks = (std::max(count / 4, count % 4) + 255) / 256;
    blocks = std::min(std::max(blocks, 1ll), (long long)kStreamBlocks);
    hipLaunchKernelGGL(mask_columns_add_kernel, dim3((unsigned)blocks), dim3(256), 0, s, dst, src, sqrt_mask, count, npix);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_sum_region_terms(const float* region_terms, int regions, int n_style, float* out, hipStream_t s) {
    ST_REQUIRE(region_terms && out && regions >= 1 && regions <= kMaxRegions && n_style >= 0 && n_style <= 16,
               "sum region terms: bad argument");
    if (n_style == 0) return 0;
    hipLaunchKernelGGL(sum_region_terms_kernel, dim3(1), dim3(64), 0, s, region_terms, regions, n_style, out);
    ST_LAUNCH_CHECK();
    return 0;
}

namespace {

constexpr size_t kPyramidPartials = (size_t)kMaskLevels * kMaskPyramidBlocks * 4;

// the levels' sizes and the pyramid kernel's scratch: its partials and, behind them, 8 results per region (a style mask: the first 8)
int ensure_pyramid_scratch(st_plan* p) {
    if (p->mask_stats) return 0;
    p->mask_h[0] = p->H;
    p->mask_w[0] = p->W;
    for (int k = 1; k < kMaskLevels; ++k) {
        p->mask_h[k] = p->pool[k - 1].h;
        p->mask_w[k] = p->pool[k - 1].w;
    }
    float* mem = nullptr;
    if (plan_alloc(p, &mem, 2 * (kPyramidPartials + 8 * kMaxRegions))) return 1;
    p->mask_stats = reinterpret_cast<double*>(mem);
    return 0;
}


// rho: the weights given, or 1 / R each
void deal_region_weights(st_plan* p, int regions, const float* given) {
    for (int r = 0; r < kMaxRegions; ++r) p->region_weight[r] = r >= regions ? 0.f : given ? given[r] : 1.f / (float)regions;
}

}  // namespace

int ensure_region_heads(st_plan* p, int regions, const int* style_ops, int n_style, const int* kinds) {
    if (regions <= 0) return 0;
    if (!p->region_amax) {
        float* mem = nullptr;
        if (plan_alloc(p, &mem, (size_t)(kMaxRegions - 1) * 16 * kAmaxWordUints)) return 1;
        p->region_amax = reinterpret_cast<unsigned int*>(mem);
    }
    if (!p->region_terms) {
        if (plan_alloc(p, &p->region_terms, (size_t)kMaxRegions * 16)) return 1;
        ST_HIP(hipMemset(p->region_terms, 0, (size_t)kMaxRegions * 16 * sizeof(float)));
    }
    for (int r = 1; r < regions; ++r)
        for (int j = 0; j < n_style; ++j) {
            const StyleHead& base = p->head[style_ops[j]];
            StyleHead& h = p->region_head[r - 1][style_ops[j]];
            h.n = base.n;
            h.npix = base.npix;
            h.npix_local = base.npix_local;
            if (ensure_style_alloc(p, h, kinds[j])) return 1;
        }
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
    for (int j = 0; j < p->n_style; ++j)
        ST_REQUIRE(!p->style_marg[j], "st_plan_set_style_mask: style layer %d is flagged marginal (st_plan_set_w2_marginal), which takes no "
                   "style mask: clear the flag first", j);
    for (int j = 0; j < p->n_style; ++j)
        ST_REQUIRE(!p->style_near[j], "st_plan_set_style_mask: style layer %d is flagged nearest (st_plan_set_style_nearest), which takes no "
                   "style mask: clear the flag first", j);
    for (int j = 0; j < p->n_style; ++j)
        ST_REQUIRE(!p->style_sliced[j], "st_plan_set_style_mask: style layer %d is flagged sliced (st_plan_set_style_sliced), which takes no "
                   "style mask: clear the flag first", j);
    ST_REQUIRE(!p->n_regions, "st_plan_set_style_mask: %d style regions are in force on this plan (st_plan_set_style_regions): "
               "clear them first", p->n_regions);
    constexpr size_t kPartials = kPyramidPartials;
    if (ensure_pyramid_scratch(p)) return 1;
    for (int k = 0; k < kMaskLevels; ++k)
        if (!p->mask_sqrt[k] && plan_alloc(p, &p->mask_sqrt[k], (size_t)p->mask_h[k] * p->mask_w[k])) return 1;
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

namespace {

// What both weight-map setters do: the first `levels` levels of `map`'s pyramid, stored as they are (level 0: a bit-exact
// copy), validated by the same pass - one read-back of the level sums, the range and the NaN count.  `who` names the setter.
int take_weight_map(st_plan* p, const float* map, float** level, int levels, const char* who, hipStream_t s) {
    if (ensure_pyramid_scratch(p)) return 1;
    for (int k = 0; k < levels; ++k)
        if (!level[k] && plan_alloc(p, &level[k], (size_t)p->mask_h[k] * p->mask_w[k])) return 1;
    double* results = p->mask_stats + kPyramidPartials;
    if (launch_mask_pyramid(map, p->mask_h, p->mask_w, level, p->mask_stats, results, s, /*store_root=*/false, levels)) return 1;
    double stats[8];
    ST_HIP(hipMemcpyAsync(stats, results, sizeof(stats), hipMemcpyDeviceToHost, s));
    ST_HIP(hipStreamSynchronize(s));
    ST_REQUIRE(stats[7] == 0.0, "%s: the map holds %.0f NaN value(s): a map's values lie in [0, 1]", who, stats[7]);
    ST_REQUIRE(stats[5] >= 0.0 && stats[6] <= 1.0, "%s: the map's values span [%g, %g]: a map's values lie in [0, 1]", who, stats[5],
               stats[6]);
    ST_REQUIRE(stats[0] > 0.0, "%s: the map is zero everywhere: the term would vanish (set its weight to 0 for that)", who);
    return 0;
}

}  // namespace

int st_plan_set_content_mask(st_plan* p, const float* mask, void* stream) {
    ST_REQUIRE(p, "st_plan_set_content_mask: null plan");
    ST_REQUIRE(!p->strip, "st_plan_set_content_mask: strip plans take no content map (the general closure serves it, on one device)");
    // no map is in force until it is accepted: the levels are overwritten whether or not it then is
    if (p->content_mask || mask) invalidate_graph(p);
    p->content_mask = false;
    if (!mask) return 0;
    if (take_weight_map(p, mask, p->content_map, kMaskLevels, "st_plan_set_content_mask", static_cast<hipStream_t>(stream))) return 1;
    p->content_mask = true;
    return 0;
}

int st_plan_content_mask(const st_plan* p, int level, const float** map, int* h, int* w) {
    ST_REQUIRE(p, "st_plan_content_mask: null plan");
    ST_REQUIRE(p->content_mask, "st_plan_content_mask: no content map is set on this plan (st_plan_set_content_mask)");
    ST_REQUIRE(level >= 0 && level < kMaskLevels, "st_plan_content_mask: level %d out of range (0 .. %d)", level, kMaskLevels - 1);
    if (map) *map = p->content_map[level];
    if (h) *h = p->mask_h[level];
    if (w) *w = p->mask_w[level];
    return 0;
}

int st_plan_set_tv_mask(st_plan* p, const float* mask, void* stream) {
    ST_REQUIRE(p, "st_plan_set_tv_mask: null plan");
    ST_REQUIRE(!p->strip, "st_plan_set_tv_mask: strip plans take no TV map (the general closure serves it, on one device)");
    if (p->tv_mask || mask) invalidate_graph(p);
    p->tv_mask = false;
    if (!mask) return 0;
    if (take_weight_map(p, mask, &p->tv_map, 1, "st_plan_set_tv_mask", static_cast<hipStream_t>(stream))) return 1;
    p->tv_mask = true;
    return 0;
}

int st_plan_tv_mask(const st_plan* p, const float** map, int* h, int* w) {
    ST_REQUIRE(p, "st_plan_tv_mask: null plan");
    ST_REQUIRE(p->tv_mask, "st_plan_tv_mask: no TV map is set on this plan (st_plan_set_tv_mask)");
    if (map) *map = p->tv_map;
    if (h) *h = p->H;
    if (w) *w = p->W;
    return 0;
}

int st_plan_set_style_regions(st_plan* p, int n_regions, const float* const* masks, void* stream) {
    ST_REQUIRE(p, "st_plan_set_style_regions: null plan");
    ST_REQUIRE(!p->strip, "st_plan_set_style_regions: strip plans take no style regions (a level's sum would span the ranks)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int j = 0; n_regions != 0 && j < p->n_style; ++j)
        ST_REQUIRE(!p->style_marg[j], "st_plan_set_style_regions: style layer %d is flagged marginal (st_plan_set_w2_marginal), which takes "
                   "no style regions: clear the flag first", j);
    for (int j = 0; n_regions != 0 && j < p->n_style; ++j)
        ST_REQUIRE(!p->style_near[j], "st_plan_set_style_regions: style layer %d is flagged nearest (st_plan_set_style_nearest), which takes "
                   "no style regions: clear the flag first", j);
    for (int j = 0; n_regions != 0 && j < p->n_style; ++j)
        ST_REQUIRE(!p->style_sliced[j], "st_plan_set_style_regions: style layer %d is flagged sliced (st_plan_set_style_sliced), which takes "
                   "no style regions: clear the flag first", j);
    // no regions are in force until every one of them is accepted
    p->n_regions = 0;
    invalidate_graph(p);
    if (n_regions == 0) return 0;
    ST_REQUIRE(n_regions >= 1 && n_regions <= kMaxRegions, "st_plan_set_style_regions: %d regions: a plan takes 1 to %d", n_regions,
               kMaxRegions);
    ST_REQUIRE(masks, "st_plan_set_style_regions: null list of masks");
    for (int r = 0; r < n_regions; ++r) ST_REQUIRE(masks[r], "st_plan_set_style_regions: the mask of region %d is null", r);
    ST_REQUIRE(!p->style_mask, "st_plan_set_style_regions: a style mask is in force on this plan (st_plan_set_style_mask): clear it first");
    if (ensure_pyramid_scratch(p)) return 1;
    for (int r = 0; r < n_regions; ++r)
        for (int k = 0; k < kMaskLevels; ++k)
            if (!p->region_sqrt[r][k] && plan_alloc(p, &p->region_sqrt[r][k], (size_t)p->mask_h[k] * p->mask_w[k])) return 1;
    int alloc_kinds[16];
    for (int j = 0; j < 16; ++j) alloc_kinds[j] = j < p->n_style ? alloc_kind_of(p, j) : 0;
    if (ensure_region_heads(p, n_regions, p->style_op, p->n_style, alloc_kinds)) return 1;
    assign_head_bounds(p);
    // one pyramid call per region (the partials are reused in stream order), 8 results each, ONE read-back
    double* results = p->mask_stats + kPyramidPartials;
    for (int r = 0; r < n_regions; ++r)
        if (launch_mask_pyramid(masks[r], p->mask_h, p->mask_w, p->region_sqrt[r], p->mask_stats, results + 8 * r, s)) return 1;
    double stats[8 * kMaxRegions];
    ST_HIP(hipMemcpyAsync(stats, results, (size_t)8 * n_regions * sizeof(double), hipMemcpyDeviceToHost, s));
    ST_HIP(hipStreamSynchronize(s));
    for (int r = 0; r < n_regions; ++r) {
        const double* st = stats + 8 * r;
        ST_REQUIRE(st[7] == 0.0, "st_plan_set_style_regions: the mask of region %d holds %.0f NaN value(s): a mask's values lie in [0, 1]",
                   r, st[7]);
        ST_REQUIRE(st[5] >= 0.0 && st[6] <= 1.0,
                   "st_plan_set_style_regions: the values of region %d's mask span [%g, %g]: a mask's values lie in [0, 1]", r, st[5], st[6]);
        for (int k = 0; k < kMaskLevels; ++k) {
            ST_REQUIRE(st[k] > 0.0,
                       "st_plan_set_style_regions: region %d's mask, level %d (%d x %d, behind %d poolings) sums to 0: the style layers "
                       "at that level would have no pixel to take the region's statistics from", r, k, p->mask_h[k], p->mask_w[k], k);
            p->region_sum[r][k] = st[k];
        }
    }
    deal_region_weights(p, n_regions, nullptr);
    p->n_regions = n_regions;
    return 0;
}

int st_plan_style_region(const st_plan* p, int region, int level, const float** sqrt_mask, int* h, int* w, double* sum) {
    ST_REQUIRE(p, "st_plan_style_region: null plan");
    ST_REQUIRE(p->n_regions > 0, "st_plan_style_region: no style regions are set on this plan (st_plan_set_style_regions)");
    ST_REQUIRE(region >= 0 && region < p->n_regions, "st_plan_style_region: region %d out of range (%d regions)", region, p->n_regions);
    ST_REQUIRE(level >= 0 && level < kMaskLevels, "st_plan_style_region: level %d out of range (0 .. %d)", level, kMaskLevels - 1);
    if (sqrt_mask) *sqrt_mask = p->region_sqrt[region][level];
    if (h) *h = p->mask_h[level];
    if (w) *w = p->mask_w[level];
    if (sum) *sum = p->region_sum[region][level];
    return 0;
}

int st_plan_set_region_weights(st_plan* p, const float* weights) {
    ST_REQUIRE(p, "st_plan_set_region_weights: null plan");
    ST_REQUIRE(p->n_regions > 0, "st_plan_set_region_weights: no style regions are set on this plan (st_plan_set_style_regions)");
    for (int r = 0; weights && r < p->n_regions; ++r)
        ST_REQUIRE(std::isfinite(weights[r]), "st_plan_set_region_weights: the weight of region %d is not finite", r);
    deal_region_weights(p, p->n_regions, weights);
    invalidate_graph(p);       // the weights are baked into kernel arguments
    return 0;
}

int st_plan_region_terms(st_plan* p, float** terms, int* regions, int* styles) {
    ST_REQUIRE(p && terms, "st_plan_region_terms: null argument");
    ST_REQUIRE(p->n_regions > 0, "st_plan_region_terms: no style regions are set on this plan (st_plan_set_style_regions)");
    *terms = p->region_terms;
    if (regions) *regions = p->n_regions;
    if (styles) *styles = p->n_style;
    return 0;
}

}  // extern "C"
