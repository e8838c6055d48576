// The reference's loss modules outside a plan (include/st_amd.h "NATIVE LOSS MODULES"): a standalone style head that is not
// welded to an st_plan, and the pointwise terms - MSE, scaled MSE, TV - as value / gradient pairs whose upstream gradient is a
// DEVICE scalar (autograd's grad_output, the product of Scale / SumLoss: never read on the host).
//
// A head runs st_head_core.h's sequence - a plan's heads' own, launch for launch - on its own StyleHead with weight 1 and no mask;
// its backward is (u Ssym, u b) and the bound of u Ssym by head_scale_kernel, the one head kernel of this file, then head_step.
// What a plan knows and a head must find out: the operand bound of the fp16x3 kernels.  A trunk kernel leaves max |y| of the
// tap it writes; here the tensor is whatever autograd hands over - signed, possibly all zeros (bound 0: scale_exp gives 2^0,
// the planes are exact zeros and the bias term alone makes the result) - so head_moments measures it, once per forward, into
// the per-call state that the backward reads.  eps is the module's, where the plan passes its entry's (kCovEps / kScaledMseEps by default).
#include <cstdint>
#include <vector>

#include "../../include/st_amd.h"
#include "st_head_core.h"

struct st_head {
    int kind = 0, height = 0, width = 0, precision = 0;
    long long bytes = 0;
    std::vector<void*> allocations;
    st::StyleHead w;                 // this forward's moments and W2 matrices; (ssym, bvec, s_amax): the backward's (u Ssym, u b), max |u Ssym|
    unsigned int* feat_bound = nullptr;                    // fp16x3: max |F| of a forward without state
    // Gram only
    float *kind_partials = nullptr, *totals = nullptr;
    unsigned int* ticket = nullptr;
};

namespace st {
namespace {

constexpr long long kReduceScratchFloats = 4 * kStreamBlocks;

int head_alloc(st_head* h, float** out, size_t floats) {
    void* p = nullptr;
    ST_HIP(hipMalloc(&p, floats * sizeof(float)));
    h->allocations.push_back(p);
    h->bytes += (long long)(floats * sizeof(float));
    *out = static_cast<float*>(p);
    return 0;
}

size_t state_floats(const st_head* h) { return (size_t)h->w.n * h->w.n + h->w.n + kAmaxWordUints; }

// (u Ssym, u b) and the bound on max |u Ssym| for the fp16x3 1x1 step; one workgroup per row.  u Ssym stays exactly symmetric.
__global__ __launch_bounds__(256) void head_scale_kernel(const float* __restrict__ ssym, const float* __restrict__ bvec,
                                                         const float* __restrict__ upstream, int n, float* __restrict__ ssym_u,
                                                         float* __restrict__ b_u, unsigned int* __restrict__ bound) {
    const float u = upstream[0];
    const int c = blockIdx.x;
    unsigned int amax = 0;
    for (int d = threadIdx.x; d < n; d += 256) {
        const float v = u * ssym[(size_t)c * n + d];
        ssym_u[(size_t)c * n + d] = v;
        const unsigned int bits = abs_bits(v);
        amax = bits > amax ? bits : amax;
    }
    if (bound) amax_commit(amax, bound);          // (every lane arrives: no early return above)
    if (threadIdx.x == 0) b_u[c] = u * bvec[c];
}

// ---- pointwise terms ---------------------------------------------------------------------------------------------------
// per-workgroup (sum d^2, sum |d|), d = x - t; VEC: 16-byte accesses (count % 4 == 0, aligned pointers)
template <bool VEC>
__global__ __launch_bounds__(256) void diff_sums_kernel(const float* __restrict__ x, const float* __restrict__ target,
                                                        long long count, float* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ float scratch[4];
    float s2 = 0.f, s1 = 0.f;
    if (VEC) {
        const long long n4 = count >> 2;
        const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
        const f32x4* t4 = reinterpret_cast<const f32x4*>(target);
        for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
            const f32x4 f = x4[i], t = t4[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d = f[k] - t[k];
                s2 += d * d;
                s1 += fabsf(d);
            }
        }
    } else {
        for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
            const float d = x[i] - target[i];
            s2 += d * d;
            s1 += fabsf(d);
        }
    }
    s2 = block_sum_256(s2, scratch);
    s1 = block_sum_256(s1, scratch);
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = s2;
        partials[2 * blockIdx.x + 1] = s1;
    }
}
// one workgroup, partials added in index order.  scaled == 0: loss = S2 / count (nn.MSELoss); else totals = (S2, S1 + eps) and
// loss = S2 / (S1 + eps) (ScaledMSELoss)
__global__ __launch_bounds__(256) void diff_sums_final_kernel(const float* __restrict__ partials, int nparts, int scaled,
                                                              float count, float eps, float* __restrict__ totals,
                                                              float* __restrict__ loss_out) {
#pragma clang fp contract(off)
    __shared__ float scratch[4];
    float t2 = 0.f, t1 = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) {
        t2 += partials[2 * i];
        t1 += partials[2 * i + 1];
    }
    t2 = block_sum_256(t2, scratch);
    t1 = block_sum_256(t1, scratch);
    if (threadIdx.x != 0) return;
    if (!scaled) {
        loss_out[0] = t2 / count;
        return;
    }
    const float sum_abs = t1 + eps;
    totals[0] = t2;
    totals[1] = sum_abs;
    loss_out[0] = t2 / sum_abs;
}
// mse_loss_backward / the scaled-MSE slope (st_pointwise.hip) times the device scalar.  SCALED: totals = (S2, S1 + eps).
template <bool SCALED, bool VEC>
__global__ __launch_bounds__(256) void diff_grad_kernel(const float* __restrict__ x, const float* __restrict__ target,
                                                        long long count, float norm, const float* __restrict__ totals,
                                                        const float* __restrict__ upstream, float* __restrict__ grad) {
#pragma clang fp contract(off)
    const float u = upstream[0];
    float s1 = 1.f, level = 0.f;
    if (SCALED) {
        s1 = totals[1];
        level = totals[0] / s1;
    }
    auto slope = [&](float d) __attribute__((always_inline)) {
        if (!SCALED) return (norm * d) * u;
        const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        return ((2.f * d - level * sg) / s1) * u;
    };
    if (VEC) {
        const long long n4 = count >> 2;
        const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
        const f32x4* t4 = reinterpret_cast<const f32x4*>(target);
        f32x4* g4 = reinterpret_cast<f32x4*>(grad);
        for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
            const f32x4 f = x4[i], t = t4[i];
            f32x4 g;
#pragma unroll
            for (int k = 0; k < 4; ++k) g[k] = slope(f[k] - t[k]);
            g4[i] = g;
        }
    } else {
        for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += (long long)gridDim.x * 256)
            grad[i] = slope(x[i] - target[i]);
    }
}

// ---- TVLoss (st_pointwise.hip has the formulas: D1 .. D4 on the replicate-padded image) ----------------------------------
// One pixel per thread, any position, no strips: the value's four sums of squares and, separately, the gradient.  The plan's
// streaming pair (tv_interior_kernel / tv_border_kernel) writes both at once with a host weight; autograd wants the value
// in forward() and the gradient - times a device scalar - in backward().
struct TvPlane {
    const float* p;        // one channel [H][W]
    int H, W;
    __device__ __forceinline__ float at(int a, int b) const {      // padded coordinates a in [-1, H], b in [-1, W]
        a = min(max(a, 0), H - 1);
        b = min(max(b, 0), W - 1);
        return p[(size_t)a * W + b];
    }
};
// gradient w.r.t. the PADDED image at (a, b) (tv_dP of st_pointwise.hip on a whole image)
__device__ __forceinline__ float tv_padded_grad(const TvPlane& im, int a, int b, float k1, float k3) {
#pragma clang fp contract(off)
    const int H = im.H, W = im.W;
    const float c = im.at(a, b);
    float g = 0.f;
    const bool row_in = (a >= 0 && a < H), col_in = (b >= 0 && b < W);
    if (row_in) {
        if (b >= 1 && b <= W) g += k1 * (c - im.at(a, b - 1));
        if (col_in) g -= k1 * (im.at(a, b + 1) - c);
    }
    if (col_in) {
        if (a >= 1 && a <= H) g += k1 * (c - im.at(a - 1, b));
        if (row_in) g -= k1 * (im.at(a + 1, b) - c);
    }
    if (a >= 0 && b >= 0) g += k3 * (c - im.at(a - 1, b - 1));            // D3(a, b)
    if (a <= H - 1 && b <= W - 1) g -= k3 * (im.at(a + 1, b + 1) - c);    // D3(a+1, b+1)
    if (a >= 0 && b <= W - 1) g += k3 * (c - im.at(a - 1, b + 1));        // D4(a, b+1)
    if (a <= H - 1 && b >= 0) g -= k3 * (im.at(a + 1, b - 1) - c);        // D4(a+1, b)
    return g;
}
__global__ __launch_bounds__(256) void tv_value_kernel(const float* __restrict__ image, int H, int W,
                                                       float* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ float scratch[4];
    float s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
    const long long total = 3ll * H * W;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int x = (int)(i % W);
        const long long r = i / W;
        const int y = (int)(r % H);
        const TvPlane im{image + (size_t)(r / H) * H * W, H, W};
        // every difference is owned by exactly one pixel (the last row / column own the padding ring's)
        const float c = im.at(y, x);
        const float d1 = im.at(y, x + 1) - c, d2 = im.at(y + 1, x) - c;
        s1 += d1 * d1;
        s2 += d2 * d2;
        for (int iy = y; iy <= ((y == H - 1) ? y + 1 : y); ++iy)
            for (int jx = x; jx <= ((x == W - 1) ? W : x); ++jx) {
                const float d3 = im.at(iy, jx) - im.at(iy - 1, jx - 1);
                const float d4 = im.at(iy, jx - 1) - im.at(iy - 1, jx);
                s3 += d3 * d3;
                s4 += d4 * d4;
            }
    }
    s1 = block_sum_256(s1, scratch);
    s2 = block_sum_256(s2, scratch);
    s3 = block_sum_256(s3, scratch);
    s4 = block_sum_256(s4, scratch);
    if (threadIdx.x == 0) {
        float* mine = partials + (size_t)blockIdx.x * 4;
        mine[0] = s1; mine[1] = s2; mine[2] = s3; mine[3] = s4;
    }
}
__global__ __launch_bounds__(256) void tv_value_final_kernel(const float* __restrict__ partials, int nparts, float n, float n2,
                                                             float* __restrict__ loss_out) {
#pragma clang fp contract(off)
    __shared__ float scratch[4];
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < nparts; i += 256)
        for (int k = 0; k < 4; ++k) t[k] += partials[i * 4 + k];
    for (int k = 0; k < 4; ++k) t[k] = block_sum_256(t[k], scratch);
    if (threadIdx.x == 0) {
        const float d1 = (t[0] / n) / 3.f, d2 = (t[1] / n) / 3.f;
        const float d3 = (t[2] / n2) / 12.f, d4 = (t[3] / n2) / 12.f;
        loss_out[0] = 2.f * (((d1 + d2) + d3) + d4);
    }
}
// c1, c3: d loss / d D of the unweighted loss over D (launch_tv's k1, k3 at weight 1); the device scalar scales both
__global__ __launch_bounds__(256) void tv_grad_kernel(const float* __restrict__ image, int H, int W, float c1, float c3,
                                                      const float* __restrict__ upstream, float* __restrict__ grad) {
#pragma clang fp contract(off)
    const float u = upstream[0];
    const float k1 = u * c1, k3 = u * c3;
    const long long total = 3ll * H * W;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int x = (int)(i % W);
        const long long r = i / W;
        const int y = (int)(r % H);
        const TvPlane im{image + (size_t)(r / H) * H * W, H, W};
        // this pixel plus the padding-ring positions that replicate it
        float g = 0.f;
        for (int ry = -1; ry <= 1; ++ry) {
            if (ry != 0 && !((ry < 0 && y == 0) || (ry > 0 && y == H - 1))) continue;
            for (int rx = -1; rx <= 1; ++rx) {
                if (rx != 0 && !((rx < 0 && x == 0) || (rx > 0 && x == W - 1))) continue;
                g += tv_padded_grad(im, y + ry, x + rx, k1, k3);
            }
        }
        grad[i] = g;
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
int stream_grid(long long items) {
    const long long want = (items + 255) / 256;
    return (int)(want < 1 ? 1 : (want > kStreamBlocks ? kStreamBlocks : want));
}
bool vec4(long long count, const void* a, const void* b, const void* c) {
    return (count & 3) == 0 &&
           ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}

int diff_sums(const float* x, const float* target, long long count, int scaled, float eps, float* scratch, float* totals,
              float* loss_out, hipStream_t s) {
    const bool vec = vec4(count, x, target, nullptr);
    const int blocks = stream_grid(vec ? count / 4 : count);
    if (vec) hipLaunchKernelGGL(diff_sums_kernel<true>, dim3(blocks), dim3(256), 0, s, x, target, count, scratch);
    else hipLaunchKernelGGL(diff_sums_kernel<false>, dim3(blocks), dim3(256), 0, s, x, target, count, scratch);
    ST_LAUNCH_CHECK();
    hipLaunchKernelGGL(diff_sums_final_kernel, dim3(1), dim3(256), 0, s, scratch, blocks, scaled, (float)count, eps, totals, loss_out);
    ST_LAUNCH_CHECK();
    return 0;
}

template <bool SCALED>
int diff_grad(const float* x, const float* target, long long count, const float* totals, const float* upstream, float* grad,
              hipStream_t s) {
    const bool vec = vec4(count, x, target, grad);
    const int blocks = stream_grid(vec ? count / 4 : count);
    const float norm = (float)(2.0 / (double)count);
    if (vec) hipLaunchKernelGGL((diff_grad_kernel<SCALED, true>), dim3(blocks), dim3(256), 0, s, x, target, count, norm, totals, upstream, grad);
    else hipLaunchKernelGGL((diff_grad_kernel<SCALED, false>), dim3(blocks), dim3(256), 0, s, x, target, count, norm, totals, upstream, grad);
    ST_LAUNCH_CHECK();
    return 0;
}

// this forward's moments, with max |F| measured into `bound` first (fp16x3); cov != nullptr: the covariance too
int moments_of(st_head* h, const float* feat, unsigned int* bound, float* mean, float* srm, float* cov, float eps, hipStream_t s) {
    HeadMoments m;
    m.feat = feat; m.mean = mean; m.srm = srm; m.cov = cov; m.eps = eps;
    if (h->precision == 4) { m.bound = bound; m.measure_bound = true; }
    return head_moments(h->w, m, s);
}

}  // namespace
}  // namespace st

using namespace st;

extern "C" {

int st_head_create(st_head** out, int kind, int channels, int height, int width, int precision) {
    ST_REQUIRE(out, "st_head_create: null argument");
    *out = nullptr;
    ST_REQUIRE(kind >= 0 && kind <= 2, "st_head_create: unknown kind %d (0: w2 - StyleLossW2, 1: gram - StyleLoss, 2: moments only)", kind);
    ST_REQUIRE(channels == 64 || channels == 128 || channels == 256 || channels == 512,
               "st_head_create: %d channels: must be 64, 128, 256 or 512", channels);
    ST_REQUIRE(height >= 1 && width >= 1, "st_head_create: a %d x %d tap: height and width >= 1", height, width);
    ST_REQUIRE_PIXELS("st_head_create", (long long)height * width);
    ST_REQUIRE(precision == 0 || precision == 4, "st_head_create: precision must be 0 (fp32) or 4 (fp16x3)");
    st_head* h = new st_head;
    h->kind = kind; h->height = height; h->width = width; h->precision = precision;
    StyleHead& w = h->w;
    w.n = channels;
    w.npix = w.npix_local = (long long)height * width;
    auto fail = [&] { st_head_destroy(h); return 1; };
    auto alloc = [h](float** out, size_t floats) { return head_alloc(h, out, floats); };
    // sized by the routines that size a plan's heads - except that of the split cap this one shape ever uses gram_choose_splits'
    // pick (a plan's head may be handed fewer local pixels later).  A moments-only head: the Gram workspace, a mean, the bound words.
    if (alloc_head_moments(w, gram_choose_splits(w.n, w.npix, head_gram_split_cap(w.n)), /*with_step=*/kind != 2, alloc)) return fail();
    float* words = nullptr;
    if (head_alloc(h, &words, 2 * kAmaxWordUints)) return fail();
    h->feat_bound = reinterpret_cast<unsigned int*>(words);
    w.s_amax = h->feat_bound + kAmaxWordUints;
    if (hipMemset(words, 0, 2 * kAmaxWordUints * sizeof(float)) != hipSuccess) { set_error("st_head_create: hipMemset failed"); return fail(); }
    if (kind == 1) {
        float* tick = nullptr;
        if (head_alloc(h, &h->kind_partials, 2 * kStreamBlocks) || head_alloc(h, &h->totals, 64) || head_alloc(h, &tick, 64)) return fail();
        h->ticket = reinterpret_cast<unsigned int*>(tick);
        if (hipMemset(tick, 0, 64 * sizeof(float)) != hipSuccess) { set_error("st_head_create: hipMemset failed"); return fail(); }
    } else if (kind == 0 && alloc_head_w2(w, alloc)) {
        return fail();
    }
    if (hipStreamSynchronize(nullptr) != hipSuccess) { set_error("st_head_create: synchronise failed"); return fail(); }
    *out = h;
    return 0;
}

int st_op_gram_split_plan(int channels, long long npix, int precision, int* splits, long long* per_split, int* wide) {
    ST_REQUIRE(channels == 64 || channels == 128 || channels == 256 || channels == 512,
               "st_op_gram_split_plan: %d channels: must be 64, 128, 256 or 512", channels);
    ST_REQUIRE_PIXELS("st_op_gram_split_plan", npix);
    ST_REQUIRE(precision == 0 || precision == 4, "st_op_gram_split_plan: precision must be 0 (fp32) or 4 (fp16x3)");
    // st_head_create sizes the workspace by this pick, and head_moments picks again under that size: the same number
    const int n = gram_choose_splits(channels, npix, head_gram_split_cap(channels));
    if (splits) *splits = n;
    if (per_split) *per_split = gram_per_split(npix, n);
    if (wide) *wide = (precision == 4 && gram_wide_tiles(channels, npix)) ? 1 : 0;
    return 0;
}

int st_head_destroy(st_head* h) {
    if (!h) return 0;
    for (void* p : h->allocations) hipFree(p);
    delete h;
    return 0;
}

long long st_head_device_bytes(const st_head* h) { return h ? h->bytes : 0; }

long long st_head_state_floats(const st_head* h) { return h ? (long long)state_floats(h) : 0; }

int st_head_moments(st_head* h, const float* feat, float* mean_out, float* srm_out, void* stream) {
    ST_REQUIRE(h && feat && srm_out, "st_head_moments: null argument");
    ST_REQUIRE(aligned16(feat), "st_head_moments: feat must be 16-byte aligned");
    return moments_of(h, feat, h->feat_bound, mean_out ? mean_out : h->w.mean, srm_out, nullptr, 0.f, static_cast<hipStream_t>(stream));
}

int st_head_forward(st_head* h, const float* feat, const float* mean_t, const float* cov_t, const float* root_t,
                    const float* gram_t, float eps, float* loss_out, float* state, void* stream) {
    ST_REQUIRE(h && feat && loss_out, "st_head_forward: null argument");
    ST_REQUIRE(h->kind != 2, "st_head_forward: a moments-only head");
    ST_REQUIRE(aligned16(feat), "st_head_forward: feat must be 16-byte aligned");
    ST_REQUIRE(aligned16(state), "st_head_forward: state must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    StyleHead& w = h->w;
    const int n = w.n;
    const size_t nn = (size_t)n * n;
    float* ssym = state;
    float* bvec = state ? state + nn : nullptr;
    unsigned int* bound = state ? reinterpret_cast<unsigned int*>(state + nn + n) : h->feat_bound;
    if (h->kind == 1) {
        // StyleLoss.forward (style_transfer.py:141-142): ScaledMSELoss of the Gram matrix against its target
        ST_REQUIRE(gram_t, "st_head_forward: a Gram head needs gram_t");
        if (moments_of(h, feat, bound, w.mean, w.srm, nullptr, 0.f, s)) return 1;
        return gram_body(w, gram_t, 1.f, eps, h->kind_partials, h->totals, h->ticket, loss_out, ssym, bvec, nullptr, 0.f, s);
    }
    // StyleLossW2.forward (style_transfer.py:174-181)
    ST_REQUIRE(mean_t && cov_t && root_t, "st_head_forward: a W2 head needs mean_t, cov_t and root_t");
    if (moments_of(h, feat, bound, w.mean, w.srm, w.cov, eps, s)) return 1;
    int m_partials = 0, root_partials = 0;
    if (w2_open(w, root_t, s, &m_partials)) return 1;
    if (ns_sqrt_forward(w.mmat, w.root, n, w.ns, s, m_partials, &root_partials)) return 1;
    if (!state)       // the value alone: no Lyapunov chain to ride in
        return launch_style_loss_value(w.mean, mean_t, w.cov, cov_t, w.root, n, 1.f, loss_out, w.gdiag, s);
    // the loss term and the seed dL/d root = gdiag I in the backward chain's opening kernel, then dL/dM
    const W2LossJob job = w2_loss_job(w, mean_t, cov_t, 1.f, loss_out);
    if (ns_sqrt_backward(w.root, nullptr, w.gdiag, w.gm, n, w.ns, s, &job, root_partials)) return 1;
    return w2_close(w, mean_t, root_t, 1.f, ssym, bvec, nullptr, 0.f, s);
}

int st_head_backward(st_head* h, const float* feat, const float* state, const float* upstream, float* grad_feat, void* stream) {
    ST_REQUIRE(h && feat && state && upstream && grad_feat, "st_head_backward: null argument");
    ST_REQUIRE(h->kind != 2, "st_head_backward: a moments-only head");
    ST_REQUIRE(aligned16(feat), "st_head_backward: feat must be 16-byte aligned");
    ST_REQUIRE(aligned16(state), "st_head_backward: state must be 16-byte aligned");
    ST_REQUIRE(aligned16(grad_feat), "st_head_backward: grad_feat must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const StyleHead& w = h->w;
    const int n = w.n;
    const size_t nn = (size_t)n * n;
    const bool f16 = h->precision == 4;
    if (f16) ST_HIP(hipMemsetAsync(w.s_amax, 0, kAmaxWordUints * sizeof(unsigned int), s));
    hipLaunchKernelGGL(head_scale_kernel, dim3(n), dim3(256), 0, s, state, state + nn, upstream, n, w.ssym, w.bvec, f16 ? w.s_amax : nullptr);
    ST_LAUNCH_CHECK();
    // dF = (u Ssym) F + (u b) 1^T: the plan's 1x1 step without a mask or a consumer's bound, on the bound the forward left in the state
    return head_step(w, feat, h->height, h->width, grad_feat, s, f16, const_cast<unsigned int*>(reinterpret_cast<const unsigned int*>(state + nn + n)));
}

long long st_op_reduce_scratch_floats(void) { return kReduceScratchFloats; }

int st_op_mse_loss(const float* x, const float* target, long long count, float* scratch, float* loss_out, void* stream) {
    ST_REQUIRE(x && target && scratch && loss_out && count > 0, "st_op_mse_loss: null argument or empty tensor");
    return diff_sums(x, target, count, 0, 0.f, scratch, nullptr, loss_out, static_cast<hipStream_t>(stream));
}

int st_op_mse_loss_backward(const float* x, const float* target, long long count, const float* upstream, float* grad,
                            void* stream) {
    ST_REQUIRE(x && target && upstream && grad && count > 0, "st_op_mse_loss_backward: null argument or empty tensor");
    return diff_grad<false>(x, target, count, nullptr, upstream, grad, static_cast<hipStream_t>(stream));
}

int st_op_scaled_mse_loss(const float* x, const float* target, long long count, float eps, float* scratch, float* totals,
                          float* loss_out, void* stream) {
    ST_REQUIRE(x && target && scratch && totals && loss_out && count > 0, "st_op_scaled_mse_loss: null argument or empty tensor");
    return diff_sums(x, target, count, 1, eps, scratch, totals, loss_out, static_cast<hipStream_t>(stream));
}

int st_op_scaled_mse_loss_backward(const float* x, const float* target, long long count, const float* totals,
                                   const float* upstream, float* grad, void* stream) {
    ST_REQUIRE(x && target && totals && upstream && grad && count > 0, "st_op_scaled_mse_loss_backward: null argument or empty tensor");
    return diff_grad<true>(x, target, count, totals, upstream, grad, static_cast<hipStream_t>(stream));
}

int st_op_tv_value(const float* image, int height, int width, float* scratch, float* loss_out, void* stream) {
    ST_REQUIRE(image && scratch && loss_out, "st_op_tv_value: null argument");
    ST_REQUIRE(height >= 1 && width >= 1, "st_op_tv_value: bad shape %d x %d", height, width);
    ST_REQUIRE_PIXELS("st_op_tv_value", (long long)height * width);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int blocks = stream_grid(3ll * height * width);
    hipLaunchKernelGGL(tv_value_kernel, dim3(blocks), dim3(256), 0, s, image, height, width, scratch);
    ST_LAUNCH_CHECK();
    const double n = 3.0 * height * width, n2 = 3.0 * (height + 1) * (width + 1);
    hipLaunchKernelGGL(tv_value_final_kernel, dim3(1), dim3(256), 0, s, scratch, blocks, (float)n, (float)n2, loss_out);
    ST_LAUNCH_CHECK();
    return 0;
}

int st_op_tv_loss_backward(const float* image, int height, int width, const float* upstream, float* grad, void* stream) {
    ST_REQUIRE(image && upstream && grad, "st_op_tv_loss_backward: null argument");
    ST_REQUIRE(height >= 1 && width >= 1, "st_op_tv_loss_backward: bad shape %d x %d", height, width);
    ST_REQUIRE_PIXELS("st_op_tv_loss_backward", (long long)height * width);
    const double n = 3.0 * height * width, n2 = 3.0 * (height + 1) * (width + 1);
    // d loss / d D = 2 * (1/3 or 1/12) * (1/n) * 2 D
    const float c1 = (float)(4.0 / (3.0 * n)), c3 = (float)(4.0 / (12.0 * n2));
    hipLaunchKernelGGL(tv_grad_kernel, dim3(stream_grid(3ll * height * width)), dim3(256), 0, static_cast<hipStream_t>(stream), image,
                       height, width, c1, c3, upstream, grad);
    ST_LAUNCH_CHECK();
    return 0;
}

// the closure's one-launch forms (launch_content_mse / launch_tv with a ticket) on the caller's scratch and ticket word
int st_op_mse_term(const float* x, const float* target, long long count, float weight, float* scratch, unsigned int* ticket,
                   float* loss_out, float* grad_out, void* stream) {
    ST_REQUIRE(x && target && scratch && ticket && loss_out && grad_out && count > 0, "st_op_mse_term: null argument or empty tensor");
    ST_REQUIRE(aligned16(x) && aligned16(target) && aligned16(grad_out), "st_op_mse_term: x, target and grad_out must be 16-byte aligned");
    return launch_content_mse(x, target, count, weight, grad_out, scratch, loss_out, static_cast<hipStream_t>(stream), ticket);
}

int st_op_tv_term(const float* image, int height, int width, float weight, float* scratch, unsigned int* ticket, float* loss_out,
                  float* grad_out, void* stream) {
    ST_REQUIRE(image && scratch && ticket && loss_out && grad_out, "st_op_tv_term: null argument");
    ST_REQUIRE(height >= 1 && width >= 1, "st_op_tv_term: bad shape %d x %d", height, width);
    ST_REQUIRE_PIXELS("st_op_tv_term", (long long)height * width);
    return launch_tv(image, height, width, weight, grad_out, scratch, loss_out, static_cast<hipStream_t>(stream), ticket);
}

}  // extern "C"
