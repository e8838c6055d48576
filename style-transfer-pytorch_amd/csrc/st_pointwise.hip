// HBM-bound pointwise kernels and small reductions of the hot loop.  All arithmetic here follows
// the reference's operation order with FP contraction disabled, so the only rounding differences
// against the CPU path are in reduction order.
#include "st_common.h"

namespace st {
namespace {

// ------------------------------------------------------------------------------------------------
__global__ void fill_kernel(float* p, long long n, float v) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) p[i] = v;
}
__global__ void identity_kernel(float* p, int n) {
    const long long nn = (long long)n * n;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < nn; i += (long long)gridDim.x * 256)
        p[i] = ((int)(i / n) == (int)(i % n)) ? 1.f : 0.f;
}

// cov = srm - mean mean^T + eps * I      (StyleLossW2.srm_to_cov + eye_like * eps, style_transfer.py:156,170-177)
__global__ void cov_kernel(const float* __restrict__ mean, const float* __restrict__ srm,
                           float* __restrict__ cov, int n, float eps) {
#pragma clang fp contract(off)
    const long long nn = (long long)n * n;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < nn; i += (long long)gridDim.x * 256) {
        const int r = (int)(i / n), c = (int)(i % n);
        const float outer = mean[r] * mean[c];
        const float d = srm[i] - outer;
        cov[i] = d + ((r == c) ? eps : 0.f);
    }
}

// two-pass Frobenius norm: partial sums of squares, then fixed-order combine + sqrt
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ a, long long count,
                                                            float* __restrict__ partials) {
    __shared__ float scratch[4];
    float s = 0.f;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
        const float v = a[i];
        s = fmaf(v, v, s);
    }
    s = block_sum_256(s, scratch);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}
__global__ __launch_bounds__(64) void sqrt_of_sum_kernel(const float* __restrict__ partials, int nparts,
                                                         float* __restrict__ out) {
    float s = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 64) s += partials[i];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[0] = sqrtf(s);
}

__global__ void div_by_dev_scalar_kernel(const float* __restrict__ a, const float* __restrict__ scalar,
                                         float* __restrict__ y, long long count) {
    const float d = scalar[0];
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += (long long)gridDim.x * 256)
        y[i] = a[i] / d;
}
__global__ void scaled_identity_div_kernel(const float* __restrict__ diag_value,
                                           const float* __restrict__ scalar, float* __restrict__ q, int n) {
    const float v = diag_value[0] / scalar[0];
    const long long nn = (long long)n * n;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < nn; i += (long long)gridDim.x * 256)
        q[i] = ((int)(i / n) == (int)(i % n)) ? v : 0.f;
}

// The two recurrences' prologues in two launches instead of four (they sit on the critical path of the whole
// iteration: the backward pass waits for relu5_1's chain): sums of squares in <= 256 partials (16-byte loads),
// then every workgroup re-combines the partials in the same fixed order, divides its share of `a` by the norm
// and fills the companion matrix.
__global__ __launch_bounds__(256) void sumsq_partial4_kernel(const float* __restrict__ a, long long count,
                                                             float* __restrict__ partials) {
    __shared__ float scratch[4];
    float s = 0.f;
    const long long n4 = count / 4;          // count = n * n with n % 64 == 0
    const f32x4* a4 = reinterpret_cast<const f32x4*>(a);
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const f32x4 v = a4[i];
        s = fmaf(v[0], v[0], s); s = fmaf(v[1], v[1], s); s = fmaf(v[2], v[2], s); s = fmaf(v[3], v[3], s);
    }
    s = block_sum_256(s, scratch);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}
// mode 0: second = I (sqrtm.py:16-20);  1: second = g / norm;  2: second = (gdiag / norm) I (sqrtm.py:38-41);
// 3: second = (3I - a / norm) / 2, the first step's t of sqrtm.py:22 for z = I (see ns_sqrt_forward)
__global__ __launch_bounds__(256) void ns_prepare_kernel(const float* __restrict__ a,
                                                         const float* __restrict__ partials, int nparts,
                                                         float* __restrict__ norm_out, float* __restrict__ a_scaled,
                                                         const float* __restrict__ g, const float* __restrict__ gdiag,
                                                         float* __restrict__ second, int n, int mode, W2LossJob loss) {
    __shared__ float scratch[4];
    __shared__ float norm_sh;
    float s = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) s += partials[i];
    s = block_sum_256(s, scratch);
    if (threadIdx.x == 0) {
        norm_sh = sqrtf(s);
        if (blockIdx.x == 0) norm_out[0] = norm_sh;
    }
    __syncthreads();
    const float d = norm_sh;
    // (a W2 job rides along: the seed gdiag is its own, written by w2_loss_block below for the chain's later launches)
    const float dv = (mode == 2) ? (loss.loss_out ? w2_gdiag(loss) : gdiag[0]) / d : 1.f;
    const long long nn = (long long)n * n;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < nn; i += (long long)gridDim.x * 256) {
        const float y = a[i] / d;
        a_scaled[i] = y;
        const bool diag = (int)(i / n) == (int)(i % n);
        second[i] = (mode == 3) ? ((diag ? 3.f : 0.f) - y) * 0.5f : (mode == 1) ? g[i] / d : (diag ? dv : 0.f);
    }
    if (loss.loss_out && blockIdx.x == 0) w2_loss_block(loss, scratch);
}

// ------------------------------------------------------------------------------------------------
// ContentLossMSE (style_transfer.py:119-126) under Scale(weight): value and gradient in one pass.
// In-kernel final reduction ("last block"): every block writes its partial sums, then takes a ticket; the block
// that draws the last one sums all partials in index order (deterministic for a given grid) and writes the loss.
// Saves the second launch - a single wave that, next to the trunk's persistent convolution workgroups, used to
// wait up to 0.7 ms for a free CU at 2048^2.  The partials are handed over write-through: sc1 stores, a wait, the ticket - no
// release fence, whose write-back of the XCD L2 (the 4 KB of gradient each of the 2048 workgroups has just dirtied) was most of
// this kernel's time at 512^2; the last block acquires at agent scope (LastBlock / last_block_arrives, st_common.h, which
// every kernel with such a sum shares; profiles/last_block.md).
// ACC (general closure, st_taps.hip): the layer is a style layer as well, whose head has WRITTEN grad - this term's is added.
template <bool ACC>
__global__ __launch_bounds__(256) void content_mse_kernel(const float* __restrict__ feat,
                                                          const float* __restrict__ target, long long count,
                                                          float weight, float norm, float* __restrict__ grad,
                                                          float* __restrict__ partials, LastBlock lb,
                                                          float final_count, float* __restrict__ loss_out) {
#pragma clang fp contract(off)
    __shared__ float scratch[4];
    __shared__ bool is_last;
    float s = 0.f;
    if ((count & 3) == 0) {           // 16-byte accesses: three streams of 4 B per element, HBM-bound
        const long long n4 = count >> 2;
        const f32x4* f4 = reinterpret_cast<const f32x4*>(feat);
        const f32x4* t4 = reinterpret_cast<const f32x4*>(target);
        f32x4* g4 = reinterpret_cast<f32x4*>(grad);
        for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
            const f32x4 f = f4[i], t = t4[i];
            f32x4 g;
            if (ACC) g = g4[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d = f[k] - t[k];
                s += d * d;
                const float v = (norm * d) * weight;      // mse_loss_backward: (2/numel) * (x - t) * grad_out
                g[k] = ACC ? g[k] + v : v;
            }
            g4[i] = g;
        }
    } else {
        for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
            const float d = feat[i] - target[i];
            s += d * d;
            const float v = (norm * d) * weight;
            grad[i] = ACC ? grad[i] + v : v;
        }
    }
    s = block_sum_256(s, scratch);
    const float mine[1] = {s};
    if (!last_block_arrives(lb, &is_last, partials + blockIdx.x, mine)) return;
    float t = 0.f;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) t += partials[i];
    t = block_sum_256(t, scratch);
    if (threadIdx.x == 0) loss_out[0] = (t / final_count) * weight;
}
__global__ __launch_bounds__(64) void content_mse_final_kernel(const float* __restrict__ partials, int nparts,
                                                               float count, float weight,
                                                               float* __restrict__ loss_out) {
    float s = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 64) s += partials[i];
    s = wave_sum(s);
    if (threadIdx.x == 0) loss_out[0] = (s / count) * weight;
}

// ------------------------------------------------------------------------------------------------
// ScaledMSELoss (style_transfer.py:93-106) under Scale(weight): the reference's ContentLoss (:109-116, x = the features, t =
// their target) and StyleLoss (:129-142, x = the Gram matrix F F^T / N, t = the target Gram matrix).
//   d = x - t,  S2 = sum d^2,  S1 = sum |d| + eps,  L = S2 / S1,  term = weight L
// Gradient, derived once: dL/dd = (dS2/dd) / S1 - (S2 / S1^2) dS1/dd = 2 d / S1 - (L / S1) sgn d = (2 d - L sgn d) / S1, with
// sgn 0 = 0 as torch's abs backward has it.  Where x and t are both zero (a ReLU's zeros) d is exactly zero and so is the
// gradient; when EVERY d is zero S2 = 0, S1 = eps, L = 0 and every gradient is (0 - 0) / eps = 0: nothing becomes NaN.
//   content:  the tap's seed is  weight (2 d - L sgn d) / S1
//   Gram:     with D = dL/dG,  G = F F^T / N  gives  dF = (weight / N) (D + D^T) F.  D + D^T is formed explicitly
//             (gram_grad_finish_kernel, as style_grad_finish_kernel forms a + b): the computed Gram matrix need not be
//             symmetric bit for bit.  The product with F is the W2 heads' 1x1 step with a zero bias (style_head_gradient).
// The totals need every element before any gradient can be formed, so a term is two launches: the sums - per-block partials,
// then the last block by ticket adds them in block order, as content_mse_kernel does - and the gradient.  No floating-point
// atomics: a given grid always adds in the same order.
__device__ __forceinline__ float scaled_mse_slope(float d, float level, float s1) {
#pragma clang fp contract(off)
    const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    return (2.f * d - level * sg) / s1;
}
// totals[0] = S2, totals[1] = S1 (eps included); loss_out[0] = weight S2 / S1.  partials: 2 floats per block.
__global__ __launch_bounds__(256) void scaled_mse_sums_kernel(const float* __restrict__ x, const float* __restrict__ target,
                                                              long long count, float weight, float eps,
                                                              float* __restrict__ partials, LastBlock lb,
                                                              float* __restrict__ totals, float* __restrict__ loss_out) {
#pragma clang fp contract(off)
    __shared__ float scratch[4];
    __shared__ bool is_last;
    float s2 = 0.f, s1 = 0.f;
    if ((count & 3) == 0) {           // 16-byte accesses: two streams of 4 B per element
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
    const float mine[2] = {s2, s1};
    if (!last_block_arrives(lb, &is_last, partials + 2 * blockIdx.x, mine)) return;
    float t2 = 0.f, t1 = 0.f;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) {
        t2 += partials[2 * i];
        t1 += partials[2 * i + 1];
    }
    t2 = block_sum_256(t2, scratch);
    t1 = block_sum_256(t1, scratch);
    if (threadIdx.x == 0) {
        const float sum_abs = t1 + eps;
        totals[0] = t2;
        totals[1] = sum_abs;
        loss_out[0] = (t2 / sum_abs) * weight;
    }
}
// the content seed: grad = (or, ACC: +=) weight (2 d - L sgn d) / S1.  ACC as content_mse_kernel's.
template <bool ACC>
__global__ __launch_bounds__(256) void scaled_mse_grad_kernel(const float* __restrict__ feat, const float* __restrict__ target,
                                                              long long count, float weight,
                                                              const float* __restrict__ totals, float* __restrict__ grad) {
#pragma clang fp contract(off)
    const float s1 = totals[1];
    const float level = totals[0] / s1;
    if ((count & 3) == 0) {           // 16-byte accesses: three (ACC: four) streams of 4 B per element, HBM-bound
        const long long n4 = count >> 2;
        const f32x4* f4 = reinterpret_cast<const f32x4*>(feat);
        const f32x4* t4 = reinterpret_cast<const f32x4*>(target);
        f32x4* g4 = reinterpret_cast<f32x4*>(grad);
        for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
            const f32x4 f = f4[i], t = t4[i];
            f32x4 g;
            if (ACC) g = g4[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float v = scaled_mse_slope(f[k] - t[k], level, s1) * weight;
                g[k] = ACC ? g[k] + v : v;
            }
            g4[i] = g;
        }
    } else {
        for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
            const float v = scaled_mse_slope(feat[i] - target[i], level, s1) * weight;
            grad[i] = ACC ? grad[i] + v : v;
        }
    }
}
// ------------------------------------------------------------------------------------------------
// The content terms under a spatial weight map (st_plan_set_content_mask, include/st_amd.h): the tap is [C][npix] flat and
// element i is weighed by wmap[i % npix], the map at the tap's level of the pyramid; the normalisers stay the element count
// (mse) and the weighted sums (scaled_mse).
//   mse:         term = weight sum_i w d^2 / count,                         seed = weight (2 / count) w d
//   scaled_mse:  S2 = sum w d^2, S1 = sum w |d| + eps, term = weight S2 / S1, seed = weight w (2 d - L sgn d) / S1, L = S2 / S1
// Siblings of the three kernels above with their structure - 16-byte groups where npix % 4 == 0 (a group then lies in one
// channel row and the map's group is aligned), one element at a time otherwise; per-block partials, the ticket, the last block's
// fixed-order sum.  A thread's pixel index is carried along its grid-stride loop (one 64-bit remainder before the loop, an add
// and a compare per step), so there is no division per element.  The map is read C times and stays in L2: the launches remain
// three-stream HBM-bound passes.  A map of ones gives the unweighted kernels' bits (1 * x = x, same operation order).
struct MapWalk {
    long long pos, step, period;
    __device__ __forceinline__ MapWalk(long long first, long long stride, long long n) : pos(first % n), step(stride % n), period(n) {}
    __device__ __forceinline__ void next() {
        pos += step;
        if (pos >= period) pos -= period;
    }
};
template <bool ACC>
__global__ __launch_bounds__(256) void content_mse_w_kernel(const float* __restrict__ feat, const float* __restrict__ target,
                                                            const float* __restrict__ wmap, long long count, long long npix,
                                                            float weight, float norm, float* __restrict__ grad,
                                                            float* __restrict__ partials, LastBlock lb, float final_count,
                                                            float* __restrict__ loss_out) {
#pragma clang fp contract(off)
    __shared__ float scratch[4];
    __shared__ bool is_last;
    float s = 0.f;
    const long long first = blockIdx.x * 256ll + threadIdx.x, stride = (long long)gridDim.x * 256;
    if ((npix & 3) == 0) {
        const long long n4 = count >> 2;
        const f32x4* f4 = reinterpret_cast<const f32x4*>(feat);
        const f32x4* t4 = reinterpret_cast<const f32x4*>(target);
        const f32x4* w4 = reinterpret_cast<const f32x4*>(wmap);
        f32x4* g4 = reinterpret_cast<f32x4*>(grad);
        MapWalk px(first, stride, npix >> 2);
        for (long long i = first; i < n4; i += stride, px.next()) {
            const f32x4 f = f4[i], t = t4[i], w = w4[px.pos];
            f32x4 g;
            if (ACC) g = g4[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d = f[k] - t[k];
                s += w[k] * (d * d);
                const float v = (norm * (w[k] * d)) * weight;
                g[k] = ACC ? g[k] + v : v;
            }
            g4[i] = g;
        }
    } else {
        MapWalk px(first, stride, npix);
        for (long long i = first; i < count; i += stride, px.next()) {
            const float d = feat[i] - target[i], w = wmap[px.pos];
            s += w * (d * d);
            const float v = (norm * (w * d)) * weight;
            grad[i] = ACC ? grad[i] + v : v;
        }
    }
    s = block_sum_256(s, scratch);
    const float mine[1] = {s};
    if (!last_block_arrives(lb, &is_last, partials + blockIdx.x, mine)) return;
    float t = 0.f;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) t += partials[i];
    t = block_sum_256(t, scratch);
    if (threadIdx.x == 0) loss_out[0] = (t / final_count) * weight;
}
__global__ __launch_bounds__(256) void scaled_mse_sums_w_kernel(const float* __restrict__ x, const float* __restrict__ target,
                                                                const float* __restrict__ wmap, long long count, long long npix,
                                                                float weight, float eps, float* __restrict__ partials,
                                                                LastBlock lb, float* __restrict__ totals,
                                                                float* __restrict__ loss_out) {
#pragma clang fp contract(off)
    __shared__ float scratch[4];
    __shared__ bool is_last;
    float s2 = 0.f, s1 = 0.f;
    const long long first = blockIdx.x * 256ll + threadIdx.x, stride = (long long)gridDim.x * 256;
    if ((npix & 3) == 0) {
        const long long n4 = count >> 2;
        const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
        const f32x4* t4 = reinterpret_cast<const f32x4*>(target);
        const f32x4* w4 = reinterpret_cast<const f32x4*>(wmap);
        MapWalk px(first, stride, npix >> 2);
        for (long long i = first; i < n4; i += stride, px.next()) {
            const f32x4 f = x4[i], t = t4[i], w = w4[px.pos];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d = f[k] - t[k];
                s2 += w[k] * (d * d);
                s1 += w[k] * fabsf(d);
            }
        }
    } else {
        MapWalk px(first, stride, npix);
        for (long long i = first; i < count; i += stride, px.next()) {
            const float d = x[i] - target[i], w = wmap[px.pos];
            s2 += w * (d * d);
            s1 += w * fabsf(d);
        }
    }
    s2 = block_sum_256(s2, scratch);
    s1 = block_sum_256(s1, scratch);
    const float mine[2] = {s2, s1};
    if (!last_block_arrives(lb, &is_last, partials + 2 * blockIdx.x, mine)) return;
    float t2 = 0.f, t1 = 0.f;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) {
        t2 += partials[2 * i];
        t1 += partials[2 * i + 1];
    }
    t2 = block_sum_256(t2, scratch);
    t1 = block_sum_256(t1, scratch);
    if (threadIdx.x == 0) {
        const float sum_abs = t1 + eps;
        totals[0] = t2;
        totals[1] = sum_abs;
        loss_out[0] = (t2 / sum_abs) * weight;
    }
}
template <bool ACC>
__global__ __launch_bounds__(256) void scaled_mse_grad_w_kernel(const float* __restrict__ feat, const float* __restrict__ target,
                                                                const float* __restrict__ wmap, long long count, long long npix,
                                                                float weight, const float* __restrict__ totals,
                                                                float* __restrict__ grad) {
#pragma clang fp contract(off)
    const float s1 = totals[1];
    const float level = totals[0] / s1;
    const long long first = blockIdx.x * 256ll + threadIdx.x, stride = (long long)gridDim.x * 256;
    if ((npix & 3) == 0) {
        const long long n4 = count >> 2;
        const f32x4* f4 = reinterpret_cast<const f32x4*>(feat);
        const f32x4* t4 = reinterpret_cast<const f32x4*>(target);
        const f32x4* w4 = reinterpret_cast<const f32x4*>(wmap);
        f32x4* g4 = reinterpret_cast<f32x4*>(grad);
        MapWalk px(first, stride, npix >> 2);
        for (long long i = first; i < n4; i += stride, px.next()) {
            const f32x4 f = f4[i], t = t4[i], w = w4[px.pos];
            f32x4 g;
            if (ACC) g = g4[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float v = (w[k] * scaled_mse_slope(f[k] - t[k], level, s1)) * weight;
                g[k] = ACC ? g[k] + v : v;
            }
            g4[i] = g;
        }
    } else {
        MapWalk px(first, stride, npix);
        for (long long i = first; i < count; i += stride, px.next()) {
            const float v = (wmap[px.pos] * scaled_mse_slope(feat[i] - target[i], level, s1)) * weight;
            grad[i] = ACC ? grad[i] + v : v;
        }
    }
}
// The Gram head's (Ssym, b) for the 1x1 step, one workgroup per row c of the n x n matrix (n = 64 ... 512):
//   ssym[c][d] = (weight / npix) (D[c][d] + D[d][c]),  D = (2 (G - G_t) - L sgn(G - G_t)) / S1;   bvec[c] = 0
__global__ __launch_bounds__(256) void gram_grad_finish_kernel(const float* __restrict__ gram, const float* __restrict__ gram_t,
                                                               const float* __restrict__ totals, int n, float weight,
                                                               float npix, float* __restrict__ ssym, float* __restrict__ bvec,
                                                               unsigned int* __restrict__ ssym_amax) {
#pragma clang fp contract(off)
    const int c = blockIdx.x;
    const float s1 = totals[1];
    const float level = totals[0] / s1;
    const float wn = weight / npix;
    unsigned int amax = 0;
    for (int d = threadIdx.x; d < n; d += 256) {
        const size_t cd = (size_t)c * n + d, dc = (size_t)d * n + c;
        const float a = scaled_mse_slope(gram[cd] - gram_t[cd], level, s1);
        const float b = scaled_mse_slope(gram[dc] - gram_t[dc], level, s1);
        const float sv = (a + b) * wn;
        ssym[cd] = sv;
        const unsigned int bits = abs_bits(sv);
        amax = bits > amax ? bits : amax;
    }
    if (ssym_amax) amax_commit(amax, ssym_amax);      // bound on max |Ssym| for the fp16x3 1x1 convolution (every lane arrives)
    if (threadIdx.x == 0) bvec[c] = 0.f;
}

// The seeding of st_plan_backward (the backward of VGGFeatures.forward, style_transfer.py:78-90, for gradients that arrive
// at the taps from outside): an external tap gradient enters the node's gradient buffer.
//   ACC == false: g = ext.  Ahead of the data-gradient launch that accumulates into the node - that launch masks the total -
//                 and at the top of the pass;
//   ACC == true:  g += ext.  Behind a pooling backward, which WRITES its input node's gradient (masked already).
//   relu_out != nullptr: the result is masked by (relu_out > 0), the node's own threshold_backward - the top of the pass, where
//                 nothing accumulates afterwards, and the ACC form (a select on both shares is the select on their sum).
//   bound != nullptr (fp16x3 networks): max |g| of what this launch leaves goes into the bound the consuming data gradient
//                 scales its operand by (amax_commit).
// n4 16-byte groups first, then the count - 4 n4 elements behind them one by one (n4 == 0: a pointer is not 16-byte aligned).
template <bool ACC>
__global__ __launch_bounds__(256) void seed_grad_kernel(const float* __restrict__ ext, const float* __restrict__ relu_out,
                                                        float* __restrict__ g, long long count, long long n4,
                                                        unsigned int* __restrict__ bound) {
#pragma clang fp contract(off)
    unsigned int amax = 0;
    const long long first = blockIdx.x * 256ll + threadIdx.x, stride = (long long)gridDim.x * 256;
    const f32x4* ext4 = reinterpret_cast<const f32x4*>(ext);
    const f32x4* relu4 = reinterpret_cast<const f32x4*>(relu_out);
    f32x4* g4 = reinterpret_cast<f32x4*>(g);
    for (long long i = first; i < n4; i += stride) {
        f32x4 v = ext4[i];
        if (ACC) {
            const f32x4 o = g4[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] += o[k];
        }
        if (relu_out) {
            const f32x4 m = relu4[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = m[k] > 0.f ? v[k] : 0.f;
        }
        g4[i] = v;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned int bits = abs_bits(v[k]);
            amax = bits > amax ? bits : amax;
        }
    }
    for (long long i = 4 * n4 + first; i < count; i += stride) {
        float v = ext[i];
        if (ACC) v += g[i];
        if (relu_out) v = relu_out[i] > 0.f ? v : 0.f;
        g[i] = v;
        const unsigned int bits = abs_bits(v);
        amax = bits > amax ? bits : amax;
    }
    if (bound) amax_commit(amax, bound);       // (every lane arrives here: grid-stride loops, no early return)
}

// W2 head scalars (StyleLossW2.forward, style_transfer.py:178-181) for one layer; single workgroup.
__global__ __launch_bounds__(256) void style_loss_value_kernel(W2LossJob job) {
    __shared__ float scratch[4];
    w2_loss_block(job, scratch);
}

// One workgroup per row c of dcov = g + (weight/n) I:
//   ssym[c][d] = (dcov[c][d] + dcov[d][c]) / npix
//   bvec[c]    = (2 (weight/n) (mu - mu_t)[c] - sum_d (dcov[c][d] + dcov[d][c]) mu[d]) / npix
__global__ __launch_bounds__(256) void style_grad_finish_kernel(const float* __restrict__ g,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ mean_t, int n,
                                                                float weight, float npix,
                                                                float* __restrict__ ssym,
                                                                float* __restrict__ bvec,
                                                                unsigned int* __restrict__ ssym_amax) {
#pragma clang fp contract(off)
    __shared__ float scratch[4];
    const int c = blockIdx.x;
    const float wn = weight / (float)n;
    float dot = 0.f;
    unsigned int amax = 0;
    for (int d = threadIdx.x; d < n; d += 256) {
        float a = g[(size_t)c * n + d], b = g[(size_t)d * n + c];
        if (d == c) { a += wn; b += wn; }
        const float sym = a + b;
        const float sv = sym / npix;
        ssym[(size_t)c * n + d] = sv;
        const unsigned int bits = abs_bits(sv);
        amax = bits > amax ? bits : amax;
        dot += sym * mean[d];
    }
    if (ssym_amax) amax_commit(amax, ssym_amax);      // bound on max |Ssym| for the fp16x3 1x1 convolution
    dot = block_sum_256(dot, scratch);
    if (threadIdx.x == 0) bvec[c] = ((wn * 2.f) * (mean[c] - mean_t[c]) - dot) / npix;
}

// ------------------------------------------------------------------------------------------------
// TVLoss (style_transfer.py:184-195): value and gradient.  P(a, b) is the replicate-padded image in
// padded coordinates a in [-1, H], b in [-1, W].  Differences:
//   D1(a,b) = P(a,b+1) - P(a,b), D2(a,b) = P(a+1,b) - P(a,b)            on [0,H) x [0,W)
//   D3(i,j) = P(i,j) - P(i-1,j-1), D4(i,j) = P(i,j-1) - P(i-1,j)        on [0,H] x [0,W]
//   loss = 2 (mean(D1^2)/3 + mean(D2^2)/3 + mean(D3^2)/12 + mean(D4^2)/12)
// The gradient w.r.t. the padding ring folds back onto the nearest image pixel.
struct TVImage {
    const float* p;        // this channel of the local strip [H][W]
    int H, W;              // local rows, width
    int row0, Hg;          // global row of local row 0, global height
    const float* top;      // neighbour rows (this channel) or nullptr at the global border
    const float* bot;
    __device__ __forceinline__ float at(int a, int b) const {   // a = LOCAL row index, may be -1 / H
        b = min(max(b, 0), W - 1);
        if (a < 0) {
            if (top) return top[b];
            a = 0;
        } else if (a >= H) {
            if (bot) return bot[b];
            a = H - 1;
        }
        return p[(size_t)a * W + b];
    }
};

// gradient w.r.t. the padded image at local row a (global row a + row0), column b
__device__ __forceinline__ float tv_dP(const TVImage& im, int a, int b, float k1, float k3) {
#pragma clang fp contract(off)
    const int H = im.Hg, W = im.W;
    const int ag = a + im.row0;
    const float c = im.at(a, b);
    float g = 0.f;
    const bool row_in = (ag >= 0 && ag < H), col_in = (b >= 0 && b < W);
    if (row_in) {
        if (b >= 1 && b <= W) g += k1 * (c - im.at(a, b - 1));
        if (col_in) g -= k1 * (im.at(a, b + 1) - c);
    }
    if (col_in) {
        if (ag >= 1 && ag <= H) g += k1 * (c - im.at(a - 1, b));
        if (row_in) g -= k1 * (im.at(a + 1, b) - c);
    }
    if (ag >= 0 && b >= 0) g += k3 * (c - im.at(a - 1, b - 1));            // D3(a, b)
    if (ag <= H - 1 && b <= W - 1) g -= k3 * (im.at(a + 1, b + 1) - c);    // D3(a+1, b+1)
    if (ag >= 0 && b <= W - 1) g += k3 * (c - im.at(a - 1, b + 1));        // D4(a, b+1)
    if (ag <= H - 1 && b >= 0) g -= k3 * (im.at(a + 1, b - 1) - c);        // D4(a+1, b)
    return g;
}

// One pixel, any position (global borders: the padding ring's gradient folds onto it; strips: neighbour rows come
// from the halo): gradient + the squared differences this pixel owns.
__device__ __forceinline__ float tv_pixel_generic(const TVImage& im, int y, int x, int yg, int Hg, int W, float k1,
                                                  float k3, float& s1, float& s2, float& s3, float& s4) {
#pragma clang fp contract(off)
    // gradient: this pixel plus the GLOBAL padding-ring positions that replicate it
    float g = 0.f;
    for (int ry = -1; ry <= 1; ++ry) {
        if (ry != 0 && !((ry < 0 && yg == 0) || (ry > 0 && yg == Hg - 1))) continue;
        for (int rx = -1; rx <= 1; ++rx) {
            if (rx != 0 && !((rx < 0 && x == 0) || (rx > 0 && x == W - 1))) continue;
            g += tv_dP(im, y + ry, x + rx, k1, k3);
        }
    }
    // value: every difference is owned by exactly one pixel
    const float c = im.at(y, x);
    const float d1 = im.at(y, x + 1) - c, d2 = im.at(y + 1, x) - c;
    s1 += d1 * d1;
    s2 += d2 * d2;
    for (int iy = y; iy <= ((yg == Hg - 1) ? y + 1 : y); ++iy)
        for (int jx = x; jx <= ((x == W - 1) ? W : x); ++jx) {
            const float d3 = im.at(iy, jx) - im.at(iy - 1, jx - 1);
            const float d4 = im.at(iy, jx - 1) - im.at(iy - 1, jx);
            s3 += d3 * d3;
            s4 += d4 * d4;
        }
    return g;
}

// Two kernels.  tv_interior_kernel: HBM-bound streaming pass - reads the image once (the 3 x 3 neighbourhoods come from
// L1 / L2), writes the gradient once.  A thread owns 4 consecutive pixels of a row: three 16-byte loads + six edge
// scalars, one 16-byte store; rows are dealt to workgroups and a row's groups to the threads, so there is no division
// per element.  Its formula is tv_dP with every range condition true, in the same operation order: identical bits to
// the generic path.  It skips the first / last row and the first / last group of every row; tv_border_kernel takes
// those (and everything when the width is not a multiple of 4) with tv_pixel_generic - global borders fold the
// padding ring, strip borders read the neighbours' halo rows - and its last block finishes the four sums of BOTH
// kernels.  (Round 1: one pixel per thread of a 256-block grid-stride loop, nine tv_dP evaluations and two 64-bit
// divisions per pixel: 991 + 709 us in situ at 2048^2.  One kernel with both paths needed 125 registers: 141 us
// isolated; split: see profiles/r02_side_kernels.md.)
// VAR (ST_TV_VARIANT; profiles/r05_tv_hazard.md - the flaky TV term of round 4, root-caused in round 5):
//   1 = SHIPPED.  The four accumulators are pinned to registers of their own after every update (an empty asm statement), so
//       that the SLP vectoriser cannot pair (d1, d2) / (d3, d4) into packed-FP32 operations.
//   0 = the round-1 ... 4 code, kept as the REPRODUCER: the optimiser turns `d1 = M[j+2] - cc, d2 = D[j+1] - cc` of pixel j = 0
//       into ONE `v_pk_add_f32 vdst, vsrc0, vsrc1 op_sel:[0,1] neg_lo:[0,1] neg_hi:[0,1]` (both lanes subtract the HIGH half of
//       vsrc1).  On MI355X that instruction returned `vsrc0 - 0` in its LOW lane for lanes 48 - 63 of a wave - i.e. d1 = M[2]
//       instead of M[2] - M[1], identified to 1e-8 per thread (tools/tv_hazard_threads.py) - in 55 - 75 % of the FIRST
//       closures of a fresh plan when the kernel ran at the tail of a head stream beside the launch-per-product
//       Newton-Schulz chains, never on a warm plan, never at the start of the iteration.  Neither aligned-only loads, nor a
//       full s_waitcnt vmcnt(0) + 16 idle cycles before the first use, nor another block reduction changed the rate (variants
//       2, 4, 5, 6 of the investigation); the variant WITHOUT that one instruction never failed (0 / 144 closures).  It is the
//       only packed-FP32 instruction with a cross-half op_sel in the whole library; build.py now refuses to build a kernel
//       that contains one (hazard guard), this reproducer and its dumping twin excepted.
//   3 = variant 0 + every thread's four accumulators and its group count written to `dbg` ([blocks][256][5]).
template <int VAR>
__global__ __launch_bounds__(256) void tv_interior_kernel(const float* __restrict__ image, int H, int W, float k1,
                                                          float k3, float* __restrict__ grad,
                                                          float* __restrict__ partials, float* __restrict__ dbg) {
#pragma clang fp contract(off)
    __shared__ float scratch[4];
    float s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
    int visited = 0;
    const int gpr = W >> 2;                                  // groups of 4 pixels per row
    int tpr = 256;                                           // threads sharing a row: power of two covering it
    while (tpr > 1 && (tpr >> 1) >= gpr) tpr >>= 1;
    const int rpb = 256 / tpr;
    const int lr = threadIdx.x / tpr, gx = threadIdx.x % tpr;
    const int rows = 3 * H;
    for (int row0 = blockIdx.x * rpb; row0 < rows; row0 += gridDim.x * rpb) {
        const int row = row0 + lr;
        const int ch = row / H;
        const int y = row - ch * H;
        if (row >= rows || y < 1 || y > H - 2) continue;
        const float* rowp = image + (size_t)ch * H * W + (size_t)y * W;
        float* growp = grad + (size_t)ch * H * W + (size_t)y * W;
        for (int g4 = gx; g4 < gpr; g4 += tpr) {
            if (g4 == 0 || g4 == gpr - 1) continue;
            const float* c = rowp + 4 * g4;
            const f32x4 up = *reinterpret_cast<const f32x4*>(c - W);
            const f32x4 mid = *reinterpret_cast<const f32x4*>(c);
            const f32x4 dn = *reinterpret_cast<const f32x4*>(c + W);
            const float U[6] = {c[-W - 1], up[0], up[1], up[2], up[3], c[-W + 4]};
            const float M[6] = {c[-1], mid[0], mid[1], mid[2], mid[3], c[4]};
            const float D[6] = {c[W - 1], dn[0], dn[1], dn[2], dn[3], c[W + 4]};
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float cc = M[j + 1];
                float g = 0.f;
                g += k1 * (cc - M[j]);
                g -= k1 * (M[j + 2] - cc);
                g += k1 * (cc - U[j + 1]);
                g -= k1 * (D[j + 1] - cc);
                g += k3 * (cc - U[j]);               // D3(a, b)
                g -= k3 * (D[j + 2] - cc);           // D3(a+1, b+1)
                g += k3 * (cc - U[j + 2]);           // D4(a, b+1)
                g -= k3 * (D[j] - cc);               // D4(a+1, b)
                o[j] = g;
                const float d1 = M[j + 2] - cc, d2 = D[j + 1] - cc, d3 = cc - U[j], d4 = M[j] - U[j + 1];
                s1 += d1 * d1;
                s2 += d2 * d2;
                s3 += d3 * d3;
                s4 += d4 * d4;
                if (VAR == 1) asm volatile("" : "+v"(s1), "+v"(s2), "+v"(s3), "+v"(s4));
            }
            *reinterpret_cast<f32x4*>(growp + 4 * g4) = o;
            if (VAR == 3) ++visited;
        }
    }
    if (VAR == 3) {
        float* d = dbg + ((size_t)blockIdx.x * 256 + threadIdx.x) * 5;
        d[0] = s1; d[1] = s2; d[2] = s3; d[3] = s4; d[4] = (float)visited;
    }
    s1 = block_sum_256(s1, scratch);
    s2 = block_sum_256(s2, scratch);
    s3 = block_sum_256(s3, scratch);
    s4 = block_sum_256(s4, scratch);
    if (threadIdx.x == 0) {
        partials[blockIdx.x * 4 + 0] = s1;
        partials[blockIdx.x * 4 + 1] = s2;
        partials[blockIdx.x * 4 + 2] = s3;
        partials[blockIdx.x * 4 + 3] = s4;
    }
}

// interior != 0: only the groups tv_interior_kernel skipped; partials holds `first` blocks of that kernel already and
// this one appends its own.  The last block sums all of them in index order (lb.ticket != nullptr).
__global__ __launch_bounds__(256) void tv_border_kernel(const float* __restrict__ image, int H, int W, float k1,
                                                        float k3, float* __restrict__ grad,
                                                        float* __restrict__ partials, StripInfo strip, int interior,
                                                        int first, LastBlock lb, float fin_n, float fin_n2,
                                                        float fin_weight, float* __restrict__ loss_out) {
#pragma clang fp contract(off)
    __shared__ float scratch[4];
    __shared__ bool is_last;
    const int Hg = strip.global_height;
    float s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
    auto pixel = [&](int ch, int y, int x) __attribute__((always_inline)) {
        TVImage im{image + (size_t)ch * H * W, H, W, strip.row0, Hg,
                   (strip.halo && strip.has_up) ? strip.halo + (size_t)ch * W : nullptr,
                   (strip.halo && strip.has_down) ? strip.halo + (size_t)(3 + ch) * W : nullptr};
        grad[(size_t)ch * H * W + (size_t)y * W + x] = tv_pixel_generic(im, y, x, y + strip.row0, Hg, W, k1, k3, s1, s2, s3, s4);
    };
    if (interior) {
        const int gpr = W >> 2;
        const int per_ch = 2 * gpr + 2 * (H - 2);              // groups of the first / last row + both ends of the others
        const int total = 3 * per_ch * 4;                      // ... as pixels
        for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
            const int gi = i >> 2, j = i & 3;
            const int ch = gi / per_ch, k = gi - ch * per_ch;
            int y, g4;
            if (k < gpr) { y = 0; g4 = k; }
            else if (k < 2 * gpr) { y = H - 1; g4 = k - gpr; }
            else { y = 1 + ((k - 2 * gpr) >> 1); g4 = ((k - 2 * gpr) & 1) ? gpr - 1 : 0; }
            pixel(ch, y, 4 * g4 + j);
        }
    } else {
        const int total = 3 * H * W;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
            const int x = i % W, r = i / W;
            pixel(r / H, r % H, x);
        }
    }
    s1 = block_sum_256(s1, scratch);
    s2 = block_sum_256(s2, scratch);
    s3 = block_sum_256(s3, scratch);
    s4 = block_sum_256(s4, scratch);
    const float mine[4] = {s1, s2, s3, s4};
    if (!last_block_arrives(lb, &is_last, partials + (size_t)(first + blockIdx.x) * 4, mine)) return;
    const int nparts = first + (int)gridDim.x;
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < nparts; i += 256)
        for (int k = 0; k < 4; ++k) t[k] += partials[i * 4 + k];
    for (int k = 0; k < 4; ++k) t[k] = block_sum_256(t[k], scratch);
    if (threadIdx.x == 0) {
        const float d1 = (t[0] / fin_n) / 3.f, d2 = (t[1] / fin_n) / 3.f;
        const float d3 = (t[2] / fin_n2) / 12.f, d4 = (t[3] / fin_n2) / 12.f;
        loss_out[0] = (2.f * (((d1 + d2) + d3) + d4)) * fin_weight;
    }
}
// ------------------------------------------------------------------------------------------------
// TVLoss under a spatial weight map (st_plan_set_tv_mask, include/st_amd.h): every squared difference is weighed by the mean
// of the map at its two end points, the map replicate-padded as the image is; the counts in the denominators are unchanged.
//   loss = 2 (sum e1 D1^2 / (3 n) + sum e2 D2^2 / (3 n) + sum e3 D3^2 / (12 n2) + sum e4 D4^2 / (12 n2)),  e = (w_a + w_b) / 2
// so d loss / d P through a difference is the unweighted one times e.  The two kernels below are tv_interior_kernel<1> and
// tv_border_kernel (whole images only) on the same split, reading the map's 3 x 3 neighbourhood beside the image's: every
// k (c - x) of the gradient becomes k (e (c - x)) and every s += d d becomes s += e (d d).  A map of ones gives the unweighted
// kernels' bits ((1 + 1) / 2 = 1, 1 * x = x).  The four sums are four weighted sums; partials, ticket and the finish are shared.
struct TVMap {
    const float* p;        // [H][W]
    int H, W;
    __device__ __forceinline__ float at(int a, int b) const {
        a = min(max(a, 0), H - 1);
        b = min(max(b, 0), W - 1);
        return p[(size_t)a * W + b];
    }
};
// (the sum is one VALU addition of its own: left to the optimiser, the SLP vectoriser pairs a pixel's edge sums wc + w_a,
// wc + w_b into ONE packed-FP32 addition with a cross-half op_sel on wc - the instruction of profiles/r05_tv_hazard.md, which
// build.py's hazard guard refuses)
__device__ __forceinline__ float tv_edge(float wa, float wb) {
#pragma clang fp contract(off)
    float sum;
    asm("v_add_f32 %0, %1, %2" : "=v"(sum) : "v"(wa), "v"(wb));
    return 0.5f * sum;
}

// tv_dP with the edge weights (im: a whole image, row0 = 0, no halo)
__device__ __forceinline__ float tv_dP_w(const TVImage& im, const TVMap& wm, int a, int b, float k1, float k3) {
#pragma clang fp contract(off)
    const int H = im.H, W = im.W;
    const float c = im.at(a, b), wc = wm.at(a, b);
    float g = 0.f;
    const bool row_in = (a >= 0 && a < H), col_in = (b >= 0 && b < W);
    if (row_in) {
        if (b >= 1 && b <= W) g += k1 * (tv_edge(wc, wm.at(a, b - 1)) * (c - im.at(a, b - 1)));
        if (col_in) g -= k1 * (tv_edge(wc, wm.at(a, b + 1)) * (im.at(a, b + 1) - c));
    }
    if (col_in) {
        if (a >= 1 && a <= H) g += k1 * (tv_edge(wc, wm.at(a - 1, b)) * (c - im.at(a - 1, b)));
        if (row_in) g -= k1 * (tv_edge(wc, wm.at(a + 1, b)) * (im.at(a + 1, b) - c));
    }
    if (a >= 0 && b >= 0) g += k3 * (tv_edge(wc, wm.at(a - 1, b - 1)) * (c - im.at(a - 1, b - 1)));            // D3(a, b)
    if (a <= H - 1 && b <= W - 1) g -= k3 * (tv_edge(wc, wm.at(a + 1, b + 1)) * (im.at(a + 1, b + 1) - c));    // D3(a+1, b+1)
    if (a >= 0 && b <= W - 1) g += k3 * (tv_edge(wc, wm.at(a - 1, b + 1)) * (c - im.at(a - 1, b + 1)));        // D4(a, b+1)
    if (a <= H - 1 && b >= 0) g -= k3 * (tv_edge(wc, wm.at(a + 1, b - 1)) * (im.at(a + 1, b - 1) - c));        // D4(a+1, b)
    return g;
}

// tv_pixel_generic with the edge weights
__device__ __forceinline__ float tv_pixel_w(const TVImage& im, const TVMap& wm, int y, int x, float k1, float k3, float& s1,
                                            float& s2, float& s3, float& s4) {
#pragma clang fp contract(off)
    const int H = im.H, W = im.W;
    float g = 0.f;
    for (int ry = -1; ry <= 1; ++ry) {
        if (ry != 0 && !((ry < 0 && y == 0) || (ry > 0 && y == H - 1))) continue;
        for (int rx = -1; rx <= 1; ++rx) {
            if (rx != 0 && !((rx < 0 && x == 0) || (rx > 0 && x == W - 1))) continue;
            g += tv_dP_w(im, wm, y + ry, x + rx, k1, k3);
        }
    }
    const float c = im.at(y, x), wc = wm.at(y, x);
    const float d1 = im.at(y, x + 1) - c, d2 = im.at(y + 1, x) - c;
    s1 += tv_edge(wm.at(y, x + 1), wc) * (d1 * d1);
    s2 += tv_edge(wm.at(y + 1, x), wc) * (d2 * d2);
    for (int iy = y; iy <= ((y == H - 1) ? y + 1 : y); ++iy)
        for (int jx = x; jx <= ((x == W - 1) ? W : x); ++jx) {
            const float d3 = im.at(iy, jx) - im.at(iy - 1, jx - 1);
            const float d4 = im.at(iy, jx - 1) - im.at(iy - 1, jx);
            s3 += tv_edge(wm.at(iy, jx), wm.at(iy - 1, jx - 1)) * (d3 * d3);
            s4 += tv_edge(wm.at(iy, jx - 1), wm.at(iy - 1, jx)) * (d4 * d4);
        }
    return g;
}

__global__ __launch_bounds__(256) void tv_interior_w_kernel(const float* __restrict__ image, const float* __restrict__ wmap,
                                                            int H, int W, float k1, float k3, float* __restrict__ grad,
                                                            float* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ float scratch[4];
    float s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
    const int gpr = W >> 2;                                  // groups of 4 pixels per row
    int tpr = 256;                                           // threads sharing a row: power of two covering it
    while (tpr > 1 && (tpr >> 1) >= gpr) tpr >>= 1;
    const int rpb = 256 / tpr;
    const int lr = threadIdx.x / tpr, gx = threadIdx.x % tpr;
    const int rows = 3 * H;
    for (int row0 = blockIdx.x * rpb; row0 < rows; row0 += gridDim.x * rpb) {
        const int row = row0 + lr;
        const int ch = row / H;
        const int y = row - ch * H;
        if (row >= rows || y < 1 || y > H - 2) continue;
        const float* rowp = image + (size_t)ch * H * W + (size_t)y * W;
        const float* wrowp = wmap + (size_t)y * W;
        float* growp = grad + (size_t)ch * H * W + (size_t)y * W;
        for (int g4 = gx; g4 < gpr; g4 += tpr) {
            if (g4 == 0 || g4 == gpr - 1) continue;
            const float* c = rowp + 4 * g4;
            const float* m = wrowp + 4 * g4;
            const f32x4 up = *reinterpret_cast<const f32x4*>(c - W);
            const f32x4 mid = *reinterpret_cast<const f32x4*>(c);
            const f32x4 dn = *reinterpret_cast<const f32x4*>(c + W);
            const f32x4 wup = *reinterpret_cast<const f32x4*>(m - W);
            const f32x4 wmid = *reinterpret_cast<const f32x4*>(m);
            const f32x4 wdn = *reinterpret_cast<const f32x4*>(m + W);
            const float U[6] = {c[-W - 1], up[0], up[1], up[2], up[3], c[-W + 4]};
            const float M[6] = {c[-1], mid[0], mid[1], mid[2], mid[3], c[4]};
            const float D[6] = {c[W - 1], dn[0], dn[1], dn[2], dn[3], c[W + 4]};
            const float WU[6] = {m[-W - 1], wup[0], wup[1], wup[2], wup[3], m[-W + 4]};
            const float WM[6] = {m[-1], wmid[0], wmid[1], wmid[2], wmid[3], m[4]};
            const float WD[6] = {m[W - 1], wdn[0], wdn[1], wdn[2], wdn[3], m[W + 4]};
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float cc = M[j + 1], wc = WM[j + 1];
                float g = 0.f;
                g += k1 * (tv_edge(wc, WM[j]) * (cc - M[j]));
                g -= k1 * (tv_edge(wc, WM[j + 2]) * (M[j + 2] - cc));
                g += k1 * (tv_edge(wc, WU[j + 1]) * (cc - U[j + 1]));
                g -= k1 * (tv_edge(wc, WD[j + 1]) * (D[j + 1] - cc));
                g += k3 * (tv_edge(wc, WU[j]) * (cc - U[j]));               // D3(a, b)
                g -= k3 * (tv_edge(wc, WD[j + 2]) * (D[j + 2] - cc));       // D3(a+1, b+1)
                g += k3 * (tv_edge(wc, WU[j + 2]) * (cc - U[j + 2]));       // D4(a, b+1)
                g -= k3 * (tv_edge(wc, WD[j]) * (D[j] - cc));               // D4(a+1, b)
                o[j] = g;
                const float d1 = M[j + 2] - cc, d2 = D[j + 1] - cc, d3 = cc - U[j], d4 = M[j] - U[j + 1];
                s1 += tv_edge(WM[j + 2], wc) * (d1 * d1);
                s2 += tv_edge(WD[j + 1], wc) * (d2 * d2);
                s3 += tv_edge(wc, WU[j]) * (d3 * d3);
                s4 += tv_edge(WM[j], WU[j + 1]) * (d4 * d4);
                // (the accumulators pinned as in tv_interior_kernel<1>: no packed-FP32 pairing of the four updates)
                asm volatile("" : "+v"(s1), "+v"(s2), "+v"(s3), "+v"(s4));
            }
            *reinterpret_cast<f32x4*>(growp + 4 * g4) = o;
        }
    }
    s1 = block_sum_256(s1, scratch);
    s2 = block_sum_256(s2, scratch);
    s3 = block_sum_256(s3, scratch);
    s4 = block_sum_256(s4, scratch);
    if (threadIdx.x == 0) {
        partials[blockIdx.x * 4 + 0] = s1;
        partials[blockIdx.x * 4 + 1] = s2;
        partials[blockIdx.x * 4 + 2] = s3;
        partials[blockIdx.x * 4 + 3] = s4;
    }
}

__global__ __launch_bounds__(256) void tv_border_w_kernel(const float* __restrict__ image, const float* __restrict__ wmap,
                                                          int H, int W, float k1, float k3, float* __restrict__ grad,
                                                          float* __restrict__ partials, int interior, int first, LastBlock lb,
                                                          float fin_n, float fin_n2, float fin_weight,
                                                          float* __restrict__ loss_out) {
#pragma clang fp contract(off)
    __shared__ float scratch[4];
    __shared__ bool is_last;
    float s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
    const TVMap wm{wmap, H, W};
    auto pixel = [&](int ch, int y, int x) __attribute__((always_inline)) {
        TVImage im{image + (size_t)ch * H * W, H, W, 0, H, nullptr, nullptr};
        grad[(size_t)ch * H * W + (size_t)y * W + x] = tv_pixel_w(im, wm, y, x, k1, k3, s1, s2, s3, s4);
    };
    if (interior) {
        const int gpr = W >> 2;
        const int per_ch = 2 * gpr + 2 * (H - 2);              // groups of the first / last row + both ends of the others
        const int total = 3 * per_ch * 4;                      // ... as pixels
        for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
            const int gi = i >> 2, j = i & 3;
            const int ch = gi / per_ch, k = gi - ch * per_ch;
            int y, g4;
            if (k < gpr) { y = 0; g4 = k; }
            else if (k < 2 * gpr) { y = H - 1; g4 = k - gpr; }
            else { y = 1 + ((k - 2 * gpr) >> 1); g4 = ((k - 2 * gpr) & 1) ? gpr - 1 : 0; }
            pixel(ch, y, 4 * g4 + j);
        }
    } else {
        const int total = 3 * H * W;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
            const int x = i % W, r = i / W;
            pixel(r / H, r % H, x);
        }
    }
    s1 = block_sum_256(s1, scratch);
    s2 = block_sum_256(s2, scratch);
    s3 = block_sum_256(s3, scratch);
    s4 = block_sum_256(s4, scratch);
    const float mine[4] = {s1, s2, s3, s4};
    if (!last_block_arrives(lb, &is_last, partials + (size_t)(first + blockIdx.x) * 4, mine)) return;
    const int nparts = first + (int)gridDim.x;
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < nparts; i += 256)
        for (int k = 0; k < 4; ++k) t[k] += partials[i * 4 + k];
    for (int k = 0; k < 4; ++k) t[k] = block_sum_256(t[k], scratch);
    if (threadIdx.x == 0) {
        const float d1 = (t[0] / fin_n) / 3.f, d2 = (t[1] / fin_n) / 3.f;
        const float d3 = (t[2] / fin_n2) / 12.f, d4 = (t[3] / fin_n2) / 12.f;
        loss_out[0] = (2.f * (((d1 + d2) + d3) + d4)) * fin_weight;
    }
}
// sums[k] = fixed-order sum over the per-block partials (k = 0..width-1)
__global__ __launch_bounds__(64) void reduce_partials_kernel(const float* __restrict__ partials, int nparts,
                                                             int width, float* __restrict__ sums) {
    for (int k = 0; k < width; ++k) {
        float s = 0.f;
        for (int i = threadIdx.x; i < nparts; i += 64) s += partials[i * width + k];
        s = wave_sum(s);
        if (threadIdx.x == 0) sums[k] = s;
    }
}
__global__ void tv_from_sums_kernel(const float* __restrict__ s, float n, float n2, float weight,
                                    float* __restrict__ loss_out) {
#pragma clang fp contract(off)
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const float d1 = (s[0] / n) / 3.f, d2 = (s[1] / n) / 3.f;
        const float d3 = (s[2] / n2) / 12.f, d4 = (s[3] / n2) / 12.f;
        loss_out[0] = (2.f * (((d1 + d2) + d3) + d4)) * weight;
    }
}
__global__ void mse_from_sum_kernel(const float* __restrict__ s, float count, float weight,
                                    float* __restrict__ loss_out) {
#pragma clang fp contract(off)
    if (threadIdx.x == 0 && blockIdx.x == 0) loss_out[0] = (s[0] / count) * weight;
}
__global__ void div_by_scalar_kernel(const float* __restrict__ a, float d, float* __restrict__ y,
                                     long long count) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += (long long)gridDim.x * 256)
        y[i] = a[i] / d;
}
__global__ __launch_bounds__(64) void tv_final_kernel(const float* __restrict__ partials, int nparts, float n,
                                                      float n2, float weight, float* __restrict__ loss_out) {
#pragma clang fp contract(off)
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < nparts; i += 64)
        for (int k = 0; k < 4; ++k) s[k] += partials[i * 4 + k];
    for (int k = 0; k < 4; ++k) s[k] = wave_sum(s[k]);
    if (threadIdx.x == 0) {
        const float d1 = (s[0] / n) / 3.f, d2 = (s[1] / n) / 3.f;
        const float d3 = (s[2] / n2) / 12.f, d4 = (s[3] / n2) / 12.f;
        loss_out[0] = (2.f * (((d1 + d2) + d3) + d4)) * weight;
    }
}

// `copy` (optional): the caller's 8-float result buffer, written by the same launch (a separate 32-byte device copy
// was a 16 us kernel at the very end of every iteration's critical path)
__global__ void sum_losses_kernel(float* l, float* copy) {
#pragma clang fp contract(off)
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        float t = 0.f;
        for (int i = 0; i < 7; ++i) t = t + l[i];        // Python sum(): 0 + l0 + l1 + ... (SumLoss, :208)
        l[7] = t;
        if (copy) {
            for (int i = 0; i < 7; ++i) copy[i] = l[i];
            copy[7] = t;
        }
    }
}

// General closure (st_taps.hip): the weighted terms of a configured plan in SumLoss order (style_transfer.py:455) - n_content
// content terms, n_style style terms, tv - folded into the 8-float loss array: [0] the content terms' sum, [1] the style
// terms', [2..5] zero, [6] tv, [7] total.  The total is formed as sum_losses_kernel and AdamTail form it, 0 + l[0] + ... +
// l[6], so that a step whose tail sums the array again leaves the same bits.
__global__ void sum_terms_kernel(const float* __restrict__ terms, int n_content, int n_style, float* __restrict__ l,
                                 float* __restrict__ copy) {
#pragma clang fp contract(off)
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        float c = 0.f, st = 0.f;
        for (int i = 0; i < n_content; ++i) c = c + terms[i];
        for (int i = 0; i < n_style; ++i) st = st + terms[n_content + i];
        const float tv = terms[n_content + n_style];
        float t = 0.f;
        t = t + c;
        t = t + st;
        for (int i = 2; i < 6; ++i) t = t + 0.f;
        t = t + tv;
        for (int k = 0; k < (copy ? 2 : 1); ++k) {
            float* o = k ? copy : l;
            o[0] = c; o[1] = st; o[2] = 0.f; o[3] = 0.f; o[4] = 0.f; o[5] = 0.f; o[6] = tv; o[7] = t;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// torch.optim.Adam single-tensor step (torch/optim/adam.py:414-547, as configured at
// style_transfer.py:458) + image.clamp_(0, 1) (:485) + EMA.update (:250-253), one pass over 3HW.
__global__ __launch_bounds__(256) void adam_clamp_ema_kernel(float* __restrict__ image,
                                                             const float* __restrict__ grad,
                                                             float* __restrict__ exp_avg,
                                                             float* __restrict__ exp_avg_sq,
                                                             float* __restrict__ ema, long long count,
                                                             AdamScalars sc, AdamTail tail) {
#pragma clang fp contract(off)
    adam_tail(tail);
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
        const float g = grad[i];
        float m = exp_avg[i], v = exp_avg_sq[i], p = image[i], e = ema[i];
        adam_clamp_ema_element(g, m, v, p, e, sc);
        exp_avg[i] = m;
        exp_avg_sq[i] = v;
        image[i] = p;
        ema[i] = e;
    }
}

int grid_for(long long n, int cap = 4096) {
    long long b = (n + 255) / 256;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

}  // namespace

int launch_fill(float* p, long long n, float v, hipStream_t s) {
    hipLaunchKernelGGL(fill_kernel, dim3(grid_for(n)), dim3(256), 0, s, p, n, v);
    ST_LAUNCH_CHECK();
    return 0;
}
int launch_identity(float* p, int n, hipStream_t s) {
    hipLaunchKernelGGL(identity_kernel, dim3(grid_for((long long)n * n)), dim3(256), 0, s, p, n);
    ST_LAUNCH_CHECK();
    return 0;
}
int launch_cov_from_moments(const float* mean, const float* srm, float* cov, int n, float eps, hipStream_t s) {
    hipLaunchKernelGGL(cov_kernel, dim3(grid_for((long long)n * n)), dim3(256), 0, s, mean, srm, cov, n, eps);
    ST_LAUNCH_CHECK();
    return 0;
}
int launch_frobenius(const float* a, long long count, float* out, hipStream_t s) {
    // out[2..] doubles as the partial buffer: callers pass a scalar slot followed by >= 64 spare floats
    const int blocks = grid_for(count, 32);
    float* partials = out + 2;
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3(blocks), dim3(256), 0, s, a, count, partials);
    ST_LAUNCH_CHECK();
    hipLaunchKernelGGL(sqrt_of_sum_kernel, dim3(1), dim3(64), 0, s, partials, blocks, out);
    ST_LAUNCH_CHECK();
    return 0;
}
int launch_sumsq_partials(const float* a, long long count, float* partials, int* nparts, hipStream_t s) {
    const int blocks = grid_for(count / 4, 256);
    hipLaunchKernelGGL(sumsq_partial4_kernel, dim3(blocks), dim3(256), 0, s, a, count, partials);
    ST_LAUNCH_CHECK();
    *nparts = blocks;
    return 0;
}
int launch_ns_prepare(const float* a, int n, float* norm_out, float* partials, float* a_scaled, const float* g,
                      const float* gdiag, float* second, hipStream_t s, bool first_t, const W2LossJob* loss,
                      int partials_ready) {
    const long long nn = (long long)n * n;
    int blocks = partials_ready;              // (the product that made `a` left its tiles' sums of squares: no launch here)
    if (blocks <= 0 && launch_sumsq_partials(a, nn, partials, &blocks, s)) return 1;
    const int mode = first_t ? 3 : g ? 1 : (gdiag ? 2 : 0);
    ST_REQUIRE(!loss || mode == 2, "ns prepare: a W2 job needs the diagonal form");
    hipLaunchKernelGGL(ns_prepare_kernel, dim3(grid_for(nn, 1024)), dim3(256), 0, s, a, partials, blocks, norm_out,
                       a_scaled, g, gdiag, second, n, mode, loss ? *loss : W2LossJob{});
    ST_LAUNCH_CHECK();
    return 0;
}
int launch_div_by_dev_scalar(const float* a, const float* scalar, float* y, long long count, hipStream_t s) {
    hipLaunchKernelGGL(div_by_dev_scalar_kernel, dim3(grid_for(count)), dim3(256), 0, s, a, scalar, y, count);
    ST_LAUNCH_CHECK();
    return 0;
}
int launch_scaled_identity_div(const float* diag_value, const float* scalar, float* q, int n, hipStream_t s) {
    hipLaunchKernelGGL(scaled_identity_div_kernel, dim3(grid_for((long long)n * n)), dim3(256), 0, s,
                       diag_value, scalar, q, n);
    ST_LAUNCH_CHECK();
    return 0;
}

// streaming kernels with a two-level sum: up to kStreamBlocks workgroups (8 waves per SIMD chip-wide) of 256 threads
static int stream_blocks(long long work_items) { return grid_for(work_items, kStreamBlocks); }

// ST_LAST_BLOCK_FENCE=1: the partials' former hand-off (plain stores behind an agent-scope release fence), for A/B runs and
// tests/test_last_block_gpu.py; both flavours give the same bits
LastBlock last_block(unsigned int* ticket) {
    static Option fence_opt("ST_LAST_BLOCK_FENCE", 0);
    return LastBlock{ticket, ticket != nullptr && fence_opt.get() != 0 ? 1 : 0};
}

int launch_content_mse(const float* feat, const float* target, long long count, float weight, float* grad,
                       float* partials, float* loss_out, hipStream_t s, unsigned int* ticket, int accumulate) {
    const int blocks = stream_blocks((count & 3) == 0 ? count / 4 : count);
    const float norm = (float)(2.0 / (double)count);
    if (accumulate)
        hipLaunchKernelGGL(content_mse_kernel<true>, dim3(blocks), dim3(256), 0, s, feat, target, count, weight, norm,
                           grad, partials, last_block(ticket), (float)count, loss_out);
    else
        hipLaunchKernelGGL(content_mse_kernel<false>, dim3(blocks), dim3(256), 0, s, feat, target, count, weight, norm,
                           grad, partials, last_block(ticket), (float)count, loss_out);
    ST_LAUNCH_CHECK();
    if (ticket) return 0;                 // the last block wrote the loss
    hipLaunchKernelGGL(content_mse_final_kernel, dim3(1), dim3(64), 0, s, partials, blocks, (float)count,
                       weight, loss_out);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_scaled_mse_sums(const float* x, const float* target, long long count, float weight, float* partials, float* totals,
                           float* loss_out, hipStream_t s, unsigned int* ticket, float eps) {
    ST_REQUIRE(ticket, "scaled MSE sums: the last block finishes the sum, a ticket word is needed");
    const int blocks = stream_blocks((count & 3) == 0 ? count / 4 : count);
    hipLaunchKernelGGL(scaled_mse_sums_kernel, dim3(blocks), dim3(256), 0, s, x, target, count, weight, eps, partials,
                       last_block(ticket), totals, loss_out);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_scaled_mse_grad(const float* feat, const float* target, long long count, float weight, const float* totals,
                           float* grad, hipStream_t s, int accumulate) {
    const int blocks = stream_blocks((count & 3) == 0 ? count / 4 : count);
    if (accumulate)
        hipLaunchKernelGGL(scaled_mse_grad_kernel<true>, dim3(blocks), dim3(256), 0, s, feat, target, count, weight, totals, grad);
    else
        hipLaunchKernelGGL(scaled_mse_grad_kernel<false>, dim3(blocks), dim3(256), 0, s, feat, target, count, weight, totals, grad);
    ST_LAUNCH_CHECK();
    return 0;
}

// the content terms under a weight map (the kernels' comment has the formulas): wmap [npix], count = channels * npix
int launch_content_mse_weighted(const float* feat, const float* target, const float* wmap, long long count, long long npix,
                                float weight, float* grad, float* partials, float* loss_out, hipStream_t s, unsigned int* ticket,
                                int accumulate) {
    ST_REQUIRE(wmap && ticket && npix > 0 && count % npix == 0, "weighted content MSE: bad argument");
    const int blocks = stream_blocks((npix & 3) == 0 ? count / 4 : count);
    const float norm = (float)(2.0 / (double)count);
    if (accumulate)
        hipLaunchKernelGGL(content_mse_w_kernel<true>, dim3(blocks), dim3(256), 0, s, feat, target, wmap, count, npix, weight, norm,
                           grad, partials, last_block(ticket), (float)count, loss_out);
    else
        hipLaunchKernelGGL(content_mse_w_kernel<false>, dim3(blocks), dim3(256), 0, s, feat, target, wmap, count, npix, weight, norm,
                           grad, partials, last_block(ticket), (float)count, loss_out);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_scaled_mse_sums_weighted(const float* x, const float* target, const float* wmap, long long count, long long npix,
                                    float weight, float* partials, float* totals, float* loss_out, hipStream_t s,
                                    unsigned int* ticket, float eps) {
    ST_REQUIRE(wmap && ticket && npix > 0 && count % npix == 0, "weighted scaled MSE sums: bad argument");
    const int blocks = stream_blocks((npix & 3) == 0 ? count / 4 : count);
    hipLaunchKernelGGL(scaled_mse_sums_w_kernel, dim3(blocks), dim3(256), 0, s, x, target, wmap, count, npix, weight, eps, partials,
                       last_block(ticket), totals, loss_out);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_scaled_mse_grad_weighted(const float* feat, const float* target, const float* wmap, long long count, long long npix,
                                    float weight, const float* totals, float* grad, hipStream_t s, int accumulate) {
    ST_REQUIRE(wmap && npix > 0 && count % npix == 0, "weighted scaled MSE gradient: bad argument");
    const int blocks = stream_blocks((npix & 3) == 0 ? count / 4 : count);
    if (accumulate)
        hipLaunchKernelGGL(scaled_mse_grad_w_kernel<true>, dim3(blocks), dim3(256), 0, s, feat, target, wmap, count, npix, weight,
                           totals, grad);
    else
        hipLaunchKernelGGL(scaled_mse_grad_w_kernel<false>, dim3(blocks), dim3(256), 0, s, feat, target, wmap, count, npix, weight,
                           totals, grad);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_gram_grad_finish(const float* gram, const float* gram_t, const float* totals, int n, float weight, long long npix,
                            float* ssym, float* bvec, hipStream_t s, unsigned int* ssym_amax, float mask_sum) {
    hipLaunchKernelGGL(gram_grad_finish_kernel, dim3(n), dim3(256), 0, s, gram, gram_t, totals, n, weight,
                       mask_sum > 0.f ? mask_sum : (float)npix, ssym, bvec, ssym_amax);
    ST_LAUNCH_CHECK();
    return 0;
}

// HBM-bound (reads 4 - 12 bytes and writes 4 per element): the 16-byte groups when every pointer allows them, like the
// pool kernels' launcher; what is left of `count` behind them, or everything, goes one element at a time
int launch_seed_grad(const float* ext, const float* relu_out, float* g, long long count, int accumulate, unsigned int* bound,
                     hipStream_t s) {
    ST_REQUIRE(ext && g && count > 0, "seed gradient: null argument");
    const bool aligned = ((reinterpret_cast<uintptr_t>(ext) | reinterpret_cast<uintptr_t>(relu_out) |
                           reinterpret_cast<uintptr_t>(g)) & 15) == 0;
    const long long n4 = aligned ? count / 4 : 0;
    const int blocks = grid_for(std::max(n4, count - 4 * n4));
    if (accumulate) hipLaunchKernelGGL(seed_grad_kernel<true>, dim3(blocks), dim3(256), 0, s, ext, relu_out, g, count, n4, bound);
    else hipLaunchKernelGGL(seed_grad_kernel<false>, dim3(blocks), dim3(256), 0, s, ext, relu_out, g, count, n4, bound);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_style_loss_value(const float* mean, const float* mean_t, const float* cov, const float* cov_t,
                            const float* root, int n, float weight, float* loss_out, float* gdiag_out,
                            hipStream_t s) {
    hipLaunchKernelGGL(style_loss_value_kernel, dim3(1), dim3(256), 0, s,
                       W2LossJob{mean, mean_t, cov, cov_t, root, n, weight, loss_out, gdiag_out});
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_style_grad_finish(const float* g, const float* mean, const float* mean_t, int n, float weight,
                             long long npix, float* ssym, float* bvec, hipStream_t s, unsigned int* ssym_amax, float mask_sum) {
    hipLaunchKernelGGL(style_grad_finish_kernel, dim3(n), dim3(256), 0, s, g, mean, mean_t, n, weight,
                       mask_sum > 0.f ? mask_sum : (float)npix, ssym, bvec, ssym_amax);
    ST_LAUNCH_CHECK();
    return 0;
}

// diagnostic (ST_TV_VARIANT=3): per-thread accumulators of tv_interior_kernel, kStreamBlocks x 256 x 5 floats, allocated once
float* tv_debug_buffer() {
    static float* buf = nullptr;
    if (!buf && hipMalloc(reinterpret_cast<void**>(&buf), (size_t)kStreamBlocks * 256 * 5 * sizeof(float)) != hipSuccess) buf = nullptr;
    return buf;
}

// the two TV launches; returns the number of partial-sum blocks (4 floats each) in `partials`
// (wmap: a whole image's weight map - the weighted kernels; null: the kernels of the unweighted term, as ever)
static int launch_tv_kernels(const float* image, int height, int width, StripInfo strip, float k1, float k3, float* grad,
                             float* partials, LastBlock lb, float n, float n2, float weight, float* loss_out,
                             hipStream_t s, int* nparts, const float* wmap = nullptr) {
    // (width >= 8 and height >= 2: with a single 4-pixel group per row, or a single row, the border kernel's "first and
    // last group / row" coincide and it would visit - and sum - those pixels twice)
    const bool vec = (width & 3) == 0 && width >= 8 && height >= 2 && (((long long)height * width) & 3) == 0 &&
                     ((reinterpret_cast<uintptr_t>(image) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(wmap)) & 15) == 0;
    int first = 0;
    long long border_threads;
    if (vec) {
        const int gpr = width >> 2;
        int tpr = 256;
        while (tpr > 1 && (tpr >> 1) >= gpr) tpr >>= 1;
        const int rpb = 256 / tpr;
        first = std::min((3 * height + rpb - 1) / rpb, kStreamBlocks - 256);
        static Option variant("ST_TV_VARIANT", 1);              // 1: shipped; 0 / 3: the reproducer (see the kernel)
        float* none = nullptr;
        switch (wmap ? -1 : kExperiments ? variant.get() : 1) {
            case -1: hipLaunchKernelGGL(tv_interior_w_kernel, dim3(first), dim3(256), 0, s, image, wmap, height, width, k1, k3, grad, partials); break;
#if defined(ST_EXPERIMENTS)          // (the reproducer kernels exist only in builds with --experiments)
            case 0: hipLaunchKernelGGL(tv_interior_kernel<0>, dim3(first), dim3(256), 0, s, image, height, width, k1, k3, grad, partials, none); break;
            case 3: hipLaunchKernelGGL(tv_interior_kernel<3>, dim3(first), dim3(256), 0, s, image, height, width, k1, k3, grad, partials, tv_debug_buffer()); break;
#endif
            default: hipLaunchKernelGGL(tv_interior_kernel<1>, dim3(first), dim3(256), 0, s, image, height, width, k1, k3, grad, partials, none); break;
        }
        ST_LAUNCH_CHECK();
        border_threads = 3ll * (2 * gpr + 2 * (height - 2)) * 4;
    } else {
        border_threads = 3ll * height * width;
    }
    const int nb = (int)std::min<long long>((border_threads + 255) / 256, vec ? 256 : kStreamBlocks);
    if (wmap)
        hipLaunchKernelGGL(tv_border_w_kernel, dim3(nb), dim3(256), 0, s, image, wmap, height, width, k1, k3, grad, partials,
                           vec ? 1 : 0, first, lb, n, n2, weight, loss_out);
    else
        hipLaunchKernelGGL(tv_border_kernel, dim3(nb), dim3(256), 0, s, image, height, width, k1, k3, grad, partials, strip,
                           vec ? 1 : 0, first, lb, n, n2, weight, loss_out);
    ST_LAUNCH_CHECK();
    *nparts = first + nb;
    return 0;
}

int launch_tv(const float* image, int height, int width, float weight, float* grad, float* partials,
              float* loss_out, hipStream_t s, unsigned int* ticket, const float* wmap) {
    const double n = 3.0 * height * width, n2 = 3.0 * (height + 1) * (width + 1);
    // d loss / d D = weight * 2 * (1/3 or 1/12) * (1/n) * 2 D
    const float k1 = (float)(weight * 4.0 / (3.0 * n));
    const float k3 = (float)(weight * 4.0 / (12.0 * n2));
    StripInfo whole{0, height, 0, 0, nullptr};
    int nparts = 0;
    if (launch_tv_kernels(image, height, width, whole, k1, k3, grad, partials, last_block(ticket), (float)n, (float)n2,
                          weight, loss_out, s, &nparts, wmap))
        return 1;
    if (ticket) return 0;                 // the border kernel's last block wrote the loss
    hipLaunchKernelGGL(tv_final_kernel, dim3(1), dim3(64), 0, s, partials, nparts, (float)n, (float)n2, weight,
                       loss_out);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_tv_strip(const float* image, int height, int width, StripInfo strip, float weight, float* grad,
                    float* partials, float* sums4, hipStream_t s) {
    const double n = 3.0 * strip.global_height * width, n2 = 3.0 * (strip.global_height + 1) * (width + 1);
    const float k1 = (float)(weight * 4.0 / (3.0 * n));
    const float k3 = (float)(weight * 4.0 / (12.0 * n2));
    int nparts = 0;
    if (launch_tv_kernels(image, height, width, strip, k1, k3, grad, partials, last_block(nullptr), 0.f, 0.f, 0.f,
                          nullptr, s, &nparts))
        return 1;
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(64), 0, s, partials, nparts, 4, sums4);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_tv_final(const float* sums4, int global_height, int width, float weight, float* loss_out,
                    hipStream_t s) {
    const double n = 3.0 * global_height * width, n2 = 3.0 * (global_height + 1) * (width + 1);
    hipLaunchKernelGGL(tv_from_sums_kernel, dim3(1), dim3(64), 0, s, sums4, (float)n, (float)n2, weight, loss_out);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_content_mse_strip(const float* feat, const float* target, long long local_count,
                             long long global_count, float weight, float* grad, float* partials,
                             float* sum_out, hipStream_t s) {
    const int blocks = stream_blocks((local_count & 3) == 0 ? local_count / 4 : local_count);
    const float norm = (float)(2.0 / (double)global_count);
    hipLaunchKernelGGL(content_mse_kernel<false>, dim3(blocks), dim3(256), 0, s, feat, target, local_count, weight, norm,
                       grad, partials, last_block(nullptr), 0.f, static_cast<float*>(nullptr));
    ST_LAUNCH_CHECK();
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(64), 0, s, partials, blocks, 1, sum_out);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_content_mse_final(const float* sum, long long global_count, float weight, float* loss_out,
                             hipStream_t s) {
    hipLaunchKernelGGL(mse_from_sum_kernel, dim3(1), dim3(64), 0, s, sum, (float)global_count, weight, loss_out);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_div_by_scalar(const float* a, float d, float* y, long long count, hipStream_t s) {
    hipLaunchKernelGGL(div_by_scalar_kernel, dim3(grid_for(count)), dim3(256), 0, s, a, d, y, count);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_sum_losses(float* losses8, hipStream_t s, float* copy) {
    hipLaunchKernelGGL(sum_losses_kernel, dim3(1), dim3(64), 0, s, losses8, copy == losses8 ? nullptr : copy);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_sum_terms(const float* terms, int n_content, int n_style, float* losses8, hipStream_t s, float* copy) {
    hipLaunchKernelGGL(sum_terms_kernel, dim3(1), dim3(64), 0, s, terms, n_content, n_style, losses8, copy == losses8 ? nullptr : copy);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_adam_clamp_ema(float* image, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema,
                          long long count, AdamScalars sc, hipStream_t s, AdamTail tail) {
    if (tail.losses_copy == tail.losses8) tail.losses_copy = nullptr;
    hipLaunchKernelGGL(adam_clamp_ema_kernel, dim3(grid_for(count)), dim3(256), 0, s, image, grad, exp_avg,
                       exp_avg_sq, ema, count, sc, tail);
    ST_LAUNCH_CHECK();
    return 0;
}

}  // namespace st
