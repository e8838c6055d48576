// Laplacian loss on average-pooled images (Li et al., "Laplacian-Steered Neural Style Transfer"; semantics: include/st_amd.h).
// Per pool size p, with Q = avg_pool2d(x, p) at floor sizes h = H / p, w = W / p and L the 4-neighbour Laplacian on the
// replicate-padded map,
//   term_p = weight sum((L(Q(x)) - T_p)^2) / (C h w),   T_p = L(Q(content)),
//   d term_p / d x[c][y][x] = (2 weight / (C h w p^2)) (L^T r)[c][y / p][x / p]   for y < h p and x < w p, 0 elsewhere.
// Three memory-bound launches per pool size, all on the caller's stream:
//   lap_pool_kernel      Q from the image (skipped for p = 1, where Q is the image); a window is summed row-major.
//   lap_residual_kernel  r = L(Q) - T and the per-block sums of r^2; the last block (ticket) adds them in index order, writes
//                        term_p to its own word and adds it onto the image-space slot - one thread, stream-ordered behind the
//                        TV launch that wrote the slot.  T == nullptr: writes L(Q) and nothing else - the target pass, so an
//                        iterate equal to the content image has a residual of exactly 0.
//   lap_grad_kernel      every image pixel gathers (L^T r) of its window from the small, L2-resident r and adds k times it onto
//                        the gradient the TV launch wrote (ACC) or writes it (the standalone backward).  Where W % 4 == 0 a
//                        thread owns 16-byte groups of a row; each element has one owner, so there are no atomics and two
//                        closures give equal bits.
// L^T: row b of L holds -1 at b's four CLAMPED neighbours, so column a collects -r[b] from every b that names a - its real
// neighbours and, once per side on which a lies at the border, a itself.  That is 4 r[a] minus r at a's clamped neighbours: with
// replicate padding the operator is symmetric, and lap_transpose is written as the fold.
#include <algorithm>
#include <cmath>

#include "st_plan.h"

namespace st {

namespace {

// (L Q)[i][j] on one channel [h][w], neighbour indices clamped to the map; the subtractions in a fixed order
__device__ __forceinline__ float lap_at(const float* __restrict__ q, int h, int w, int i, int j) {
#pragma clang fp contract(off)
    const float c = q[(size_t)i * w + j];
    const float up = q[(size_t)max(i - 1, 0) * w + j], dn = q[(size_t)min(i + 1, h - 1) * w + j];
    const float lf = q[(size_t)i * w + max(j - 1, 0)], rt = q[(size_t)i * w + min(j + 1, w - 1)];
    return (((4.f * c - up) - dn) - lf) - rt;
}

// (L^T r)[i][j]: the real neighbours' rows of L name (i, j) once each; at a border (i, j)'s own row names it once more
__device__ __forceinline__ float lap_transpose(const float* __restrict__ r, int h, int w, int i, int j) {
#pragma clang fp contract(off)
    const float c = r[(size_t)i * w + j];
    const float up = i >= 1 ? r[(size_t)(i - 1) * w + j] : c, dn = i + 1 < h ? r[(size_t)(i + 1) * w + j] : c;
    const float lf = j >= 1 ? r[(size_t)i * w + j - 1] : c, rt = j + 1 < w ? r[(size_t)i * w + j + 1] : c;
    return (((4.f * c - up) - dn) - lf) - rt;
}

// Q[c][i][j] = mean of the p x p window, rows and columns behind h p / w p dropped.  VEC: p % 4 == 0, W % 4 == 0 and a 16-byte
// aligned image - a window row is p / 4 aligned groups, added in the same row-major order.
template <bool VEC>
__global__ __launch_bounds__(256) void lap_pool_kernel(const float* __restrict__ image, int C, int H, int W, int p, int h, int w,
                                                       float window, float* __restrict__ Q) {
#pragma clang fp contract(off)
    const int total = C * h * w;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int j = idx % w, t = idx / w;
        const int i = t % h, ch = t / h;
        const float* src = image + ((size_t)ch * H + (size_t)i * p) * W + (size_t)j * p;
        float s = 0.f;
        for (int dy = 0; dy < p; ++dy) {
            const float* row = src + (size_t)dy * W;
            if (VEC) {
                for (int dx = 0; dx < p; dx += 4) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(row + dx);
                    s += v[0];
                    s += v[1];
                    s += v[2];
                    s += v[3];
                }
            } else {
                for (int dx = 0; dx < p; ++dx) s += row[dx];
            }
        }
        Q[idx] = s / window;
    }
}

// target == nullptr: out = L(Q), nothing else.  Otherwise out = r = L(Q) - target, partials[block] = the block's sum of r^2, and
// the last block: term_out[0] = weight (sum / count); tv_out (the first pool size): the slot as the TV launch left it;
// slot (a plan): += the term.
__global__ __launch_bounds__(256) void lap_residual_kernel(const float* __restrict__ Q, const float* __restrict__ target, int C,
                                                           int h, int w, float* __restrict__ out, float* __restrict__ partials,
                                                           LastBlock lb, float count, float weight, float* __restrict__ term_out,
                                                           float* __restrict__ tv_out, float* __restrict__ slot) {
#pragma clang fp contract(off)
    __shared__ float scratch[4];
    __shared__ bool is_last;
    const int total = C * h * w;
    float s = 0.f;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int j = idx % w, t = idx / w;
        const int i = t % h;
        const float l = lap_at(Q + (size_t)(t - i) * w, h, w, i, j);
        if (target == nullptr) {
            out[idx] = l;
        } else {
            const float r = l - target[idx];
            out[idx] = r;
            s += r * r;
        }
    }
    if (target == nullptr) return;
    s = block_sum_256(s, scratch);
    const float mine[1] = {s};
    if (!last_block_arrives(lb, &is_last, partials + blockIdx.x, mine)) return;
    float t = 0.f;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) t += partials[i];
    t = block_sum_256(t, scratch);
    if (threadIdx.x == 0) {
        const float term = (t / count) * weight;
        term_out[0] = term;
        if (tv_out) tv_out[0] = slot[0];
        if (slot) slot[0] = slot[0] + term;
    }
}

// the two-launch form's second launch (the standalone value, which has no zeroed ticket word): the last block's sum
__global__ __launch_bounds__(256) void lap_final_kernel(const float* __restrict__ partials, int nparts, float count, float weight,
                                                        float* __restrict__ term_out) {
#pragma clang fp contract(off)
    __shared__ float scratch[4];
    float t = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) t += partials[i];
    t = block_sum_256(t, scratch);
    if (threadIdx.x == 0) term_out[0] = (t / count) * weight;
}

// grad[c][y][x] (+)= k (L^T r)[c][y / p][x / p] inside the pooled region.  ACC: added onto what grad holds, pixels outside the
// region untouched; else written, zeros outside.  upstream: a device scalar that multiplies k (autograd's grad_output).
// VEC: W % 4 == 0 and a 16-byte aligned grad - a thread owns groups of 4 pixels of a row and walks the window index along them.
template <bool ACC, bool VEC>
__global__ __launch_bounds__(256) void lap_grad_kernel(const float* __restrict__ r, int C, int H, int W, int p, int h, int w,
                                                       float k, const float* __restrict__ upstream, float* __restrict__ grad) {
#pragma clang fp contract(off)
    const float kk = upstream ? upstream[0] * k : k;
    const int yend = h * p, xend = w * p;
    if (VEC) {
        const int gpr = W >> 2;
        const int total = C * H * gpr;
        for (int gi = blockIdx.x * 256 + threadIdx.x; gi < total; gi += gridDim.x * 256) {
            const int g4 = gi % gpr, row = gi / gpr;
            const int y = row % H, ch = row / H;
            const int x0 = 4 * g4;
            f32x4* dst = reinterpret_cast<f32x4*>(grad + (size_t)row * W + x0);
            const bool inside = y < yend && x0 < xend;
            if (ACC && !inside) continue;
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
            if (inside) {
                if (ACC) o = *dst;
                const float* rc = r + (size_t)ch * h * w;
                const int i = y / p;
                int j = x0 / p, rem = x0 - j * p;
                float t = lap_transpose(rc, h, w, i, j);         // (x0 < xend: j < w)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (rem == p) {
                        rem = 0;
                        ++j;
                        if (j < w) t = lap_transpose(rc, h, w, i, j);
                    }
                    if (j < w) o[e] = o[e] + kk * t;
                    ++rem;
                }
            }
            *dst = o;
        }
    } else {
        const int total = C * H * W;
        for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
            const int x = idx % W, row = idx / W;
            const int y = row % H, ch = row / H;
            const bool inside = y < yend && x < xend;
            if (ACC && !inside) continue;
            float o = 0.f;
            if (inside) {
                if (ACC) o = grad[idx];
                o = o + kk * lap_transpose(r + (size_t)ch * h * w, h, w, y / p, x / p);
            }
            grad[idx] = o;
        }
    }
}

bool aligned16(const void* a) { return (reinterpret_cast<uintptr_t>(a) & 15) == 0; }
int lap_grid(long long items) {
    const long long want = (items + 255) / 256;
    return (int)(want < 1 ? 1 : (want > kLapBlocks ? kLapBlocks : want));
}

}  // namespace

int launch_lap_pool(const float* image, int C, int H, int W, int p, float* Q, hipStream_t s) {
    const int h = H / p, w = W / p;
    const int blocks = lap_grid((long long)C * h * w);
    const float window = (float)((long long)p * p);
    if (p % 4 == 0 && W % 4 == 0 && aligned16(image))
        hipLaunchKernelGGL(lap_pool_kernel<true>, dim3(blocks), dim3(256), 0, s, image, C, H, W, p, h, w, window, Q);
    else
        hipLaunchKernelGGL(lap_pool_kernel<false>, dim3(blocks), dim3(256), 0, s, image, C, H, W, p, h, w, window, Q);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_lap_residual(const float* Q, const float* target, int C, int h, int w, float weight, float* out, float* partials,
                        unsigned int* ticket, float* term_out, float* tv_out, float* slot, hipStream_t s) {
    const int blocks = lap_grid((long long)C * h * w);
    const float count = (float)((double)C * h * w);
    hipLaunchKernelGGL(lap_residual_kernel, dim3(blocks), dim3(256), 0, s, Q, target, C, h, w, out, partials, last_block(ticket),
                       count, weight, term_out, tv_out, slot);
    ST_LAUNCH_CHECK();
    if (target && !ticket) {
        hipLaunchKernelGGL(lap_final_kernel, dim3(1), dim3(256), 0, s, partials, blocks, count, weight, term_out);
        ST_LAUNCH_CHECK();
    }
    return 0;
}

int launch_lap_grad(const float* r, int C, int H, int W, int p, float weight, const float* upstream, float* grad, int accumulate,
                    hipStream_t s) {
    const int h = H / p, w = W / p;
    const float k = (float)(2.0 * (double)weight / ((double)C * h * w * (double)p * p));
    const bool vec = W % 4 == 0 && aligned16(grad);
    const int blocks = std::min(2 * kLapBlocks, std::max(1, (int)(((long long)C * H * (vec ? W / 4 : W) + 255) / 256)));
    if (vec) {
        if (accumulate) hipLaunchKernelGGL((lap_grad_kernel<true, true>), dim3(blocks), dim3(256), 0, s, r, C, H, W, p, h, w, k, upstream, grad);
        else hipLaunchKernelGGL((lap_grad_kernel<false, true>), dim3(blocks), dim3(256), 0, s, r, C, H, W, p, h, w, k, upstream, grad);
    } else {
        if (accumulate) hipLaunchKernelGGL((lap_grad_kernel<true, false>), dim3(blocks), dim3(256), 0, s, r, C, H, W, p, h, w, k, upstream, grad);
        else hipLaunchKernelGGL((lap_grad_kernel<false, false>), dim3(blocks), dim3(256), 0, s, r, C, H, W, p, h, w, k, upstream, grad);
    }
    ST_LAUNCH_CHECK();
    return 0;
}

namespace {

// what pool size k's Laplacian is taken of: the plan's pooled map, or the image itself for p = 1
const float* lap_pooled(st_plan* p, int k, const float* image) { return p->lap_pool[k] == 1 ? image : p->lap_q[k]; }

}  // namespace

int laplacian_terms(st_plan* p, const float* image, float* grad, float* slot, hipStream_t s) {
    const double image_bytes = 3.0 * 4.0 * p->H * p->W;
    for (int k = 0; k < p->n_lap; ++k) {
        const int pool = p->lap_pool[k], h = p->lap_h[k], w = p->lap_w[k];
        const double map_bytes = 3.0 * 4.0 * h * w;
        if (pool > 1 && hbm_profiled(p, HBM_TV, image_bytes + map_bytes, s, [&] {
                return launch_lap_pool(image, 3, p->H, p->W, pool, p->lap_q[k], s);
            }))
            return 1;
        if (hbm_profiled(p, HBM_TV, 3.0 * map_bytes, s, [&] {
                return launch_lap_residual(lap_pooled(p, k, image), p->lap_t[k], 3, h, w, p->lap_weight, p->lap_r[k], p->lap_partials,
                                           p->tickets + 192, p->lap_terms + 1 + k, k == 0 ? p->lap_terms : nullptr, slot, s);
            }) ||
            hbm_profiled(p, HBM_TV, 2.0 * image_bytes + map_bytes, s, [&] {
                return launch_lap_grad(p->lap_r[k], 3, p->H, p->W, pool, p->lap_weight, nullptr, grad, 1, s);
            }))
            return 1;
    }
    return 0;
}

}  // namespace st

using namespace st;

extern "C" {

int st_plan_set_laplacian(st_plan* p, const float* content_image, int n_pools, const int* pools, float weight, void* stream) {
    ST_REQUIRE(p, "st_plan_set_laplacian: null plan");
    ST_REQUIRE(!p->strip, "st_plan_set_laplacian: strip plans take no Laplacian term (the general closure serves it, on one device)");
    // no Laplacian is in force until this call has accepted one and built its targets
    if (p->n_lap || content_image) invalidate_graph(p);
    p->n_lap = 0;
    if (!content_image) return 0;
    ST_REQUIRE(n_pools >= 1 && n_pools <= kMaxLapPools, "st_plan_set_laplacian: %d pool sizes: a Laplacian takes 1 to %d", n_pools,
               kMaxLapPools);
    ST_REQUIRE(pools, "st_plan_set_laplacian: null list of pool sizes");
    for (int k = 0; k < n_pools; ++k) {
        ST_REQUIRE(pools[k] >= 1, "st_plan_set_laplacian: pool size %d (entry %d) is not positive", pools[k], k);
        for (int m = 0; m < k; ++m)
            ST_REQUIRE(pools[m] != pools[k], "st_plan_set_laplacian: pool size %d is repeated (entries %d and %d)", pools[k], m, k);
        ST_REQUIRE(p->H / pools[k] >= 2 && p->W / pools[k] >= 2,
                   "st_plan_set_laplacian: pool size %d leaves a %d x %d map of the %d x %d image: the pooled map must be at least "
                   "2 x 2 (on a 1-wide map the clamped Laplacian vanishes)", pools[k], p->H / pools[k], p->W / pools[k], p->H, p->W);
    }
    ST_REQUIRE(std::isfinite(weight) && weight > 0.f, "st_plan_set_laplacian: weight %g: the weight must be finite and > 0", (double)weight);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((!p->lap_partials && plan_alloc(p, &p->lap_partials, kLapBlocks)) || (!p->lap_terms && plan_alloc(p, &p->lap_terms, 64))) return 1;
    for (int k = 0; k < n_pools; ++k) {
        const int h = p->H / pools[k], w = p->W / pools[k];
        const size_t floats = (size_t)3 * h * w;
        if (floats > p->lap_floats[k]) {           // (a smaller set stays the plan's until it is destroyed)
            p->lap_floats[k] = 0;
            if (plan_alloc(p, &p->lap_q[k], floats) || plan_alloc(p, &p->lap_r[k], floats) || plan_alloc(p, &p->lap_t[k], floats)) return 1;
            p->lap_floats[k] = floats;
        }
        p->lap_pool[k] = pools[k];
        p->lap_h[k] = h;
        p->lap_w[k] = w;
        // the target with the closure's own kernels: T = L(Q(content))
        if (pools[k] > 1 && launch_lap_pool(content_image, 3, p->H, p->W, pools[k], p->lap_q[k], s)) return 1;
        if (launch_lap_residual(pools[k] == 1 ? content_image : p->lap_q[k], nullptr, 3, h, w, 0.f, p->lap_t[k], nullptr, nullptr,
                                nullptr, nullptr, nullptr, s))
            return 1;
    }
    ST_HIP(hipMemsetAsync(p->lap_terms, 0, 64 * sizeof(float), s));
    ST_HIP(hipStreamSynchronize(s));
    p->lap_weight = weight;
    p->n_lap = n_pools;
    return 0;
}

int st_plan_laplacian(const st_plan* p, int k, const float** target, int* h, int* w) {
    ST_REQUIRE(p, "st_plan_laplacian: null plan");
    ST_REQUIRE(p->n_lap > 0, "st_plan_laplacian: no Laplacian is set on this plan (st_plan_set_laplacian)");
    ST_REQUIRE(k >= 0 && k < p->n_lap, "st_plan_laplacian: pool size %d out of range (0 .. %d)", k, p->n_lap - 1);
    if (target) *target = p->lap_t[k];
    if (h) *h = p->lap_h[k];
    if (w) *w = p->lap_w[k];
    return 0;
}

int st_plan_laplacian_terms(st_plan* p, float** terms, int* count) {
    ST_REQUIRE(p && terms && count, "st_plan_laplacian_terms: null argument");
    ST_REQUIRE(p->n_lap > 0, "st_plan_laplacian_terms: no Laplacian is set on this plan (st_plan_set_laplacian)");
    *terms = p->lap_terms;
    *count = 1 + p->n_lap;
    return 0;
}

namespace {
int lap_op_shape(const char* who, int channels, int height, int width, int pool) {
    ST_REQUIRE(channels >= 1 && height >= 1 && width >= 1, "%s: bad shape %d x %d x %d", who, channels, height, width);
    ST_REQUIRE_PIXELS(who, (long long)height * width);
    // (the kernels count C * H * W elements in an `int`)
    ST_REQUIRE((long long)channels * height * width < (1ll << 31), "%s: %d x %d x %d: fewer than 2^31 elements", who, channels, height, width);
    ST_REQUIRE(pool >= 1 && height / pool >= 2 && width / pool >= 2,
               "%s: pool size %d on a %d x %d image: it must be >= 1 and leave a pooled map of at least 2 x 2", who, pool, height, width);
    return 0;
}
}  // namespace

long long st_op_laplacian_scratch_floats(int channels, int height, int width, int pool) {
    if (channels < 1 || height < 1 || width < 1 || pool < 1) return 0;
    return (long long)channels * (height / pool) * (width / pool) + kLapBlocks;
}

int st_op_laplacian_target(const float* image, int channels, int height, int width, int pool, float* scratch, float* target_out,
                           void* stream) {
    ST_REQUIRE(image && scratch && target_out, "st_op_laplacian_target: null argument");
    if (lap_op_shape("st_op_laplacian_target", channels, height, width, pool)) return 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (pool > 1 && launch_lap_pool(image, channels, height, width, pool, scratch, s)) return 1;
    return launch_lap_residual(pool == 1 ? image : scratch, nullptr, channels, height / pool, width / pool, 0.f, target_out, nullptr,
                               nullptr, nullptr, nullptr, nullptr, s);
}

int st_op_laplacian_value(const float* image, const float* target, int channels, int height, int width, int pool, float* scratch,
                          float* residual_out, float* loss_out, void* stream) {
    ST_REQUIRE(image && target && scratch && residual_out && loss_out, "st_op_laplacian_value: null argument");
    if (lap_op_shape("st_op_laplacian_value", channels, height, width, pool)) return 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int h = height / pool, w = width / pool;
    if (pool > 1 && launch_lap_pool(image, channels, height, width, pool, scratch, s)) return 1;
    return launch_lap_residual(pool == 1 ? image : scratch, target, channels, h, w, 1.f, residual_out, scratch + (size_t)channels * h * w,
                               nullptr, loss_out, nullptr, nullptr, s);
}

int st_op_laplacian_backward(const float* residual, int channels, int height, int width, int pool, const float* upstream, float* grad,
                             void* stream) {
    ST_REQUIRE(residual && upstream && grad, "st_op_laplacian_backward: null argument");
    if (lap_op_shape("st_op_laplacian_backward", channels, height, width, pool)) return 1;
    return launch_lap_grad(residual, channels, height, width, pool, 1.f, upstream, grad, 0, static_cast<hipStream_t>(stream));
}

}  // extern "C"
