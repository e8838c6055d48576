// Internal to libst_amd.so: ONE style head's host sequence - its moments, the W2 body around the Newton-Schulz chains, the Gram
// body, the 1x1 step, its memory - for the plan's closures (through the plan's wrappers, st_closure.hip and st_taps.hip) and the
// standalone loss modules (st_head.hip) alike.  Nothing here knows of st_plan, Node, streams by index, timeline events or profiling
// brackets.  The shallow heads in lockstep (style_heads_shallow_lockstep) batch differently, on one_gemm, w2_loss_job and the wrappers.
#pragma once

#include <algorithm>

#include "st_common.h"

namespace st {

// The work of one head: what a plan keeps per trunk position (st_plan::head) and a standalone head (st_head) per module.
struct StyleHead {
    int n = 0;            // channels
    long long npix = 0;        // GLOBAL pixel count of the tap (normalisation of the moments)
    long long npix_local = 0;  // pixels held here (== npix unless the plan is strip-sharded)
    unsigned int* s_amax = nullptr;   // fp16x3: bound on max |ssym| of this pass (a plan's: one of plan->amax_word's bounds)
    bool target_set = false;
    bool joined_in_build = false;    // phase construction: this head's broadcast + gradient step have been placed
    // targets (plans; a standalone head is handed its module's with every call)
    float *mean_t = nullptr, *cov_t = nullptr, *root_t = nullptr;
    // per-iteration
    float *mean = nullptr, *srm = nullptr, *cov = nullptr, *tmat = nullptr, *mmat = nullptr, *root = nullptr,
          *gm = nullptr, *dt = nullptr, *dcov = nullptr, *ssym = nullptr, *bvec = nullptr, *gdiag = nullptr;
    float* conv_scratch = nullptr;     // split-K workspace of the head's 1x1 gradient conv (small taps only)
    float* gram_t = nullptr;           // Gram kind (st_plan::style_kind[j] == 1): the target Gram matrix [n][n]
    NSWorkspace ns{};
    GramWorkspace gram{};
    bool allocated = false;            // plans: alloc_head_moments has run ...
    bool w2_allocated = false;         // ... and alloc_head_w2, with the targets' buffers
    // a W2 entry whose covariances are diagonal (st_plan_set_w2_diagonal): all it reads - the target (mu_t, sigma_t), the stats
    // launch's scratch (ticket, partials) and the gradient's coefficients [a | b]; none of the buffers above
    float *diag_mean_t = nullptr, *diag_std_t = nullptr, *diag_scratch = nullptr, *diag_coeffs = nullptr;
    // a W2 entry matched on its exact per-channel marginals (st_plan_set_w2_marginal): the target's quantile functions [n][npix]
    // and the sort's scratch (ticket, partials, two buffers of keys: marginal_scratch_bytes); none of the buffers above
    float *marg_t = nullptr, *marg_scratch = nullptr;
    // a W2 entry matched on nearest style vectors (st_plan_set_style_nearest): the prepared style set (bound, bias, S^T for near_m
    // vectors), the search's scratch and the last closure's matches [npix]; near_prep_floats / near_scratch_floats: what the two
    // buffers hold
    float *near_prep = nullptr, *near_scratch = nullptr;
    int* near_idx = nullptr;
    long long near_m = 0;
    size_t near_prep_floats = 0, near_scratch_floats = 0;
    // a W2 entry matched on sliced projections (st_plan_set_style_sliced): the directions R [P][C] and R^T [C][P] (buffers for
    // P = 512) of epoch sl_epoch, the target T [P][npix], the style images' feature vectors side by side in image order
    // (sl_feats: image i is [n][sl_m[i]], blend weight sl_a[i]), the bound words (R's, 1 by construction, then one per image,
    // measured once by the setter) and the call's scratch (sliced_scratch_bytes: Y, G, the sort's keys, partials and ticket)
    float *sl_r = nullptr, *sl_rt = nullptr, *sl_t = nullptr, *sl_feats = nullptr, *sl_bounds = nullptr, *sl_scratch = nullptr;
    int sl_images = 0;
    long long sl_m[kSlicedMaxImages] = {};
    float sl_a[kSlicedMaxImages] = {};
    long long sl_rows = 0;              // the longest row the scratch was sized for: max(npix, max sl_m)
    unsigned long long sl_epoch = 0;
    size_t sl_t_floats = 0, sl_feats_floats = 0, sl_scratch_floats = 0;
};

// what a sliced head needs for P projections and style images of `total` feature vectors in all, the longest row (the tap's
// pixels or an image's vectors) `rows`.  R, R^T and the bound words are allocated once; T, the vectors and the scratch grow when
// asked for more than they hold, and an outgrown buffer stays the allocator's until the plan is destroyed, as a nearest head's.
// R's bound word holds 1.0f; the ticket in front of the sort's scratch is zeroed; both on the null stream, which the caller
// synchronises
template <class Alloc>
int alloc_head_sliced(StyleHead& h, int proj, long long total, long long rows, Alloc&& alloc) {
    if (alloc(&h.sl_r, (size_t)512 * h.n) || alloc(&h.sl_rt, (size_t)512 * h.n)) return 1;
    if (!h.sl_bounds) {
        if (alloc(&h.sl_bounds, (size_t)(1 + kSlicedMaxImages) * kAmaxWordUints)) return 1;
        ST_HIP(hipMemset(h.sl_bounds, 0, (size_t)(1 + kSlicedMaxImages) * kAmaxWordUints * sizeof(float)));
        const float one = 1.f;
        ST_HIP(hipMemcpy(h.sl_bounds, &one, sizeof(float), hipMemcpyHostToDevice));
    }
    const size_t t = (size_t)proj * (size_t)h.npix_local, feats = (size_t)h.n * (size_t)total;
    const size_t scratch = (size_t)(sliced_scratch_bytes(proj, rows) / 4);
    if (t > h.sl_t_floats) {
        h.sl_t = nullptr;
        h.sl_t_floats = 0;
        if (alloc(&h.sl_t, t)) return 1;
        h.sl_t_floats = t;
    }
    if (feats > h.sl_feats_floats) {
        h.sl_feats = nullptr;
        h.sl_feats_floats = 0;
        if (alloc(&h.sl_feats, feats)) return 1;
        h.sl_feats_floats = feats;
    }
    if (scratch > h.sl_scratch_floats) {
        h.sl_scratch = nullptr;
        h.sl_scratch_floats = 0;
        if (alloc(&h.sl_scratch, scratch)) return 1;
        h.sl_scratch_floats = scratch;
    }
    // (the layout of the scratch depends on (P, rows): the ticket's place is zeroed for this one)
    ST_HIP(hipMemset(sliced_scratch_of(h.sl_scratch, proj, rows).sort, 0, 16));
    return 0;
}

// what a nearest head needs for m style vectors.  Each buffer is sized by its own function of (C, N, m) and grows when that
// function asks for more than it holds - the split count, hence the scratch, is not monotone in m.  A buffer that is outgrown
// stays the allocator's until the plan is destroyed (plans free nothing before that), so a style set that keeps growing
// accumulates dead device memory; one that shrinks or repeats allocates nothing.  The ticket in front of the scratch is zeroed on
// the null stream, which the caller synchronises.  metric != 0 (st_plan_set_nearest_metric): the prepared buffer also holds the
// centre, and both buffers are sized by the cosine entries' functions
template <class Alloc>
int alloc_head_nearest(StyleHead& h, long long m, Alloc&& alloc, int metric = 0) {
    if (!h.near_idx) {
        float* idx = nullptr;
        if (alloc(&idx, (size_t)h.npix_local)) return 1;
        h.near_idx = reinterpret_cast<int*>(idx);
    }
    const size_t prep = (size_t)(metric ? nearest_cosine_prepared_floats(h.n, m) : nearest_prepared_floats(h.n, m));
    const size_t scratch = (size_t)(metric ? nearest_cosine_scratch_floats(h.n, h.npix_local, m) : nearest_scratch_floats(h.n, h.npix_local, m));
    if (prep > h.near_prep_floats) {
        h.near_prep = nullptr;
        h.near_prep_floats = 0;
        if (alloc(&h.near_prep, prep)) return 1;
        h.near_prep_floats = prep;
    }
    if (scratch > h.near_scratch_floats) {
        h.near_scratch = nullptr;
        h.near_scratch_floats = 0;
        if (alloc(&h.near_scratch, scratch)) return 1;
        ST_HIP(hipMemset(h.near_scratch, 0, 16));
        h.near_scratch_floats = scratch;
    }
    return 0;
}

// what a marginal head needs; the ticket in front of its scratch is zeroed on the null stream, which the caller synchronises
template <class Alloc>
int alloc_head_marginal(StyleHead& h, Alloc&& alloc) {
    if (alloc(&h.marg_t, (size_t)h.n * (size_t)h.npix_local)) return 1;
    if (h.marg_scratch) return 0;
    if (alloc(&h.marg_scratch, (size_t)(marginal_scratch_bytes(h.n, h.npix_local) / 4))) return 1;
    ST_HIP(hipMemset(h.marg_scratch, 0, 16));
    return 0;
}

// what a diagonal head needs (alloc_head_diag); the ticket in front of its scratch is zeroed on the null stream, which the caller
// synchronises
template <class Alloc>
int alloc_head_diag(StyleHead& h, Alloc&& alloc) {
    if (alloc(&h.diag_mean_t, (size_t)h.n) || alloc(&h.diag_std_t, (size_t)h.n) || alloc(&h.diag_coeffs, 2 * (size_t)h.n)) return 1;
    if (h.diag_scratch) return 0;
    if (alloc(&h.diag_scratch, (size_t)channel_stats_scratch_floats(h.n, h.npix_local))) return 1;
    ST_HIP(hipMemset(h.diag_scratch, 0, 4 * sizeof(float)));
    return 0;
}
// The diagonal head on feat [n][npix]: the stats launch with the term and the coefficients, then dF written to (accumulate: added
// onto) grad.  mask_sum > 0 with sqrt_mask: the weighted moments and their normaliser.
inline int diag_head_run(const StyleHead& h, const float* feat, float weight, float eps, const float* sqrt_mask, float mask_sum,
                         float* loss_out, float* grad, int accumulate, hipStream_t s) {
    ChannelStatsFinish fin;
    fin.mean_t = h.diag_mean_t;
    fin.std_t = h.diag_std_t;
    fin.eps = eps;
    fin.weight = weight;
    fin.norm = sqrt_mask ? (double)mask_sum : (double)h.npix;
    fin.coeffs = h.diag_coeffs;
    fin.loss_out = loss_out;
    if (launch_channel_stats(feat, sqrt_mask, h.n, h.npix_local, h.diag_scratch, fin, s)) return 1;
    return launch_channel_affine_grad(feat, sqrt_mask, h.diag_coeffs, nullptr, h.n, h.npix_local, grad, accumulate, s);
}

// The moments of a tap: max |feat| (optional), the Gram partials, finalize
struct HeadMoments {
    const float* feat = nullptr;        // [n][npix_local]
    float *mean = nullptr, *srm = nullptr, *cov = nullptr;      // cov, optional: srm - mean mean^T + eps I from the same pass
    float eps = 0.f;
    unsigned int* bound = nullptr;      // fp16x3 arithmetic scaled by this bound on max |feat| (null: the exact fp32 pipe) ...
    bool measure_bound = false;         // ... which is cleared and measured here first (a tensor no trunk kernel wrote)
    const float* sqrt_mask = nullptr;   // a style mask: its square root at the tap's level ...
    float mask_sum = 0.f;               // ... and that level's sum, the normaliser then
    int given_splits = 0;               // > 0: that many partials are there already (conv1_1's fused launch left them)
    long long norm = 0;                 // in the place of h.npix (1: raw sums)
};
inline int head_moments(const StyleHead& h, const HeadMoments& m, hipStream_t s) {
    if (m.measure_bound) {
        ST_HIP(hipMemsetAsync(m.bound, 0, kAmaxWordUints * sizeof(unsigned int), s));
        if (launch_amax(m.feat, (long long)h.n * h.npix_local, m.bound, 0, s)) return 1;
    }
    const int splits = m.given_splits > 0 ? m.given_splits : gram_choose_splits(h.n, h.npix_local, h.gram.max_splits);
    if (m.given_splits <= 0 && launch_gram_partial(m.feat, h.n, h.npix_local, splits, h.gram, s, m.bound, m.sqrt_mask)) return 1;
    return launch_gram_finalize(h.gram, h.n, m.norm ? m.norm : h.npix, splits, m.mean, m.srm, s, m.cov, m.eps, m.mask_sum);
}

inline GemmBatch one_gemm(int n, const float* a, const float* b, float* d, int ta, int tb) {
    GemmBatch g{};
    g.n = n; g.count = 1;
    g.p[0].a1 = a; g.p[0].b1 = b; g.p[0].d = d; g.p[0].ta1 = ta; g.p[0].tb1 = tb;
    g.p[0].epilogue = EPI_SCALE; g.p[0].c = 1.f;
    return g;
}
// The W2 body around the caller's Newton-Schulz chains, A = root_t.  Opening: sqrt_term = sqrtm(cov_sqrt @ cov @ cov_sqrt)
// (style_transfer.py:179), M = (A cov) A into h.mmat.  n = 512: the Frobenius norms the two chains open with - of M and of the
// root, sqrtm.py:16,38 - come out of the products that make those matrices instead of two launches of their own on relu5_1's
// critical path: *m_partials partial sums of squares of M are left in h.ns.scalars + 8 (0: none).
inline int w2_open(const StyleHead& h, const float* root_t, hipStream_t s, int* m_partials) {
    if (launch_gemm_batch(one_gemm(h.n, root_t, h.cov, h.tmat, 0, 0), s)) return 1;
    GemmBatch mm = one_gemm(h.n, h.tmat, root_t, h.mmat, 0, 0);
    *m_partials = gemm_sumsq_fusable(h.n) ? (h.n / 32) * (h.n / 32) : 0;
    if (*m_partials) mm.p[0].sumsq_partials = h.ns.scalars + 8;
    return launch_gemm_batch(mm, s);
}
// the loss term (style_transfer.py:178-181) and the seed dL/d root = gdiag * I, which ride in the backward chain's opening kernel
inline W2LossJob w2_loss_job(const StyleHead& h, const float* mean_t, const float* cov_t, float weight, float* loss_out) {
    return W2LossJob{h.mean, mean_t, h.cov, cov_t, h.root, h.n, weight, loss_out, h.gdiag};
}
// Closing, from dL/dM in h.gm: M = (A cov) A with A constant, so d cov = A^T (G A^T); then (Ssym, b) and the bound on max |Ssym|
inline int w2_close(const StyleHead& h, const float* mean_t, const float* root_t, float weight, float* ssym, float* bvec,
                    unsigned int* ssym_amax, float mask_sum, hipStream_t s) {
    if (launch_gemm_batch(one_gemm(h.n, h.gm, root_t, h.dt, 0, 1), s)) return 1;
    if (launch_gemm_batch(one_gemm(h.n, root_t, h.dt, h.dcov, 1, 0), s)) return 1;
    return launch_style_grad_finish(h.dcov, h.mean, mean_t, h.n, weight, h.npix, ssym, bvec, s, ssym_amax, mask_sum);
}

// The Gram body, StyleLoss.forward (style_transfer.py:141-142) on h.srm: the scaled-MSE sums against the target, then D + D^T ->
// (Ssym, 0).  scratch: 2 kStreamBlocks floats, totals: 2, ticket: a zeroed device word.  ssym == nullptr: the value alone.
inline int gram_body(const StyleHead& h, const float* gram_t, float weight, float eps, float* scratch, float* totals,
                     unsigned int* ticket, float* loss_out, float* ssym, float* bvec, unsigned int* ssym_amax, float mask_sum, hipStream_t s) {
    if (launch_scaled_mse_sums(h.srm, gram_t, (long long)h.n * h.n, weight, scratch, totals, loss_out, s, ticket, eps)) return 1;
    if (!ssym) return 0;
    return launch_gram_grad_finish(h.srm, gram_t, totals, h.n, weight, h.npix, ssym, bvec, s, ssym_amax, mask_sum);
}

// The 1x1 step: out = h.ssym F + h.bvec 1^T over feat [n][height][width].  f16: large taps run the fp16x3 kernel scaled by feat_bound and
// h.s_amax (split-K problems, on h.conv_scratch, stay fp32).  out_amax: optional bound of out; out_mask: out = 0 where it is <= 0.
inline int head_step(const StyleHead& h, const float* feat, int height, int width, float* out, hipStream_t s, bool f16 = false,
                     unsigned int* feat_bound = nullptr, unsigned int* out_amax = nullptr, const float* out_mask = nullptr) {
    const long long npix = (long long)height * width;
    if (head_dgrad_small_applies(h.n, npix))       // a tap of <= 1024 pixels: one small-GEMM launch instead of split-K + reduce
        return launch_head_dgrad_small(h.ssym, feat, h.bvec, out_mask, out, h.n, npix, out_amax, s);
    ConvProblem c{};
    c.in = feat; c.wgt = h.ssym; c.bias = h.bvec; c.out = out; c.out_amax = out_amax; c.out_mask = out_mask;
    c.cin = h.n; c.cout = h.n; c.height = height; c.width = width; c.taps = 1;
    if (f16) { c.planes = 2; c.elem = 1; c.amax_word = feat_bound; c.wgt_amax = h.s_amax; }
    c.scratch = h.conv_scratch;
    return launch_conv(c, s);
}

// ---- memory.  The most Gram splits a head's workspace holds: 64 MiB of partials, 8 to 1024 of them
inline int head_gram_split_cap(int n) { return (int)std::min(1024ll, std::max(8ll, (16ll << 20) / ((long long)n * n))); }
// The 1x1 step's own split-K workspace (it runs on the head's stream, not the trunk's), needed only while the tap is too small
// to fill the chip (0: none).  launch_conv keeps >= 4 chunks of 8 channels per slice, i.e. splits at most n / 32 ways, and never
// beyond kConvScratchFloats.
inline size_t head_step_scratch_floats(int n, long long npix) {
    return ((npix + 255) / 256) * (n / 64) >= 512 ? 0 : std::min((size_t)(n / 32) * n * (size_t)npix, kConvScratchFloats);
}
// alloc: int(float** out, size_t floats), the caller's allocator (plan_alloc rounds to 256 bytes, a standalone head's does not).
// The Gram workspace for max_splits and the mean; with_step: also srm, (Ssym, b) and the 1x1 step's scratch for h.npix_local
template <class Alloc>
int alloc_head_moments(StyleHead& h, int max_splits, bool with_step, Alloc&& alloc) {
    const size_t n = (size_t)h.n, nn = n * n;
    h.gram.max_splits = max_splits;
    if (alloc(&h.gram.partial, max_splits * nn) || alloc(&h.gram.partial_sum, max_splits * n) || alloc(&h.mean, n)) return 1;
    if (!with_step) return 0;
    if (alloc(&h.srm, nn) || alloc(&h.ssym, nn) || alloc(&h.bvec, n)) return 1;
    const size_t scratch = head_step_scratch_floats(h.n, h.npix_local);
    return scratch ? alloc(&h.conv_scratch, scratch) : 0;
}
// what only the W2 kind needs; the Newton-Schulz workspace is zeroed on the null stream, which the caller synchronises
template <class Alloc>
int alloc_head_w2(StyleHead& h, Alloc&& alloc) {
    float* nsbase = nullptr;
    for (float** m : {&h.cov, &h.tmat, &h.mmat, &h.root, &h.gm, &h.dt, &h.dcov})
        if (alloc(m, (size_t)h.n * h.n)) return 1;
    if (alloc(&h.gdiag, 64) || alloc(&nsbase, ns_workspace_floats(h.n))) return 1;
    ns_workspace_carve(h.ns, nsbase, h.n);
    return ns_workspace_reset(h.ns, nullptr);
}

}  // namespace st
