// Configured taps (st_plan_set_taps): the reference's content_layers / style_layers / style_weights (style_transfer.py:315-322,
// read by every scale at :425-453) on any of the trunk's 17 taps, and the GENERAL closure that serves them.
//
// A plan describes its loss terms once (st_plan.h): the two lists as kProgram positions, a weight per listed entry, and the
// head, content target and seed buffer of a POSITION.  Both closures, the strips and the entry points below read that one
// store; st_plan::reference_taps only says which closure runs.
//
// The reference's own configuration - content [22], style [1, 6, 11, 20, 29] - stays on loss_and_grad (st_closure.hip): the
// fused conv1_1 Gram, the pools' argmax codes, the shallow heads in lockstep, the heads' streams.  Every other one runs
// general_loss_and_grad below, put together from the same parts without those specialisations:
//   TV                      writes grad_out                                             (launch_tv)
//   a plain forward         to the deepest configured layer, every map kept            (run_forward, no codes)
//   one W2 head per style layer, deepest first; dF goes into the position's SEED buffer (style_head on a HeadSite)
//   one MSE per content layer: its gradient is written to the seed buffer, or added to the one a style head of the same
//                           layer has written                                          (launch_content_mse, accumulate)
//   the terms' total        both loss arrays                                           (launch_sum_terms)
//   the tap backward        from the seeds to the pixels, onto the TV gradient, with the step's update folded into
//                           conv1_1's data gradient as in the default closure          (run_tap_backward, onto_image)
// on the caller's stream, in that order.  Masking by the producer, accumulation into seeded nodes and the fp16x3 bounds are
// run_tap_backward's, unchanged.  ST_GENERAL_TAPS=1 (st_set_option) sends the reference's configuration down this path too, so
// that it can be compared with the default closure on the same plan.
//
// Loss kinds (st_plan_set_loss_kinds for a whole list, st_plan_set_layer_loss_kinds per entry): a kind per LISTED entry says
// WHAT its term is, as the reference builds one module per layer.  The defaults - ContentLossMSE, StyleLossW2 - are the lines
// above.  Kind 1 of either list is the reference's ScaledMSELoss (st_pointwise.hip has the formulas), on the features
// (ContentLoss) or on the Gram matrix (StyleLoss).  Each entry also has its module's eps (st_plan_set_loss_eps): W2's
// covariance eps, in the target's root and the input's covariance, or ScaledMSELoss's, in the sums.  Any non-default kind
// or eps on any entry runs this closure, the reference's lists too, and every head runs by its own entry's kind:
//   a Gram head             the tap's second raw moment (moments_of_tap: no mean, no covariance), the sums and the term, then
//                           Ssym = (w / N) (D + D^T) with a zero b, and the W2 heads' own 1x1 step dF = Ssym F into the seed
//                           buffer (gram_head: four launches, no Newton-Schulz chain)
//   a scaled-MSE content term   the sums and the term, then the seed written or added  (launch_scaled_mse_sums / _grad)
// Everything around the terms - TV, the forward, the terms' total, the tap backward, the step's fold - is unchanged.
// (Either kind's launches are st_head_core.h's, shared with the standalone modules; gram_head and style_head add the plan's part.)
//
// A style mask (st_plan_set_style_mask, st_mask.hip) also runs this closure, the reference's configuration under the default
// kinds and eps included: every head's site carries sqrt(m) at its tap's level and the level's sum (mask_head_site), the Gram
// launch and the normalisers read them, and the head's seed buffer is multiplied by m per pixel column (launch_mask_columns)
// right behind the head's 1x1 step, before a content term of the same layer adds onto it.
//
// Style regions (st_plan_set_style_regions, st_mask.hip) run it too.  Per style entry, deepest first, and per region in order: a
// site with that region's level and sum, head, weight style_weight[j] rho_r and term slot (region_head_site) through the same
// style_head / gram_head.  Region 0 writes the seed and is multiplied by m_0 as above; region r >= 1 writes its 1x1 step into
// the plan's one scratch buffer, which launch_mask_columns_add adds onto the seed times m_r.  The entries' terms are then summed
// from the regions' in region order (launch_sum_region_terms) before the terms' total.  The bound words of the heads of regions
// r >= 1 lie in a block of their own, cleared here before the first head.
//
// Weight maps for the content and TV terms (st_plan_set_content_mask / st_plan_set_tv_mask, st_mask.hip) run it as well.  The TV
// launch gets the map (launch_tv's weighted kernels); a content entry gets the content map's level of its tap and runs the
// weighted siblings of its kind's launches (launch_content_mse_weighted, launch_scaled_mse_*_weighted), which write or add
// the seed as the unweighted ones do.  Everything behind the seeds is unchanged.
//
// A Laplacian loss (st_plan_set_laplacian, st_laplacian.hip) runs it as well: a pure image-space term like TV, launched right
// behind it - each pool size's term is added onto the TV term's slot (the image-space slot: the last entry of the terms) and
// its gradient onto the TV gradient, which run_tap_backward then adds the trunk's onto.
//
// A W2 entry flagged diagonal (st_plan_set_w2_diagonal, st_w2diag.hip) runs it too, on the reference's lists as well: that entry's
// head is two launches through the same site - the channel statistics with the term and the gradient's coefficients, then
// dF m_p written to the seed buffer (a region r >= 1: added onto it) - with no Gram pass, chain, 1x1 step, bound word,
// mask-column launch or region scratch.  Every other entry runs by its kind as above.
//
// So does a W2 entry flagged marginal (st_plan_set_w2_marginal, st_sort.hip): its head is the segmented sort of the tap's rows and
// the residual pass against the target's quantile functions, which writes dF to the seed buffer through the permutation.  Such an
// entry takes no style mask and no regions.
//
// So does a W2 entry flagged nearest (st_plan_set_style_nearest, st_nearest.hip): its head is the fused search - the scores of the
// tap's pixels against the style's feature vectors, reduced to one match per pixel without ever being written - and the finish
// pass, which writes dF = w (2 / (C N)) (f - s_k*) to the seed buffer and keeps the matches (st_plan_nearest_indices).  Such an
// entry takes no style mask and no regions either.
//
// So does a W2 entry flagged sliced (st_plan_set_style_sliced, st_sliced.hip): with resampling on its head draws new unit
// directions at the plan's epoch and derives the target again from the stored style vectors - project, sort, resample, blend - and
// in either case projects the tap, sorts and takes the residual on P rows and writes dF = R^T G to the seed buffer through the
// 1x1 step.  The epoch is a host counter, advanced at the end of every evaluation of this closure (it is never captured).  Such an
// entry takes no style mask and no regions either.
#include <algorithm>
#include <cmath>

#include "st_plan.h"

namespace st {

namespace {
// the reference's own lists and weights (style_transfer.py:315-322, :366): what a fresh plan holds
constexpr int kContentFeat = 22;
const int kStyleFeat[5] = {1, 6, 11, 20, 29};
const float kStyleWeight[5] = {256.f / 341, 64.f / 341, 16.f / 341, 4.f / 341, 1.f / 341};

// the kind of a list of n entries: the one they agree on (an empty list: what a later entry would get), -1: they differ
int list_kind(const int* kinds, int n) {
    for (int i = 1; i < n; ++i)
        if (kinds[i] != kinds[0]) return -1;
    return kinds[0];
}

// every target set before is gone, every bound word is dealt again, and nothing built on the former terms survives
void drop_targets(st_plan* p) {
    for (int op = 0; op < kNumOps; ++op) {
        p->head[op].target_set = false;
        for (int r = 1; r < kMaxRegions; ++r) p->region_head[r - 1][op].target_set = false;
        p->content_set[op] = false;
    }
    assign_head_bounds(p);
    invalidate_graph(p);
    p->phases.clear();
}
}  // namespace

int tap_position(int layer) {
    for (int i = 0; i < kNumOps; ++i)
        if (kProgram[i].feat_index == layer) return i;
    return -1;
}

// every listed entry is of the default kind (ContentLossMSE / StyleLossW2) ... and has its kind's default eps
static bool default_kinds(const st_plan* p) {
    bool ok = true;
    for (int i = 0; i < p->n_content; ++i) ok = ok && p->content_kind[i] == 0;
    for (int j = 0; j < p->n_style; ++j) ok = ok && p->style_kind[j] == 0;
    return ok;
}
static bool any_diagonal(const st_plan* p) {
    bool any = false;
    for (int j = 0; j < p->n_style; ++j) any = any || p->style_diag[j] != 0;
    return any;
}
static bool any_marginal(const st_plan* p) {
    bool any = false;
    for (int j = 0; j < p->n_style; ++j) any = any || p->style_marg[j] != 0;
    return any;
}
static bool any_nearest(const st_plan* p) {
    bool any = false;
    for (int j = 0; j < p->n_style; ++j) any = any || p->style_near[j] != 0;
    return any;
}
static bool any_sliced(const st_plan* p) {
    bool any = false;
    for (int j = 0; j < p->n_style; ++j) any = any || p->style_sliced[j] != 0;
    return any;
}
static bool default_eps(const st_plan* p) {
    bool ok = true;
    for (int i = 0; i < p->n_content; ++i) ok = ok && p->content_eps[i] < 0.f;
    for (int j = 0; j < p->n_style; ++j) ok = ok && p->style_eps[j] < 0.f;
    return ok;
}

bool general_taps(const st_plan* p) {
    static Option force("ST_GENERAL_TAPS", 0);
    return !p->strip && (!p->reference_taps || !default_kinds(p) || !default_eps(p) || p->style_mask || p->n_regions > 0 ||
                         p->content_mask || p->tv_mask || p->n_lap > 0 || any_diagonal(p) || any_marginal(p) || any_nearest(p) ||
                         any_sliced(p) || force.get() != 0);
}

float style_eps_of(const st_plan* p, int j) {
    return p->style_eps[j] >= 0.f ? p->style_eps[j] : p->style_kind[j] == 1 ? kScaledMseEps : kCovEps;
}

float content_eps_of(const st_plan* p, int i) {
    return p->content_kind[i] == 0 ? -1.f : p->content_eps[i] >= 0.f ? p->content_eps[i] : kScaledMseEps;
}

int alloc_kind_of(const st_plan* p, int j) { return p->style_near[j] ? 4 : p->style_marg[j] ? 3 : p->style_diag[j] ? 2 : p->style_kind[j]; }

int closure_top_op(const st_plan* p) {
    if (!general_taps(p)) return kNumOps - 1;
    int top = 0;
    for (int i = 0; i < p->n_content; ++i) top = std::max(top, p->content_op[i]);
    for (int i = 0; i < p->n_style; ++i) top = std::max(top, p->style_op[i]);
    return top;
}

bool targets_ready(const st_plan* p) {
    bool ok = true;
    for (int i = 0; i < p->n_content; ++i) ok = ok && p->content_set[p->content_op[i]];
    for (int r = 0; r < std::max(p->n_regions, 1); ++r)
        for (int j = 0; j < p->n_style; ++j) ok = ok && region_head_at(p, r, p->style_op[j]).target_set;
    return ok;
}

// the reference's configuration: the 8-float array IS the terms in SumLoss order, whichever closure runs
float* loss_terms(st_plan* p) { return p->reference_taps ? p->losses : p->terms; }

int sliced_projections_of(const st_plan* p, int j) { return p->sliced_proj[j] ? p->sliced_proj[j] : p->head[p->style_op[j]].n; }

// flagged entry j's directions at `epoch` and its target from the stored style vectors: per image project, sort, unpack, resample
// to the tap's N, and blend in image order
int sliced_refresh(st_plan* p, int j, unsigned long long epoch, hipStream_t s) {
    StyleHead& h = p->head[p->style_op[j]];
    const int proj = sliced_projections_of(p, j);
    const bool f16 = p->net->conv_elem == 1;
    if (launch_sliced_directions(p->sliced_seed, j, epoch, proj, h.n, h.sl_r, h.sl_rt, s)) return 1;
    h.sl_epoch = epoch;
    const SlicedScratch sc = sliced_scratch_of(h.sl_scratch, proj, h.sl_rows);
    const unsigned int* bounds = reinterpret_cast<const unsigned int*>(h.sl_bounds);
    const float* feat = h.sl_feats;
    for (int i = 0; i < h.sl_images; ++i) {
        if (sliced_target_add(feat, h.n, h.sl_m[i], h.sl_r, h.sl_rt, proj, h.npix_local, sc, f16 ? bounds + (size_t)(1 + i) * kAmaxWordUints : nullptr,
                              f16 ? bounds : nullptr, h.sl_t, i > 0, h.sl_a[i], s))
            return 1;
        feat += (size_t)h.n * (size_t)h.sl_m[i];
    }
    return 0;
}

namespace {

// the j-th listed head as THIS closure runs it: dF goes to the position's seed buffer (run_tap_backward commits the bound),
// the term behind the content terms, and none of the default closure's slot-keyed specialisations apply
HeadSite general_head_site(st_plan* p, int j) {
    HeadSite at = head_site(p, j);
    at.loss = loss_terms(p) + p->n_content + j;
    at.grad = p->tap_seed[p->style_op[j]];
    at.grad_amax = nullptr;
    at.slot = -1;
    return at;
}

// ... and of region r while style regions are in force: that region's level of its own pyramid, its head of the position, the
// entry's weight times rho_r, and the (region, entry) term.  Region r >= 1 writes its 1x1 step into the scratch buffer.
HeadSite region_head_site(st_plan* p, int j, int r) {
    HeadSite at = general_head_site(p, j);
    const int op = p->style_op[j];
    int level = 0;
    for (int i = 0; i <= op; ++i) level += kProgram[i].kind == 1;
    at.h = &region_head_at(p, r, op);
    at.weight = p->style_weight[j] * p->region_weight[r];
    at.loss = p->region_terms + (size_t)r * p->n_style + j;
    if (r > 0) at.grad = p->region_scratch;
    at.sqrt_mask = p->region_sqrt[r][level];
    at.mask_sum = (float)p->region_sum[r][level];
    return at;
}

// the totals (sum d^2, sum |d| + eps) of scaled-MSE term k in SumLoss order, behind the per-block partials
float* kind_totals(st_plan* p, int k) { return p->kind_scratch + 2 * kStreamBlocks + 2 * k; }

// StyleLoss (style_transfer.py:129-142) under Scale(weight) + its backward down to the tap's feature gradient.  The term's
// scratch and ticket are shared with the content terms: every launch of this closure is on the caller's stream.
int gram_head(st_plan* p, const HeadSite& at, int term, hipStream_t s) {
    StyleHead& h = *at.h;
    if (moments_of_tap(p, at, h.mean, h.srm, s)) return 1;
    if (gram_body(h, h.gram_t, at.weight, at.eps, p->kind_scratch, kind_totals(p, term), p->tickets + 128, at.loss, h.ssym, h.bvec,
                  p->net->conv_elem == 1 ? h.s_amax : nullptr, at.mask_sum, s))
        return 1;
    return style_head_gradient(p, at, s);
}

// A W2 entry flagged diagonal (st_plan_set_w2_diagonal, st_w2diag.hip): the stats launch - moments, term, coefficients - and the
// gradient launch, which writes dF m_p to the seed (accumulate: adds it, a region r >= 1).  The site's mask and normaliser are
// read by both, so no launch_mask_columns follows; no bound word is touched.
int diag_head(st_plan* p, const HeadSite& at, float* seed, int accumulate, hipStream_t s) {
    return diag_head_run(*at.h, at.tap->y, at.weight, at.eps, at.sqrt_mask, at.mask_sum, at.loss, seed, accumulate, s);
}

// A W2 entry flagged marginal (st_plan_set_w2_marginal, st_sort.hip): the sort of the tap's rows, then the residual pass, which
// writes dF to the seed through the permutation and the weighted term to the entry's slot.  No mask, no eps, no bound word.
int marginal_head(st_plan* p, const HeadSite& at, float* seed, hipStream_t s) {
    const StyleHead& h = *at.h;
    return marginal_head_run(at.tap->y, h.n, h.npix_local, h.marg_t, h.marg_scratch, at.weight, seed, at.loss, s);
}

// A W2 entry flagged nearest (st_plan_set_style_nearest, st_nearest.hip): the search against the style set, then the finish pass,
// which writes dF to the seed, the matches to the head and the weighted term to the entry's slot.  No mask, no eps.  The tap's
// bound word where the producing convolution leaves one (fp16x3 trunks), otherwise measured by the search's launcher.
// Entry j's metric (st_plan_set_nearest_metric) picks the finish pass: cosine and centred cosine run the same search on the unit
// rows and the bias the setter prepared, then the cosine finish (st_nearest.hip).
int nearest_head(st_plan* p, int j, const HeadSite& at, float* seed, hipStream_t s) {
    const StyleHead& h = *at.h;
    const NearestPrepared pr = nearest_prepared_of(h.near_prep, h.n, h.near_m);
    const NearestScratch sc = nearest_scratch_of(h.near_scratch, h.n, h.npix_local, h.near_m);
    const unsigned int* bound = p->net->conv_elem == 1 ? at.tap->y_amax : nullptr;
    if (p->style_near_metric[j])
        return nearest_cosine_head_run(at.tap->y, h.n, h.npix_local, pr, sc, bound, at.weight, h.near_idx, seed, at.loss, s);
    return nearest_head_run(at.tap->y, h.n, h.npix_local, pr, sc, bound, at.weight, h.near_idx, nullptr, seed, at.loss, s);
}

// A W2 entry flagged sliced (st_plan_set_style_sliced, st_sliced.hip).  Resampling on: the directions of the plan's epoch and the
// target from the stored style vectors, image by image in image order.  Then the head.  No mask, no eps.  fp16x3 trunks: both
// products in fp16x3 under the tap's bound word, R's (1 by construction), each image's (measured by the setter) and G's (measured
// here); an fp32 trunk: the exact fp32 MFMA.
int sliced_head(st_plan* p, int j, const HeadSite& at, float* seed, hipStream_t s) {
    StyleHead& h = *at.h;
    const int proj = sliced_projections_of(p, j);
    const bool f16 = p->net->conv_elem == 1;
    if (p->sliced_resample[j] && sliced_refresh(p, j, p->sliced_epoch, s)) return 1;
    const SlicedScratch sc = sliced_scratch_of(h.sl_scratch, proj, h.sl_rows);
    const unsigned int* rb = reinterpret_cast<const unsigned int*>(h.sl_bounds);
    return sliced_head_run(at.tap->y, h.n, h.npix_local, h.sl_r, h.sl_rt, proj, h.sl_t, sc, f16 ? at.tap->y_amax : nullptr,
                           f16 ? rb : nullptr, at.weight, seed, at.loss, s);
}

// Style regions in force: the heads of every listed entry, in `order`, one per region in region order.  dF_r's pixel columns
// times m_r: region 0 in place on the seed it wrote (the masked plan's launches), region r >= 1 from the scratch buffer ONTO the
// seed.  Then each entry's term from its regions' terms.
int region_heads(st_plan* p, const int* order, bool* styled, hipStream_t s) {
    const int nc = p->n_content, ns = p->n_style, regions = p->n_regions;
    if (regions > 1)
        ST_HIP(hipMemsetAsync(p->region_amax, 0, (size_t)(kMaxRegions - 1) * 16 * kAmaxWordUints * sizeof(unsigned int), s));
    for (int k = 0; k < ns; ++k) {
        const int j = order[k];
        float* seed = p->tap_seed[p->style_op[j]];
        for (int r = 0; r < regions; ++r) {
            const HeadSite at = region_head_site(p, j, r);
            ST_REQUIRE(!p->style_marg[j], "style layer %d is flagged marginal (st_plan_set_w2_marginal): it takes no style regions", j);
            ST_REQUIRE(!p->style_near[j], "style layer %d is flagged nearest (st_plan_set_style_nearest): it takes no style regions", j);
            ST_REQUIRE(!p->style_sliced[j], "style layer %d is flagged sliced (st_plan_set_style_sliced): it takes no style regions", j);
            if (p->style_diag[j]) {            // region 0 writes the seed, region r >= 1 adds onto it: no scratch buffer
                if (diag_head(p, at, seed, r > 0, s)) return 1;
                continue;
            }
            if (p->style_kind[j] == 1 ? gram_head(p, at, nc + j, s) : style_head(p, at, s)) return 1;
            if (r == 0 ? launch_mask_columns(seed, at.sqrt_mask, at.h->n, at.h->npix, s)
                       : launch_mask_columns_add(seed, at.grad, at.sqrt_mask, at.h->n, at.h->npix, s))
                return 1;
        }
        styled[p->style_op[j]] = true;
    }
    return launch_sum_region_terms(p->region_terms, regions, ns, loss_terms(p) + nc, s);
}

// seed buffers of the tapped positions and the terms' array
int ensure_tap_buffers(st_plan* p) {
    if (!default_kinds(p) && !p->kind_scratch &&
        plan_alloc(p, &p->kind_scratch, 2 * kStreamBlocks + 2 * 32))
        return 1;
    if (!p->terms) {
        if (plan_alloc(p, &p->terms, 64)) return 1;
        ST_HIP(hipMemset(p->terms, 0, 64 * sizeof(float)));
    }
    auto seed = [&](int op) { return p->tap_seed[op] ? 0 : plan_alloc(p, &p->tap_seed[op], node_at(p, op).count()); };
    for (int i = 0; i < p->n_content; ++i)
        if (seed(p->content_op[i])) return 1;
    for (int i = 0; i < p->n_style; ++i)
        if (seed(p->style_op[i])) return 1;
    // style regions: one buffer of the largest listed style tap for the 1x1 steps of regions r >= 1
    size_t largest = 0;
    for (int i = 0; p->n_regions > 1 && i < p->n_style; ++i)
        if (!p->style_diag[i]) largest = std::max(largest, node_at(p, p->style_op[i]).count());      // (a diagonal entry needs none)
    if (largest > p->region_scratch_floats) {
        p->region_scratch = nullptr;         // (the smaller one stays the plan's until it is destroyed)
        if (plan_alloc(p, &p->region_scratch, largest)) { p->region_scratch_floats = 0; return 1; }
        p->region_scratch_floats = largest;
    }
    return 0;
}

}  // namespace

int general_loss_and_grad(st_plan* p, const float* image, float* grad_out, float* losses_out, hipStream_t s) {
    if (require_targets(p) || ensure_grad_alloc(p) || ensure_streams(p, s) || ensure_tap_buffers(p)) return 1;
    const int nc = p->n_content, ns = p->n_style;
    float* terms = loss_terms(p);
    // TVLoss on the un-normalised image (style_transfer.py:376): WRITES grad_out; conv1_1's data gradient adds to it
    const float* tv_map = p->tv_mask ? p->tv_map : nullptr;
    if (hbm_profiled(p, HBM_TV, (2.0 * 3 + (tv_map ? 1 : 0)) * 4.0 * p->H * p->W, s, [&] {
            return launch_tv(image, p->H, p->W, p->tv_weight, grad_out, p->red_partials, terms + nc + ns, s, p->tickets + 0, tv_map);
        }))
        return 1;
    // the Laplacian terms (st_plan_set_laplacian): onto the TV term's slot and onto the gradient it wrote, before the trunk's
    if (p->n_lap && laplacian_terms(p, image, grad_out, terms + nc + ns, s)) return 1;
    const int top = closure_top_op(p);
    if (run_forward(p, image, kProgram[top].feat_index, s, /*fork_heads=*/false)) return 1;
    // style heads, deepest first (the deepest one's gradient is what the backward starts from)
    int order[16];
    for (int j = 0; j < ns; ++j) order[j] = j;
    std::sort(order, order + ns, [&](int a, int b) { return p->style_op[a] > p->style_op[b]; });
    bool styled[kNumOps] = {};
    if (p->n_regions) {
        if (region_heads(p, order, styled, s)) return 1;
    } else {
        for (int k = 0; k < ns; ++k) {
            const HeadSite at = general_head_site(p, order[k]);
            if (p->style_sliced[order[k]]) {
                if (sliced_head(p, order[k], at, at.grad, s)) return 1;
                styled[p->style_op[order[k]]] = true;
                continue;
            }
            if (p->style_near[order[k]]) {
                if (nearest_head(p, order[k], at, at.grad, s)) return 1;
                styled[p->style_op[order[k]]] = true;
                continue;
            }
            if (p->style_marg[order[k]]) {
                if (marginal_head(p, at, at.grad, s)) return 1;
                styled[p->style_op[order[k]]] = true;
                continue;
            }
            if (p->style_diag[order[k]]) {
                if (diag_head(p, at, at.grad, 0, s)) return 1;
                styled[p->style_op[order[k]]] = true;
                continue;
            }
            if (p->style_kind[order[k]] == 1 ? gram_head(p, at, nc + order[k], s) : style_head(p, at, s)) return 1;
            // a style mask: dF's pixel columns times m, on the seed as the head's 1x1 step left it and BEFORE a content term of
            // the same layer adds onto it
            if (at.sqrt_mask && launch_mask_columns(at.grad, at.sqrt_mask, at.h->n, at.h->npix, s)) return 1;
            styled[p->style_op[order[k]]] = true;
        }
    }
    // ContentLossMSE per content layer (style_transfer.py:425-429), behind the style head of the same layer where there is one;
    // an entry of kind 1: ContentLoss, its sums and then its seed
    for (int i = 0; i < nc; ++i) {
        const int op = p->content_op[i];
        const Node& ct = node_at(p, op);
        if (p->content_mask) {
            // a content map: the level of the pools at or before the tap, and the weighted siblings of the entry's launches
            int level = 0;
            for (int k = 0; k <= op; ++k) level += kProgram[k].kind == 1;
            const float* wmap = p->content_map[level];
            const long long npix = (long long)ct.h * ct.w, count = (long long)ct.count();
            const double map_bytes = 4.0 * (double)npix;
            if (p->content_kind[i] == 1) {
                float* totals = kind_totals(p, i);
                if (hbm_profiled(p, HBM_CONTENT, 2.0 * 4.0 * ct.count() + map_bytes, s, [&] {
                        return launch_scaled_mse_sums_weighted(ct.y, p->content_target[op], wmap, count, npix, p->content_weight[i],
                                                               p->kind_scratch, totals, terms + i, s, p->tickets + 128,
                                                               content_eps_of(p, i));
                    }) ||
                    hbm_profiled(p, HBM_CONTENT, (styled[op] ? 4.0 : 3.0) * 4.0 * ct.count() + map_bytes, s, [&] {
                        return launch_scaled_mse_grad_weighted(ct.y, p->content_target[op], wmap, count, npix, p->content_weight[i],
                                                               totals, p->tap_seed[op], s, styled[op] ? 1 : 0);
                    }))
                    return 1;
            } else if (hbm_profiled(p, HBM_CONTENT, 3.0 * 4.0 * ct.count() + map_bytes, s, [&] {
                           return launch_content_mse_weighted(ct.y, p->content_target[op], wmap, count, npix, p->content_weight[i],
                                                              p->tap_seed[op], p->red_partials + 4 * kStreamBlocks, terms + i, s,
                                                              p->tickets + 64, styled[op] ? 1 : 0);
                       })) {
                return 1;
            }
            continue;
        }
        if (p->content_kind[i] == 1) {
            float* totals = kind_totals(p, i);
            if (hbm_profiled(p, HBM_CONTENT, 2.0 * 4.0 * ct.count(), s, [&] {
                    return launch_scaled_mse_sums(ct.y, p->content_target[op], (long long)ct.count(), p->content_weight[i],
                                                  p->kind_scratch, totals, terms + i, s, p->tickets + 128, content_eps_of(p, i));
                }) ||
                hbm_profiled(p, HBM_CONTENT, (styled[op] ? 4.0 : 3.0) * 4.0 * ct.count(), s, [&] {
                    return launch_scaled_mse_grad(ct.y, p->content_target[op], (long long)ct.count(), p->content_weight[i], totals,
                                                  p->tap_seed[op], s, styled[op] ? 1 : 0);
                }))
                return 1;
            continue;
        }
        if (hbm_profiled(p, HBM_CONTENT, 3.0 * 4.0 * ct.count(), s, [&] {
                return launch_content_mse(ct.y, p->content_target[op], (long long)ct.count(), p->content_weight[i], p->tap_seed[op],
                                          p->red_partials + 4 * kStreamBlocks, terms + i, s, p->tickets + 64, styled[op] ? 1 : 0);
            }))
            return 1;
    }
    if (p->reference_taps) {
        if (!p->defer_sum && launch_sum_losses(p->losses, s, losses_out)) return 1;
    } else if (launch_sum_terms(terms, nc, ns, p->losses, s, p->defer_sum ? nullptr : losses_out)) {
        // (a step's tail sums the 8-float array once more - the same additions - and fills losses_out)
        return 1;
    }
    // sliced heads that resample: the next closure draws its directions at the next epoch
    for (int j = 0, bump = 1; j < ns; ++j)
        if (bump && p->style_sliced[j] && p->sliced_resample[j]) {
            ++p->sliced_epoch;
            bump = 0;
        }
    const float* seed[kNumOps] = {};
    for (int i = 0; i < nc; ++i) seed[p->content_op[i]] = p->tap_seed[p->content_op[i]];
    for (int j = 0; j < ns; ++j) seed[p->style_op[j]] = p->tap_seed[p->style_op[j]];
    return run_tap_backward(p, seed, grad_out, s, /*onto_image=*/true);
}

}  // namespace st

using namespace st;

extern "C" {

int st_plan_set_taps(st_plan* p, int n_content, const int* content_layers, int n_style, const int* style_layers) {
    ST_REQUIRE(p, "st_plan_set_taps: null plan");
    ST_REQUIRE(!p->strip, "st_plan_set_taps: strip plans run the reference's layers only (content [22], style [1, 6, 11, 20, 29])");
    ST_REQUIRE(n_content >= 0 && n_content <= 16 && n_style >= 0 && n_style <= 16,
               "st_plan_set_taps: %d content and %d style layers: each list holds 0 to 16", n_content, n_style);
    ST_REQUIRE(n_content + n_style >= 1, "st_plan_set_taps: both lists are empty");
    ST_REQUIRE((n_content == 0 || content_layers) && (n_style == 0 || style_layers), "st_plan_set_taps: null list");
    int cop[16] = {}, sop[16] = {};
    for (int pass = 0; pass < 2; ++pass) {
        const int n = pass ? n_style : n_content;
        const int* layers = pass ? style_layers : content_layers;
        int* ops = pass ? sop : cop;
        for (int i = 0; i < n; ++i) {
            ops[i] = tap_position(layers[i]);
            ST_REQUIRE(ops[i] >= 0,
                       "st_plan_set_taps: features[%d] is not one of the 17 taps (ReLU outputs 1 3 6 8 11 13 15 17 20 22 24 26 29, "
                       "pool outputs 4 9 18 27): pre-ReLU convolution outputs are not kept by the fused trunk", layers[i]);
            for (int k = 0; k < i; ++k)
                ST_REQUIRE(ops[k] != ops[i], "st_plan_set_taps: features[%d] is named twice in the %s list", layers[i],
                           pass ? "style" : "content");
        }
    }
    bool ref = n_content == 1 && content_layers[0] == kContentFeat && n_style == 5;
    for (int j = 0; ref && j < 5; ++j) ref = style_layers[j] == kStyleFeat[j];
    // everything the configuration needs, now (the reference's lists too, whose heads a plan that was never configured
    // allocates when their targets are set): a failed allocation leaves the plan as it was
    for (int i = 0; i < n_content; ++i)
        if (!p->content_target[cop[i]] && plan_alloc(p, &p->content_target[cop[i]], node_at(p, cop[i]).count())) return 1;
    // (the kinds: a list whose entries agree keeps that kind for its new entries, a mixed one returns to kind 0; every eps
    // returns to its kind's default)
    const int ckind = std::max(list_kind(p->content_kind, p->n_content), 0), skind = std::max(list_kind(p->style_kind, p->n_style), 0);
    for (int j = 0; j < n_style; ++j)
        if (ensure_style_alloc(p, p->head[sop[j]], skind)) return 1;
    int skinds[16];
    std::fill(skinds, skinds + 16, skind);
    if (ensure_region_heads(p, p->n_regions, sop, n_style, skinds)) return 1;       // (style regions in force: they stay)
    // the weights: the reference's lists named again keep theirs; every other change of lists starts from the new lists'
    // defaults - the reference's content_weight split over the layers (:366) and equal style weights, or, for the reference's
    // own lists, its own style weights
    const bool keep_weights = ref && p->reference_taps;
    p->reference_taps = ref;
    p->n_content = n_content;
    p->n_style = n_style;
    for (int i = 0; i < 16; ++i) {
        p->content_op[i] = i < n_content ? cop[i] : 0;
        p->style_op[i] = i < n_style ? sop[i] : 0;
        p->content_kind[i] = ckind;
        p->style_kind[i] = skind;
        p->content_eps[i] = p->style_eps[i] = -1.f;
        p->style_diag[i] = p->style_marg[i] = p->style_near[i] = p->style_near_metric[i] = p->style_sliced[i] = 0;
        if (keep_weights) continue;
        p->content_weight[i] = i < n_content ? 0.015f / (float)n_content : 0.f;
        p->style_weight[i] = i >= n_style ? 0.f : ref ? kStyleWeight[i] : 1.f / (float)n_style;
    }
    // a head or target buffer serves whichever lists name its position: every target set before is gone, every bound word
    // is dealt again, and nothing built on the former lists survives
    drop_targets(p);
    return 0;
}

namespace {

// what both kinds setters do once the codes are checked: `ck` / `sk` hold 16 codes each, the listed entries first
int apply_loss_kinds(st_plan* p, const int* ck, const int* sk) {
    // what the listed heads need under their new kinds, now: a failed allocation leaves the plan as it was
    for (int j = 0; j < p->n_style; ++j)
        if (ensure_style_alloc(p, p->head[p->style_op[j]], sk[j])) return 1;
    if (ensure_region_heads(p, p->n_regions, p->style_op, p->n_style, sk)) return 1;
    for (int i = 0; i < 16; ++i) {
        p->content_kind[i] = ck[i];
        p->style_kind[i] = sk[i];
        p->content_eps[i] = p->style_eps[i] = -1.f;      // an eps belongs to a module of one kind: set it after the kinds
        p->style_diag[i] = p->style_marg[i] = p->style_near[i] = p->style_near_metric[i] = p->style_sliced[i] = 0;      // ... and so do the diagonal, marginal, nearest and sliced flags of a W2 entry
    }
    // a target is kept in the form its kind reads (a root, or a Gram matrix): as after st_plan_set_taps, every target set
    // before is gone, every bound word is dealt again and nothing built on the former terms survives.  The lists and all
    // weights stay.
    drop_targets(p);
    return 0;
}

}  // namespace

int st_plan_set_loss_kinds(st_plan* p, int content_kind, int style_kind) {
    ST_REQUIRE(p, "st_plan_set_loss_kinds: null plan");
    ST_REQUIRE(content_kind == 0 || content_kind == 1,
               "st_plan_set_loss_kinds: unknown content loss kind %d (0: mse - ContentLossMSE, 1: scaled_mse - ContentLoss)", content_kind);
    ST_REQUIRE(style_kind == 0 || style_kind == 1,
               "st_plan_set_loss_kinds: unknown style loss kind %d (0: w2 - StyleLossW2, 1: gram - StyleLoss)", style_kind);
    ST_REQUIRE(!p->strip || (content_kind == 0 && style_kind == 0),
               "st_plan_set_loss_kinds: strip plans run the default loss kinds only (content mse, style w2)");
    int ck[16], sk[16];
    std::fill(ck, ck + 16, content_kind);
    std::fill(sk, sk + 16, style_kind);
    return apply_loss_kinds(p, ck, sk);
}

int st_plan_loss_kinds(const st_plan* p, int* content_kind, int* style_kind) {
    ST_REQUIRE(p, "st_plan_loss_kinds: null plan");
    if (content_kind) *content_kind = list_kind(p->content_kind, p->n_content);
    if (style_kind) *style_kind = list_kind(p->style_kind, p->n_style);
    return 0;
}

int st_plan_set_layer_loss_kinds(st_plan* p, const int* content_kinds, const int* style_kinds) {
    ST_REQUIRE(p, "st_plan_set_layer_loss_kinds: null plan");
    ST_REQUIRE((p->n_content == 0 || content_kinds) && (p->n_style == 0 || style_kinds), "st_plan_set_layer_loss_kinds: null list");
    int ck[16], sk[16];
    bool all_default = true;
    for (int i = 0; i < p->n_content; ++i) {
        ST_REQUIRE(content_kinds[i] == 0 || content_kinds[i] == 1,
                   "st_plan_set_layer_loss_kinds: unknown content loss kind %d for content layer %d (0: mse - ContentLossMSE, "
                   "1: scaled_mse - ContentLoss)", content_kinds[i], i);
        ck[i] = content_kinds[i];
        all_default = all_default && ck[i] == 0;
    }
    for (int j = 0; j < p->n_style; ++j) {
        ST_REQUIRE(style_kinds[j] == 0 || style_kinds[j] == 1,
                   "st_plan_set_layer_loss_kinds: unknown style loss kind %d for style layer %d (0: w2 - StyleLossW2, 1: gram - StyleLoss)",
                   style_kinds[j], j);
        sk[j] = style_kinds[j];
        all_default = all_default && sk[j] == 0;
    }
    ST_REQUIRE(!p->strip || all_default,
               "st_plan_set_layer_loss_kinds: strip plans run the default loss kinds only (content mse, style w2)");
    // the unlisted entries: what st_plan_set_loss_kinds would leave there for a list whose entries agree (an empty list keeps
    // what it has), kind 0 for a mixed one
    const int cu = p->n_content ? std::max(list_kind(ck, p->n_content), 0) : p->content_kind[0];
    const int su = p->n_style ? std::max(list_kind(sk, p->n_style), 0) : p->style_kind[0];
    std::fill(ck + p->n_content, ck + 16, cu);
    std::fill(sk + p->n_style, sk + 16, su);
    return apply_loss_kinds(p, ck, sk);
}

int st_plan_layer_loss_kinds(const st_plan* p, int* content_kinds, int* style_kinds) {
    ST_REQUIRE(p, "st_plan_layer_loss_kinds: null plan");
    for (int i = 0; content_kinds && i < p->n_content; ++i) content_kinds[i] = p->content_kind[i];
    for (int j = 0; style_kinds && j < p->n_style; ++j) style_kinds[j] = p->style_kind[j];
    return 0;
}

int st_plan_set_loss_eps(st_plan* p, const float* content_eps, const float* style_eps) {
    ST_REQUIRE(p, "st_plan_set_loss_eps: null plan");
    float ce[16], se[16];
    std::fill(ce, ce + 16, -1.f);
    std::fill(se, se + 16, -1.f);
    bool all_default = true;
    for (int pass = 0; pass < 2; ++pass) {
        const float* given = pass ? style_eps : content_eps;
        const int n = pass ? p->n_style : p->n_content;
        for (int i = 0; given && i < n; ++i) {
            const float e = given[i];
            ST_REQUIRE(std::isfinite(e), "st_plan_set_loss_eps: eps of %s layer %d is not finite", pass ? "style" : "content", i);
            if (e < 0.f) continue;                   // negative: the kind's default
            ST_REQUIRE(pass || p->content_kind[i] != 0,
                       "st_plan_set_loss_eps: content layer %d is of kind mse (ContentLossMSE), which has no eps: pass a negative value", i);
            const float dflt = pass ? (p->style_kind[i] == 1 ? kScaledMseEps : kCovEps) : kScaledMseEps;
            if (e == dflt) continue;                 // the default, given as a number, IS the default
            (pass ? se : ce)[i] = e;
            all_default = false;
        }
    }
    ST_REQUIRE(!p->strip || all_default, "st_plan_set_loss_eps: strip plans run the loss modules' default eps only");
    for (int j = 0; j < p->n_style; ++j)
        ST_REQUIRE(!p->style_marg[j] || se[j] < 0.f,
                   "st_plan_set_loss_eps: style layer %d is flagged marginal (st_plan_set_w2_marginal), whose term has no eps", j);
    for (int j = 0; j < p->n_style; ++j)
        ST_REQUIRE(!p->style_near[j] || se[j] < 0.f,
                   "st_plan_set_loss_eps: style layer %d is flagged nearest (st_plan_set_style_nearest), whose term has no eps", j);
    for (int j = 0; j < p->n_style; ++j)
        ST_REQUIRE(!p->style_sliced[j] || se[j] < 0.f,
                   "st_plan_set_loss_eps: style layer %d is flagged sliced (st_plan_set_style_sliced), whose term has no eps", j);
    std::copy(ce, ce + 16, p->content_eps);
    std::copy(se, se + 16, p->style_eps);
    // a W2 target is kept as the root of cov_t + eps I: every target set before is gone
    drop_targets(p);
    return 0;
}

int st_plan_set_w2_diagonal(st_plan* p, const int* flags) {
    ST_REQUIRE(p, "st_plan_set_w2_diagonal: null plan");
    int fl[16] = {};
    bool any = false;
    for (int j = 0; flags && j < p->n_style; ++j) {
        ST_REQUIRE(flags[j] == 0 || flags[j] == 1, "st_plan_set_w2_diagonal: flag %d of style layer %d: 0 or 1", flags[j], j);
        ST_REQUIRE(flags[j] == 0 || p->style_kind[j] == 0,
                   "st_plan_set_w2_diagonal: style layer %d is of kind gram (StyleLoss): only a w2 layer's covariances can be diagonal", j);
        ST_REQUIRE(flags[j] == 0 || !p->style_marg[j],
                   "st_plan_set_w2_diagonal: style layer %d is flagged marginal (st_plan_set_w2_marginal): a layer takes one of the two", j);
        ST_REQUIRE(flags[j] == 0 || !p->style_near[j],
                   "st_plan_set_w2_diagonal: style layer %d is flagged nearest (st_plan_set_style_nearest): a layer takes one of the two", j);
        ST_REQUIRE(flags[j] == 0 || !p->style_sliced[j],
                   "st_plan_set_w2_diagonal: style layer %d is flagged sliced (st_plan_set_style_sliced): a layer takes one of the two", j);
        fl[j] = flags[j];
        any = any || fl[j] != 0;
    }
    ST_REQUIRE(!p->strip || !any, "st_plan_set_w2_diagonal: strip plans run full W2 heads only");
    // style regions in force: what their heads need under the new flags, now - a failed allocation leaves the plan as it was
    int kinds[16] = {};
    for (int j = 0; j < p->n_style; ++j) kinds[j] = fl[j] ? 2 : p->style_kind[j];
    if (ensure_region_heads(p, p->n_regions, p->style_op, p->n_style, kinds)) return 1;
    std::copy(fl, fl + 16, p->style_diag);
    // a target is kept in the form its head reads - (mu_t, sigma_t), or a root: every target set before is gone
    drop_targets(p);
    return 0;
}

int st_plan_w2_diagonal(const st_plan* p, int* flags) {
    ST_REQUIRE(p && flags, "st_plan_w2_diagonal: null argument");
    for (int j = 0; j < p->n_style; ++j) flags[j] = p->style_diag[j];
    return 0;
}

int st_plan_set_w2_marginal(st_plan* p, const int* flags) {
    ST_REQUIRE(p, "st_plan_set_w2_marginal: null plan");
    int fl[16] = {};
    bool any = false;
    for (int j = 0; flags && j < p->n_style; ++j) {
        ST_REQUIRE(flags[j] == 0 || flags[j] == 1, "st_plan_set_w2_marginal: flag %d of style layer %d: 0 or 1", flags[j], j);
        ST_REQUIRE(flags[j] == 0 || p->style_kind[j] == 0,
                   "st_plan_set_w2_marginal: style layer %d is of kind gram (StyleLoss): only a w2 layer can be matched on its marginals", j);
        ST_REQUIRE(flags[j] == 0 || !p->style_diag[j],
                   "st_plan_set_w2_marginal: style layer %d is flagged diagonal (st_plan_set_w2_diagonal): a layer takes one of the two", j);
        ST_REQUIRE(flags[j] == 0 || p->style_eps[j] < 0.f,
                   "st_plan_set_w2_marginal: style layer %d has a custom eps (st_plan_set_loss_eps); the marginal term has no eps", j);
        ST_REQUIRE(flags[j] == 0 || !p->style_near[j],
                   "st_plan_set_w2_marginal: style layer %d is flagged nearest (st_plan_set_style_nearest): a layer takes one of the two", j);
        ST_REQUIRE(flags[j] == 0 || !p->style_sliced[j],
                   "st_plan_set_w2_marginal: style layer %d is flagged sliced (st_plan_set_style_sliced): a layer takes one of the two", j);
        fl[j] = flags[j];
        any = any || fl[j] != 0;
    }
    ST_REQUIRE(!p->strip || !any, "st_plan_set_w2_marginal: strip plans run full W2 heads only");
    ST_REQUIRE(!any || (!p->style_mask && !p->n_regions),
               "st_plan_set_w2_marginal: a style mask or style regions are in force on this plan; weighted quantiles are not implemented - "
               "clear them first");
    std::copy(fl, fl + 16, p->style_marg);
    // a target is kept in the form its head reads - quantile functions, or a root: every target set before is gone
    drop_targets(p);
    return 0;
}

int st_plan_w2_marginal(const st_plan* p, int* flags) {
    ST_REQUIRE(p && flags, "st_plan_w2_marginal: null argument");
    for (int j = 0; j < p->n_style; ++j) flags[j] = p->style_marg[j];
    return 0;
}

int st_plan_set_style_nearest(st_plan* p, const int* flags) {
    ST_REQUIRE(p, "st_plan_set_style_nearest: null plan");
    int fl[16] = {};
    bool any = false;
    for (int j = 0; flags && j < p->n_style; ++j) {
        ST_REQUIRE(flags[j] == 0 || flags[j] == 1, "st_plan_set_style_nearest: flag %d of style layer %d: 0 or 1", flags[j], j);
        ST_REQUIRE(flags[j] == 0 || p->style_kind[j] == 0,
                   "st_plan_set_style_nearest: style layer %d is of kind gram (StyleLoss): only a w2 layer can be matched on nearest vectors", j);
        ST_REQUIRE(flags[j] == 0 || !p->style_diag[j],
                   "st_plan_set_style_nearest: style layer %d is flagged diagonal (st_plan_set_w2_diagonal): a layer takes one of the two", j);
        ST_REQUIRE(flags[j] == 0 || !p->style_marg[j],
                   "st_plan_set_style_nearest: style layer %d is flagged marginal (st_plan_set_w2_marginal): a layer takes one of the two", j);
        ST_REQUIRE(flags[j] == 0 || !p->style_sliced[j],
                   "st_plan_set_style_nearest: style layer %d is flagged sliced (st_plan_set_style_sliced): a layer takes one of the two", j);
        ST_REQUIRE(flags[j] == 0 || p->style_eps[j] < 0.f,
                   "st_plan_set_style_nearest: style layer %d has a custom eps (st_plan_set_loss_eps); the nearest term has no eps", j);
        ST_REQUIRE(flags[j] == 0 || p->head[p->style_op[j]].n % kNearestChunk == 0,
                   "st_plan_set_style_nearest: style layer %d has %d channels: a multiple of %d", j, p->head[p->style_op[j]].n, kNearestChunk);
        fl[j] = flags[j];
        any = any || fl[j] != 0;
    }
    ST_REQUIRE(!p->strip || !any, "st_plan_set_style_nearest: strip plans run full W2 heads only");
    ST_REQUIRE(!any || (!p->style_mask && !p->n_regions),
               "st_plan_set_style_nearest: a style mask or style regions are in force on this plan; masked matching is not implemented - "
               "clear them first");
    std::copy(fl, fl + 16, p->style_near);
    std::fill(p->style_near_metric, p->style_near_metric + 16, 0);      // l2 until st_plan_set_nearest_metric says otherwise
    // a target is kept in the form its head reads - a set of style vectors, or a root: every target set before is gone
    drop_targets(p);
    return 0;
}

int st_plan_style_nearest(const st_plan* p, int* flags) {
    ST_REQUIRE(p && flags, "st_plan_style_nearest: null argument");
    for (int j = 0; j < p->n_style; ++j) flags[j] = p->style_near[j];
    return 0;
}

int st_plan_set_nearest_metric(st_plan* p, const int* metrics) {
    ST_REQUIRE(p, "st_plan_set_nearest_metric: null plan");
    int mt[16] = {};
    for (int j = 0; metrics && j < p->n_style; ++j) {
        ST_REQUIRE(metrics[j] >= 0 && metrics[j] <= 2,
                   "st_plan_set_nearest_metric: metric %d of style layer %d: 0 (l2), 1 (cosine) or 2 (centered_cosine)", metrics[j], j);
        ST_REQUIRE(metrics[j] == 0 || p->style_near[j],
                   "st_plan_set_nearest_metric: style layer %d is not flagged nearest (st_plan_set_style_nearest): only a flagged layer "
                   "takes a metric", j);
        mt[j] = metrics[j];
    }
    std::copy(mt, mt + 16, p->style_near_metric);
    // a style set is kept as its metric's search reads it - unit rows and a centre, or S^T: every target set before is gone
    drop_targets(p);
    return 0;
}

int st_plan_nearest_metric(const st_plan* p, int* metrics) {
    ST_REQUIRE(p && metrics, "st_plan_nearest_metric: null argument");
    for (int j = 0; j < p->n_style; ++j) metrics[j] = p->style_near_metric[j];
    return 0;
}

int st_plan_set_style_sliced(st_plan* p, const int* flags) {
    ST_REQUIRE(p, "st_plan_set_style_sliced: null plan");
    int fl[16] = {};
    bool any = false;
    for (int j = 0; flags && j < p->n_style; ++j) {
        ST_REQUIRE(flags[j] == 0 || flags[j] == 1, "st_plan_set_style_sliced: flag %d of style layer %d: 0 or 1", flags[j], j);
        ST_REQUIRE(flags[j] == 0 || p->style_kind[j] == 0,
                   "st_plan_set_style_sliced: style layer %d is of kind gram (StyleLoss): only a w2 layer can be matched on sliced projections", j);
        ST_REQUIRE(flags[j] == 0 || !p->style_diag[j],
                   "st_plan_set_style_sliced: style layer %d is flagged diagonal (st_plan_set_w2_diagonal): a layer takes one of the two", j);
        ST_REQUIRE(flags[j] == 0 || !p->style_marg[j],
                   "st_plan_set_style_sliced: style layer %d is flagged marginal (st_plan_set_w2_marginal): a layer takes one of the two", j);
        ST_REQUIRE(flags[j] == 0 || !p->style_near[j],
                   "st_plan_set_style_sliced: style layer %d is flagged nearest (st_plan_set_style_nearest): a layer takes one of the two", j);
        ST_REQUIRE(flags[j] == 0 || p->style_eps[j] < 0.f,
                   "st_plan_set_style_sliced: style layer %d has a custom eps (st_plan_set_loss_eps); the sliced term has no eps", j);
        ST_REQUIRE(flags[j] == 0 || p->head[p->style_op[j]].n % 64 == 0,
                   "st_plan_set_style_sliced: style layer %d has %d channels: a multiple of 64", j, p->head[p->style_op[j]].n);
        fl[j] = flags[j];
        any = any || fl[j] != 0;
    }
    ST_REQUIRE(!p->strip || !any, "st_plan_set_style_sliced: strip plans run full W2 heads only");
    ST_REQUIRE(!any || (!p->style_mask && !p->n_regions),
               "st_plan_set_style_sliced: a style mask (st_plan_set_style_mask) or style regions (st_plan_set_style_regions) are in force "
               "on this plan; weighted quantiles are not implemented - clear them first");
    std::copy(fl, fl + 16, p->style_sliced);
    // the options return to their defaults - C projections, new directions at every closure - and the epoch to 0
    for (int j = 0; j < 16; ++j) {
        p->sliced_proj[j] = 0;
        p->sliced_resample[j] = fl[j];
    }
    p->sliced_epoch = 0;
    // a target is kept in the form its head reads - stored style vectors, or a root: every target set before is gone
    drop_targets(p);
    return 0;
}

int st_plan_style_sliced(const st_plan* p, int* flags) {
    ST_REQUIRE(p && flags, "st_plan_style_sliced: null argument");
    for (int j = 0; j < p->n_style; ++j) flags[j] = p->style_sliced[j];
    return 0;
}

int st_plan_set_sliced_options(st_plan* p, int index, int projections, int resample) {
    ST_REQUIRE(p, "st_plan_set_sliced_options: null plan");
    ST_REQUIRE(index >= 0 && index < p->n_style, "st_plan_set_sliced_options: index %d out of range (%d style layers)", index, p->n_style);
    ST_REQUIRE(p->style_sliced[index], "st_plan_set_sliced_options: style layer %d is not flagged sliced (st_plan_set_style_sliced)", index);
    ST_REQUIRE(projections == 0 || (projections >= 64 && projections <= 512 && projections % 64 == 0),
               "st_plan_set_sliced_options: %d projections: 0 (the tap's channels) or a multiple of 64 in [64, 512]", projections);
    ST_REQUIRE(resample == 0 || resample == 1, "st_plan_set_sliced_options: resample %d: 0 or 1", resample);
    p->sliced_proj[index] = projections;
    p->sliced_resample[index] = resample;
    p->head[p->style_op[index]].target_set = false;     // T is [P][N] for the former P, derived under the former rule
    invalidate_graph(p);
    return 0;
}

int st_plan_set_sliced_seed(st_plan* p, unsigned long long seed) {
    ST_REQUIRE(p, "st_plan_set_sliced_seed: null plan");
    p->sliced_seed = seed;
    p->sliced_epoch = 0;
    // directions and targets drawn under the former seed are gone: set the seed before the style vectors
    for (int j = 0; j < p->n_style; ++j)
        if (p->style_sliced[j]) p->head[p->style_op[j]].target_set = false;
    return 0;
}

int st_plan_loss_eps(const st_plan* p, float* content_eps, float* style_eps) {
    ST_REQUIRE(p, "st_plan_loss_eps: null plan");
    for (int i = 0; content_eps && i < p->n_content; ++i) content_eps[i] = content_eps_of(p, i);
    for (int j = 0; style_eps && j < p->n_style; ++j) style_eps[j] = style_eps_of(p, j);
    return 0;
}

int st_plan_set_tap_weights(st_plan* p, const float* content_weights, const float* style_weights, float tv_weight) {
    ST_REQUIRE(p, "st_plan_set_tap_weights: null plan");
    ST_REQUIRE((p->n_content == 0 || content_weights) && (p->n_style == 0 || style_weights), "st_plan_set_tap_weights: null list");
    for (int i = 0; i < p->n_content; ++i) p->content_weight[i] = content_weights[i];
    for (int j = 0; j < p->n_style; ++j) p->style_weight[j] = style_weights[j];
    p->tv_weight = tv_weight;
    invalidate_graph(p);       // the weights are baked into kernel arguments
    p->phases.clear();         // (a strip's phase sequence is rebuilt by its next closure)
    return 0;
}

int st_plan_set_content_target_at(st_plan* p, int index, const float* feat, void* stream) {
    ST_REQUIRE(p && feat, "st_plan_set_content_target_at: null argument");
    ST_REQUIRE(index >= 0 && index < p->n_content, "st_plan_set_content_target_at: index %d out of range (%d content layers)", index,
               p->n_content);
    const int op = p->content_op[index];
    ST_HIP(hipMemcpyAsync(p->content_target[op], feat, node_at(p, op).count() * sizeof(float), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    p->content_set[op] = true;     // (buffer contents only: a captured graph stays valid)
    return 0;
}

int st_plan_term_losses(st_plan* p, float** terms, int* count) {
    ST_REQUIRE(p && terms && count, "st_plan_term_losses: null argument");
    if (p->reference_taps) {
        *terms = p->losses;
        *count = 7;
        return 0;
    }
    if (ensure_tap_buffers(p)) return 1;
    *terms = p->terms;
    *count = p->n_content + p->n_style + 1;
    return 0;
}

}  // extern "C"
