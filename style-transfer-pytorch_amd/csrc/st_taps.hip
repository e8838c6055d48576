// Configured taps (st_plan_set_taps): the reference's content_layers / style_layers / style_weights (style_transfer.py:315-322,
// read by every scale at :425-453) on any of the trunk's 17 taps, and the GENERAL closure that serves them.
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
#include <algorithm>

#include "st_plan.h"

namespace st {

namespace {
Node& node_at(st_plan* p, int op) { return kProgram[op].kind == 0 ? p->conv[kProgram[op].index] : p->pool[kProgram[op].index]; }
const int kDefaultStyleOp[5] = {0, 3, 6, 11, 16};
constexpr int kDefaultContentOp = 12;
}  // namespace

int tap_position(int layer) {
    for (int i = 0; i < kNumOps; ++i)
        if (kProgram[i].feat_index == layer) return i;
    return -1;
}

bool general_taps(const st_plan* p) {
    static Option force("ST_GENERAL_TAPS", 0);
    return !p->strip && (!p->taps_default || force.get() != 0);
}

int closure_top_op(const st_plan* p) {
    if (!general_taps(p)) return kNumOps - 1;
    int top = 0;
    for (int i = 0; i < p->n_content; ++i) top = std::max(top, p->content_op[i]);
    for (int i = 0; i < p->n_style; ++i) top = std::max(top, p->style_op[i]);
    return top;
}

bool targets_ready(const st_plan* p) {
    if (p->taps_default) {
        bool ok = p->content_set;
        for (int i = 0; i < 5; ++i) ok = ok && p->style[i].target_set;
        return ok;
    }
    bool ok = true;
    for (int i = 0; i < p->n_content; ++i) ok = ok && p->tap_content_set[p->content_op[i]];
    for (int i = 0; i < p->n_style; ++i) ok = ok && p->tap_head[p->style_op[i]].target_set;
    return ok;
}

// the W2 head of a position that is not one of the default closure's five (shapes from the node; buffers when first needed).
// Bound words: st_plan_set_taps gives the j-th listed head word 48 + j and parks every unlisted one on word 63, which a
// listed head owns only in a list of 16.  A parked head commits no bound (st_plan_moments reads the tap's, not the head's),
// so nothing aliases today; heads that move to side streams must keep it that way.
StyleHead& tap_head_at(st_plan* p, int op) {
    StyleHead& h = p->tap_head[op];
    if (h.n == 0) {
        const Node& tap = node_at(p, op);
        h.n = tap.c;
        h.npix = (long long)tap.hg * tap.w;
        h.npix_local = (long long)tap.h * tap.w;
        h.s_amax = reinterpret_cast<unsigned int*>(p->amax_word) + (size_t)(48 + 15) * kAmaxWordUints;
    }
    return h;
}

namespace {

StyleHead& configured_head(st_plan* p, int j) { return p->taps_default ? p->style[j] : tap_head_at(p, p->style_op[j]); }

// seed buffers of the tapped positions and the terms' array
int ensure_tap_buffers(st_plan* p) {
    if (!p->terms) {
        if (plan_alloc(p, &p->terms, 64)) return 1;
        ST_HIP(hipMemset(p->terms, 0, 64 * sizeof(float)));
    }
    auto seed = [&](int op) { return p->tap_seed[op] ? 0 : plan_alloc(p, &p->tap_seed[op], node_at(p, op).count()); };
    for (int i = 0; i < p->n_content; ++i)
        if (seed(p->content_op[i])) return 1;
    for (int i = 0; i < p->n_style; ++i)
        if (seed(p->style_op[i])) return 1;
    return 0;
}

}  // namespace

int general_loss_and_grad(st_plan* p, const float* image, float* grad_out, float* losses_out, hipStream_t s) {
    if (require_targets(p) || ensure_grad_alloc(p) || ensure_streams(p, s) || ensure_tap_buffers(p)) return 1;
    const int nc = p->n_content, ns = p->n_style;
    // the reference's configuration (ST_GENERAL_TAPS): the 8-float array IS the terms in SumLoss order
    float* terms = p->taps_default ? p->losses : p->terms;
    // TVLoss on the un-normalised image (style_transfer.py:376): WRITES grad_out; conv1_1's data gradient adds to it
    if (hbm_profiled(p, HBM_TV, 2.0 * 3 * 4.0 * p->H * p->W, s, [&] {
            return launch_tv(image, p->H, p->W, p->tv_weight, grad_out, p->red_partials, terms + nc + ns, s, p->tickets + 0);
        }))
        return 1;
    const int top = closure_top_op(p);
    if (run_forward(p, image, kProgram[top].feat_index, s, /*fork_heads=*/false)) return 1;
    // style heads, deepest first (the deepest one's gradient is what the backward starts from)
    int order[16];
    for (int j = 0; j < ns; ++j) order[j] = j;
    std::sort(order, order + ns, [&](int a, int b) { return p->style_op[a] > p->style_op[b]; });
    bool styled[kNumOps] = {};
    for (int k = 0; k < ns; ++k) {
        const int j = order[k], op = p->style_op[j];
        HeadSite at;
        at.h = &configured_head(p, j);
        at.tap = &node_at(p, op);
        at.weight = p->taps_default ? p->style_weight[j] : p->tap_style_weight[j];
        at.loss = terms + nc + j;
        at.grad = p->tap_seed[op];
        if (style_head(p, at, s)) return 1;
        styled[op] = true;
    }
    // ContentLossMSE per content layer (style_transfer.py:425-429), behind the style head of the same layer where there is one
    for (int i = 0; i < nc; ++i) {
        const int op = p->content_op[i];
        const Node& ct = node_at(p, op);
        const float* target = p->taps_default ? p->content_target : p->tap_content_target[op];
        const float weight = p->taps_default ? p->content_weight : p->tap_content_weight[i];
        if (hbm_profiled(p, HBM_CONTENT, 3.0 * 4.0 * ct.count(), s, [&] {
                return launch_content_mse(ct.y, target, (long long)ct.count(), weight, p->tap_seed[op],
                                          p->red_partials + 4 * kStreamBlocks, terms + i, s, p->tickets + 64, styled[op] ? 1 : 0);
            }))
            return 1;
    }
    if (p->taps_default) {
        if (!p->defer_sum && launch_sum_losses(p->losses, s, losses_out)) return 1;
    } else if (launch_sum_terms(terms, nc, ns, p->losses, s, p->defer_sum ? nullptr : losses_out)) {
        // (a step's tail sums the 8-float array once more - the same additions - and fills losses_out)
        return 1;
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
    bool dflt = n_content == 1 && cop[0] == kDefaultContentOp && n_style == 5;
    for (int i = 0; dflt && i < 5; ++i) dflt = sop[i] == kDefaultStyleOp[i];
    if (!dflt) {
        // everything the configuration needs, now: a failed allocation leaves the plan as it was
        for (int i = 0; i < n_content; ++i)
            if (!p->tap_content_target[cop[i]] && plan_alloc(p, &p->tap_content_target[cop[i]], node_at(p, cop[i]).count())) return 1;
        for (int j = 0; j < n_style; ++j)
            if (ensure_style_alloc(p, tap_head_at(p, sop[j]))) return 1;
    }
    p->taps_default = dflt;
    p->n_content = n_content;
    p->n_style = n_style;
    for (int i = 0; i < 16; ++i) {
        p->content_op[i] = i < n_content ? cop[i] : 0;
        p->style_op[i] = i < n_style ? sop[i] : 0;
        // (the reference's content_weight split over the layers, :366; its style weights belong to its own five layers)
        p->tap_content_weight[i] = i < n_content ? 0.015f / (float)n_content : 0.f;
        p->tap_style_weight[i] = i < n_style ? 1.f / (float)n_style : 0.f;
    }
    for (StyleHead& h : p->tap_head)                 // (unlisted heads, a former list's included: parked - see tap_head_at)
        h.s_amax = reinterpret_cast<unsigned int*>(p->amax_word) + (size_t)(48 + 15) * kAmaxWordUints;
    if (!dflt)
        for (int j = 0; j < n_style; ++j)
            p->tap_head[sop[j]].s_amax = reinterpret_cast<unsigned int*>(p->amax_word) + (size_t)(48 + j) * kAmaxWordUints;
    // every target set before is gone
    p->content_set = false;
    for (StyleHead& h : p->style) h.target_set = false;
    for (int i = 0; i < kNumOps; ++i) {
        p->tap_head[i].target_set = false;
        p->tap_content_set[i] = false;
    }
    invalidate_graph(p);
    return 0;
}

int st_plan_set_tap_weights(st_plan* p, const float* content_weights, const float* style_weights, float tv_weight) {
    ST_REQUIRE(p, "st_plan_set_tap_weights: null plan");
    ST_REQUIRE((p->n_content == 0 || content_weights) && (p->n_style == 0 || style_weights), "st_plan_set_tap_weights: null list");
    for (int i = 0; i < p->n_content; ++i) p->tap_content_weight[i] = content_weights[i];
    for (int j = 0; j < p->n_style; ++j) p->tap_style_weight[j] = style_weights[j];
    if (p->taps_default) {
        p->content_weight = content_weights[0];
        for (int j = 0; j < 5; ++j) p->style_weight[j] = style_weights[j];
    }
    p->tv_weight = tv_weight;
    invalidate_graph(p);       // the weights are baked into kernel arguments
    p->phases.clear();
    return 0;
}

int st_plan_set_content_target_at(st_plan* p, int index, const float* feat, void* stream) {
    ST_REQUIRE(p && feat, "st_plan_set_content_target_at: null argument");
    ST_REQUIRE(index >= 0 && index < p->n_content, "st_plan_set_content_target_at: index %d out of range (%d content layers)", index,
               p->n_content);
    const int op = p->content_op[index];
    float* dst = p->taps_default ? p->content_target : p->tap_content_target[op];
    ST_HIP(hipMemcpyAsync(dst, feat, node_at(p, op).count() * sizeof(float), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    if (p->taps_default) p->content_set = true;     // (buffer contents only: a captured graph stays valid)
    else p->tap_content_set[op] = true;
    return 0;
}

int st_plan_term_losses(st_plan* p, float** terms, int* count) {
    ST_REQUIRE(p && terms && count, "st_plan_term_losses: null argument");
    if (p->taps_default) {
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
