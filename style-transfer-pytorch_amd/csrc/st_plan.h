// Internal to libst_amd.so: the VGG-19 program, the plan's nodes and head sites, st_net / st_plan, and the plan helpers
// that more than one of st_api.hip, st_closure.hip, st_taps.hip, st_mask.hip, st_laplacian.hip, st_strip.hip and
// st_range_guard.hip call.
// (StyleHead and a head's launch sequence: st_head_core.h, shared with st_head.hip; the wrappers below add the plan's part.)
#pragma once

#include <functional>
#include <unordered_map>
#include <vector>

#include "../../include/st_amd.h"
#include "st_common.h"
#include "st_head_core.h"

namespace st {

// torchvision vgg19 cfg "E" truncated at features[29] (reference style_transfer.py:35)
struct OpDesc {
    int kind;        // 0 = conv(+ReLU), 1 = pool
    int index;       // conv number 0..12 or pool number 0..3
    int feat_index;  // features[] index of the produced tap (the ReLU for convs, the pool itself)
    int cin, cout;
};
const OpDesc kProgram[] = {
    {0, 0, 1, 3, 64},     {0, 1, 3, 64, 64},    {1, 0, 4, 64, 64},    {0, 2, 6, 64, 128},
    {0, 3, 8, 128, 128},  {1, 1, 9, 128, 128},  {0, 4, 11, 128, 256}, {0, 5, 13, 256, 256},
    {0, 6, 15, 256, 256}, {0, 7, 17, 256, 256}, {1, 2, 18, 256, 256}, {0, 8, 20, 256, 512},
    {0, 9, 22, 512, 512}, {0, 10, 24, 512, 512}, {0, 11, 26, 512, 512}, {1, 3, 27, 512, 512},
    {0, 12, 29, 512, 512},
};
constexpr int kNumOps = sizeof(kProgram) / sizeof(kProgram[0]);
constexpr float kCovEps = 1e-4f;                  // StyleLossW2 eps (style_transfer.py:152)

struct Node {
    float* y = nullptr;   // activation (post-ReLU conv output or pooled map) [c][h][w]
    float* g = nullptr;   // gradient w.r.t. y, same shape (allocated lazily)
    float* yhalo = nullptr;   // strip mode: [2][c][w] rows of the neighbours (only if a conv reads this node)
    float* ghalo = nullptr;   // strip mode: [2][c][w] masked gradient rows of the neighbours (conv outputs)
    int c = 0, h = 0, w = 0;
    int hg = 0;               // global height at this level (== h when not sharded)
    bool pooled_by_conv = false;   // forward, strip plans: this conv's epilogue wrote the following max pool
    unsigned char* pool_code = nullptr;   // conv feeding a max pool: argmax + mask codes of the pooled windows (closure only)
    bool coded = false;            // this pass wrote pool_code INSTEAD of y (ConvProblem::pool_code)
    // device words (raw float bits) bounding max |y| / max |g| for the fp16x3 convolutions' scales: written by
    // the kernels that finalise y / g (amax_commit), zeroed at the start of every forward.  Pooled maps reuse
    // their input's y word, and a conv feeding a pool reuses the pool's g word (see scale_exp's spare bit).
    unsigned int* y_amax = nullptr;
    unsigned int* g_amax = nullptr;
    size_t count() const { return (size_t)c * h * w; }
};

// Where a W2 style head sits: head_site(p, j) for the j-th LISTED style layer in the default and strip closures, the same
// with the seed buffer as destination in the general closure (st_taps.hip), by hand for an unlisted position (st_plan_moments).
struct HeadSite {
    StyleHead* h = nullptr;
    const Node* tap = nullptr;       // the tap's node (a conv's ReLU output or a pooled map)
    float weight = 0.f;
    float eps = kCovEps;             // the entry's eps (style_eps_of): W2's covariance eps, a Gram head's ScaledMSELoss eps
    float* loss = nullptr;           // device word of the weighted loss term
    float* grad = nullptr;           // dF is WRITTEN here: the tap's gradient buffer, or its seed buffer (general closure)
    unsigned int* grad_amax = nullptr;   // fp16x3: bound of what is written (null: whoever consumes it next commits one)
    int slot = -1;                   // 0 .. 4: the default closure's head of that index (relu1_1's fused Gram, relu5_1's mask,
                                     // the timeline events, the persistent chain's mask); -1: none of these
    const float* sqrt_mask = nullptr;    // a style mask is in force (st_plan::style_mask): sqrt of it at the tap's level ...
    float mask_sum = 0.f;                // ... and that level's sum, the moments' and the gradient step's normaliser (mask_head_site)
};

struct ProfileEvent {
    hipEvent_t start, stop;
    double flops;
};

// HBM-bound kernels of the step, timed like the conv launches when profiling is on (bench.py `roofline_hbm`):
// category, algorithmic bytes of the launch (operands read once + results written once)
enum HbmCat { HBM_CONV1_FWD = 0, HBM_CONV1_DGRAD, HBM_POOL_BWD, HBM_ADAM, HBM_TV, HBM_GRAM1, HBM_CONTENT, HBM_HEAD_1X1, HBM_CATS };
struct HbmEvent {
    hipEvent_t start, stop;
    int cat;
    double bytes;
};

}  // namespace st

struct st_net {
    int pooling = 0;
    float* w_first = nullptr;        // conv1_1 weight, torch layout [64][3][3][3]
    float w_first_l1max = 0.f;       // max over output channels of sum |w|, and max |bias|: the a-priori bound of relu1_1 per
    float b_first_max = 0.f;         // pixel block that the fused conv1_1 + Gram kernel scales its fp16 planes by
    float* bias[13] = {};
    float* w_fwd[13] = {};           // [9][Cin][Cout]   (convs 1..12)
    float* w_bwd[13] = {};           // [9][Cout][Cin], taps rotated (convs 1..12)
    int conv_planes = 0;             // 0: fp32 MFMA; 2 / 3 planes: split-precision convolutions (st_common.h)
    int conv_elem = 0;               // plane element type: 0 bf16, 1 fp16 (fp16x3)
    void* ws_fwd[13] = {};           // bf16 planes of the forward weights (convs 1..12)
    void* ws_bwd[13] = {};           // bf16 planes of the data-gradient weights
    // fp16x3 networks, dynamic-range guard: a convolution whose weights carry a channel far above the layer's median
    // (the signature of weights that compensate a tiny-valued operand channel) runs in bf16x6 instead - three bf16
    // planes, 8-bit exponents, no per-tensor scale to fall out of (see range_guard in net_fill)
    int wide_fwd[13] = {};           // 1: this layer's forward runs bf16x6
    int wide_bwd[13] = {};           // 1: its data gradient does
    void* wsx_fwd[13] = {};          // bf16x6 planes of the flagged layers
    void* wsx_bwd[13] = {};
    float* w_torch[13] = {};         // the weights as given ([Cout][Cin][3][3]): source of planes built after creation, when
                                     // the activation-aware guard (st_plan_range_guard) flags a layer
    int guard_fwd[13] = {};          // 1: flagged by the activation-aware guard (subset of wide_*)
    int guard_bwd[13] = {};
};

struct st_plan {
    const st_net* net = nullptr;
    int H = 0, W = 0;
    st::Node conv[13];
    st::Node pool[4];
    bool grads_allocated = false;
    int fwd_last_layer = 0;          // st_plan_forward's last_layer while the maps it wrote are current (st_plan_backward's
                                     // operands); 0: none has run, or a closure has since (argmax codes instead of maps)
    // The loss terms, ONE description for every configuration: the content / style lists as kProgram positions with a weight
    // per LISTED entry, and the W2 head, content target and seed buffer of a position, indexed by kProgram position.
    // st_plan_set_taps replaces the lists; a head or target buffer serves whichever configuration names its position.
    // reference_taps: the lists are the reference's own ([22], [1, 6, 11, 20, 29], style_transfer.py:315-322).  It selects
    // WHICH closure runs - loss_and_grad (st_closure.hip) for them under the default loss kinds, general_loss_and_grad
    // (st_taps.hip) for every other configuration (general_taps) - and what follows from the LISTS: the terms array and its
    // sum kernel (loss_terms, st_plan_term_losses), st_plan_set_loss_weights' refusal, and conv1_1's fused Gram with the one
    // consumer of its partials outside the closure (run_forward, st_plan_moments).  Never which state is read.
    bool reference_taps = true;
    int n_content = 1, n_style = 5;
    int content_op[16] = {12};
    int style_op[16] = {0, 3, 6, 11, 16};
    float content_weight[16] = {0.015f};             // per LISTED entry
    float style_weight[16] = {256.f / 341, 64.f / 341, 16.f / 341, 4.f / 341, 1.f / 341};
    float tv_weight = 2.0f;
    // WHAT the terms are, one kind per LISTED entry (st_plan_set_loss_kinds for a whole list, st_plan_set_layer_loss_kinds per
    // entry): content 0 = ContentLossMSE, 1 = ContentLoss (the features under ScaledMSELoss); style 0 = StyleLossW2,
    // 1 = StyleLoss (the Gram matrix under ScaledMSELoss).  And the entry's eps (st_plan_set_loss_eps): negative = the kind's
    // default (kCovEps for w2, kScaledMseEps for gram and scaled_mse; mse has none), which is also what a value equal to the
    // default is stored as.  Any non-default kind or eps runs the general closure (general_taps), on the reference's lists too.
    int content_kind[16] = {}, style_kind[16] = {};
    float content_eps[16] = {-1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f};
    float style_eps[16] = {-1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f};
    // A W2 entry whose covariances are restricted to their diagonals (st_plan_set_w2_diagonal, st_w2diag.hip): a flag per LISTED
    // style entry, 0 on every Gram entry.  Any set flag runs the general closure (general_taps), on the reference's lists too;
    // either kinds setter and st_plan_set_taps clear them.
    int style_diag[16] = {};
    // A W2 entry matched on its exact per-channel marginals (st_plan_set_w2_marginal, st_sort.hip): a flag per LISTED style entry,
    // never together with style_diag, a custom eps, a style mask or regions.  Any set flag runs the general closure; either kinds
    // setter and st_plan_set_taps clear them.
    int style_marg[16] = {};
    // A W2 entry matched on nearest style vectors (st_plan_set_style_nearest, st_nearest.hip): a flag per LISTED style entry, never
    // together with style_diag, style_marg, a custom eps, a style mask or regions.  Any set flag runs the general closure; either
    // kinds setter and st_plan_set_taps clear them.
    int style_near[16] = {};
    // ... and what a flagged entry is matched on (st_plan_set_nearest_metric): 0 l2, 1 cosine, 2 centred cosine.  Non-zero only on
    // a flagged entry; st_plan_set_style_nearest, either kinds setter and st_plan_set_taps reset them to 0.
    int style_near_metric[16] = {};
    // A W2 entry matched on sliced projections (st_plan_set_style_sliced, st_sliced.hip): a flag per LISTED style entry, never
    // together with style_diag, style_marg, style_near, a custom eps, a style mask or regions.  Any set flag runs the general
    // closure; either kinds setter and st_plan_set_taps clear them.  Per flagged entry: the number of projections (0: the tap's
    // channels) and whether every closure draws new directions (st_plan_set_sliced_options).  sliced_epoch is the epoch the
    // NEXT general closure draws its directions at: a host counter, handed to the direction kernel as an argument - the general
    // closure is never captured into a graph - and advanced once per closure while any flagged entry resamples.
    int style_sliced[16] = {};
    int sliced_proj[16] = {};
    int sliced_resample[16] = {};
    unsigned long long sliced_seed = 0, sliced_epoch = 0;
    float* kind_scratch = nullptr;                   // non-default kinds: [2 kStreamBlocks] per-block (sum d^2, sum |d|) of the
                                                     // term in flight, then [2] per term: sum d^2, sum |d| + eps (kind_totals)
    st::StyleHead head[st::kNumOps];                 // n / npix / npix_local of all 17 filled at create, buffers on first use;
                                                     // bound word: the j-th listed head owns word 48 + j, an unlisted one is parked on 63
    float* content_target[st::kNumOps] = {};         // allocated when a list first names the position ([12] at create)
    bool content_set[st::kNumOps] = {};
    float* tap_seed[st::kNumOps] = {};               // general closure: the heads' gradient of a tapped position, run_tap_backward's seed
    float* terms = nullptr;                          // general closure on other lists than the reference's: [64], at most 16 + 16 + 1
                                                     // used - the weighted terms in SumLoss order (st_plan_term_losses)
    // Spatial style mask (st_plan_set_style_mask, st_mask.hip): while style_mask is set every style head takes WEIGHTED moments
    // of its tap - the mask at the tap's level (the number of pools at or before it), as its square root, which the Gram
    // kernels put on both operands - and multiplies its gradient's pixel columns by the mask.  The general closure runs then
    // (general_taps), on the reference's configuration too.  The sums are read back once, by the setter.
    bool style_mask = false;
    float* mask_sqrt[st::kMaskLevels] = {};          // [h][w] of mask_h / mask_w, allocated by the first setter call
    int mask_h[st::kMaskLevels] = {}, mask_w[st::kMaskLevels] = {};
    double mask_sum[st::kMaskLevels] = {};
    double* mask_stats = nullptr;                    // the pyramid kernel's partials and, behind them, its 8 results per region
    // Style regions (st_plan_set_style_regions, st_mask.hip): n_regions masks with a style each, the style mask's formulas once
    // per region.  Region 0's head of a position is head[op]; regions 1 .. R - 1 have heads of their own (targets, workspaces,
    // bound word), allocated for the listed style positions whenever the regions, the lists or the kinds change.  The general
    // closure runs while n_regions > 0 (general_taps); a region's term is weighted style_weight[j] * region_weight[r].
    int n_regions = 0;                               // 0: none in force (then a style mask may be)
    float region_weight[st::kMaxRegions] = {};       // rho_r: 1 / R each from st_plan_set_style_regions, or st_plan_set_region_weights'
    float* region_sqrt[st::kMaxRegions][st::kMaskLevels] = {};   // a pyramid per region (sizes: mask_h / mask_w), on first use
    double region_sum[st::kMaxRegions][st::kMaskLevels] = {};
    st::StyleHead region_head[st::kMaxRegions - 1][st::kNumOps];     // [r - 1][op]
    unsigned int* region_amax = nullptr;             // [(kMaxRegions - 1) * 16] bound words: head (r, j) owns word (r - 1) 16 + j
    float* region_terms = nullptr;                   // [kMaxRegions][16], used [R][n_style]: the weighted terms (st_plan_region_terms)
    float* region_scratch = nullptr;                 // the 1x1 step of a region r >= 1, before it is added onto the seed ...
    size_t region_scratch_floats = 0;                // ... sized by the largest listed style tap
    // Spatial weight maps for the content and TV terms (st_plan_set_content_mask / st_plan_set_tv_mask, st_mask.hip): the
    // content map as the style mask's pyramid of the levels THEMSELVES - a content layer weighs (F - T) per pixel with the
    // level of the pools at or before it -, the TV map at the image's size only, a bit-exact copy.  Either one runs the
    // general closure (general_taps); independent of each other and of style_mask / n_regions.  Sizes: mask_h / mask_w.
    bool content_mask = false, tv_mask = false;
    float* content_map[st::kMaskLevels] = {};        // allocated by the first setter call
    float* tv_map = nullptr;
    // Laplacian loss on pooled images (st_plan_set_laplacian, st_laplacian.hip): n_lap pool sizes, each with its pooled map Q
    // (unused for p = 1), residual r and target T = L(Q(content)), all [3][lap_h][lap_w].  The general closure runs while
    // n_lap > 0 (general_taps) and adds each term onto the image-space slot and its gradient onto the TV gradient, right
    // behind the TV launch.  Independent of the masks, regions and maps.
    int n_lap = 0;                                   // 0: none in force
    int lap_pool[st::kMaxLapPools] = {}, lap_h[st::kMaxLapPools] = {}, lap_w[st::kMaxLapPools] = {};
    float lap_weight = 0.f;
    float* lap_q[st::kMaxLapPools] = {};
    float* lap_r[st::kMaxLapPools] = {};
    float* lap_t[st::kMaxLapPools] = {};
    size_t lap_floats[st::kMaxLapPools] = {};        // what slot k's three buffers hold
    float* lap_partials = nullptr;                   // [kLapBlocks] of the residual pass in flight
    float* lap_terms = nullptr;                      // [0] the TV term alone, [1 + k] pool size k's term (st_plan_laplacian_terms)
    float* grad_img = nullptr;       // [3][H][W] internal gradient for st_plan_step
    float* losses = nullptr;         // [8] device
    float* red_partials = nullptr;   // scratch for two-level reductions: TV [0, 4 kStreamBlocks), content MSE after it
    float* guard_scratch[3] = {nullptr, nullptr, nullptr};      // plan_range_guard: three maps of the largest activation ...
    float* guard_sums = nullptr;                                // ... and range_diff_kernel's per-block partial sums
    unsigned int* tickets = nullptr; // zeroed device words of the "last block finishes the sum" kernels (self-resetting)
    float* conv_scratch = nullptr;   // split-K workspace of the trunk convolutions (main stream only)
    float* dp_scratch = nullptr;     // conv1_1 data gradient on the padded domain, dp_parts x 3 (H + 2) (W + 2)
    int dp_parts = 1;                // channel slices of that kernel (conv_first_dgrad_parts of the GLOBAL shape)
    float* amax_word = nullptr;      // 64 bounds of kAmaxWordUints: Node::y_amax [conv], +16 g_amax [conv], +32 g_amax [pool], +48 StyleHead::s_amax
    long long bytes = 0;
    std::vector<void*> allocations;
    // strip sharding; strip == false -> the plan owns the whole image
    bool strip = false;
    int Hg = 0, row0 = 0, has_up = 0, has_down = 0;
    float* img_halo = nullptr;       // [2][3][W]
    // packed boundary rows, 64 * W floats each + the 16-float trailer whose first word is max |row| as raw bits (kHaloTrailer):
    // send_up = [rows | trailer] (lands as the upper neighbour's BOTTOM halo), send_down = [trailer | rows] (the lower
    // neighbour's TOP halo) - so that a halo block [trailer | top rows | bottom rows | trailer] receives either message contiguously
    float* send_up = nullptr;
    float* send_down = nullptr;
    unsigned int* pack_scratch = nullptr;   // launch_pack_rows' block maxima + ticket
    float* lossbuf = nullptr;        // [0] content sum of squares, [1..4] TV sums (all-reduced)
    float* gram_raw[5] = {};         // per head [C*C + C] raw moment sums (all-reduced); one contiguous block
    long long gram_total = 0;        // floats in that block
    // strip closure, device-ordered exchanges: halo rows travel on comm_stream while the interior rows of the consuming
    // convolution are computed on the caller's stream (pack_done: the boundary rows are packed; halo_landed: the
    // exchange has been enqueued behind it)
    hipStream_t comm_stream = nullptr;
    bool comm_stream_borrowed = false;     // from the process-wide probed set (shared_head_streams)
    hipStream_t chain_stream = nullptr;    // strip plans, compact layout: the owned heads' Newton-Schulz chains (else they run
                                           // on the head's own stream)
    hipEvent_t moments_ready[5] = {}, chain_done[5] = {};
    hipEvent_t pack_done = nullptr, halo_landed = nullptr;
    unsigned int* halo_bound = nullptr;     // operand bound of a boundary launch: the operand's own bound + its halo rows'

    int rank = 0, world = 1;         // position of this strip among the ranks (NS-chain ownership)
    float* head_result[5] = {};      // per head [C*C + C + 64]: Ssym | b | weighted loss term - what the owner broadcasts
    struct Phase {
        std::function<int(hipStream_t)> run;
        st_exchange ex;
        const float* halo = nullptr;         // the halo block a kind-1 exchange fills (finish_phases)
    };
    // halo blocks whose consumer is NOT cut into interior + boundary launches: their exchange is issued on the caller's
    // stream, in line between the pack kernel and the consumer (add_strip_conv, finish_phases)
    std::unordered_map<const float*, bool> halo_inline;
    std::vector<Phase> phases;
    size_t phase_pos = 0;
    const float* ph_image = nullptr;
    float* ph_grad = nullptr;
    int ph_last_layer = -1;
    unsigned ph_option_gen = 0;
    // Side streams: the five W2 style heads are ~60 dependent small launches each (latency bound),
    // so each runs on its own stream, forked when its tap is ready in the forward pass and joined
    // just before the backward pass needs that tap's gradient.  They overlap the trunk and each other.
    hipStream_t head_stream[5] = {};
    bool head_stream_owned[5] = {};        // false: borrowed from the process-wide set (shared_head_streams)
    hipEvent_t tap_ready[5] = {};
    hipEvent_t head_done[5] = {};
    bool streams_ready = false;
    int device = 0;
    // hipGraph replay of the closure.  The ~430 launches of one closure (6 streams) are captured once
    // per (image, grad, losses) pointer triple on an internal stream and replayed; the caller's stream
    // (possibly the legacy null stream, which cannot be captured) is bridged with two events.
    // OFF by default: measured on ROCm 7.2 / MI355X the replay of this 6-branch graph is bit-identical
    // but slower than eager launches (512^2: 5.9 vs 5.0 ms per step, 128^2: 3.1 vs 2.1 ms).
    bool graph_enabled = false;
    hipStream_t main_stream = nullptr;
    bool gram1_fused = false;              // this pass's conv1_1 launch left relu1_1's partial moments (run_forward)
    int gram1_splits = 0;
    bool compact_streams = false;          // ensure_streams: only the streams that carry work exist
    bool head4_on_caller = false;          // relu5_1's head runs on the caller's stream (shared_head_streams found no sharer)
    std::vector<hipStream_t> junk_streams;  // ST_STREAM_DUMMIES (experiments)
    hipEvent_t bridge_in = nullptr, bridge_out = nullptr;
    // TV (needs only the image) and the content MSE run beside the trunk on one auxiliary stream
    hipStream_t aux_stream = nullptr;
    hipEvent_t aux_in = nullptr, aux_fwd = nullptr, tv_done = nullptr, content_done = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    const float* gk_image = nullptr;
    float* gk_grad = nullptr;
    float* gk_losses = nullptr;
    int gk_seen = 0;
    bool capturing = false;
    // ST_AMD_TIMELINE=1: timing events at step start / forward end / each head done / backward end
    bool timeline = false;
    hipEvent_t tl_start = nullptr, tl_fwd = nullptr, tl_head[5] = {}, tl_bwd = nullptr;
    hipEvent_t tl_h4[4] = {};        // relu5_1's head: chain start, after NS forward, after NS backward, (end = tl_head[4])
    hipEvent_t tl_h3[4] = {};        // the same for relu4_1's head
    int tl_count = 0;
    // profiling
    bool profiling = false;
    std::vector<st::ProfileEvent> events;
    size_t events_used = 0;
    std::vector<st::HbmEvent> hbm_events;
    size_t hbm_used = 0;
    long long prof_launches = 0;
    double prof_ms = 0, prof_flops = 0;
    // st_plan_step: the losses' total and the clearing of the fp16x3 operand bounds ride in the update kernel (AdamTail)
    bool defer_sum = false;          // loss_and_grad leaves the total to the caller
    bool amax_clean = false;         // the update kernel has cleared amax_word: the next run_forward skips its memset
    const st::FoldUpdate* fold_update = nullptr;     // st_plan_step: conv1_1's fold kernel applies the update (and the tail)
    bool fold_updated = false;       // ... and has done so in this closure
};

namespace st {

// the node of kProgram[op]
inline Node& node_at(st_plan* p, int op) { return kProgram[op].kind == 0 ? p->conv[kProgram[op].index] : p->pool[kProgram[op].index]; }
inline const Node& node_at(const st_plan* p, int op) { return node_at(const_cast<st_plan*>(p), op); }
// the k-th listed style layer is conv `conv_index`'s ReLU
inline bool head_taps_conv(const st_plan* p, int k, int conv_index) {
    return kProgram[p->style_op[k]].kind == 0 && kProgram[p->style_op[k]].index == conv_index;
}
// The heads' bound words (plan creation, st_plan_set_taps): the j-th listed head owns word 48 + j, and every unlisted head is
// parked on word 63, which a listed one owns only in a list of 16.  A parked head commits no bound (st_plan_moments reads
// the tap's, not the head's), so nothing aliases; heads that move to side streams must keep it that way.
inline void assign_head_bounds(st_plan* p) {
    unsigned int* words = reinterpret_cast<unsigned int*>(p->amax_word);
    for (StyleHead& h : p->head) h.s_amax = words + (size_t)63 * kAmaxWordUints;
    for (int j = 0; j < p->n_style; ++j) p->head[p->style_op[j]].s_amax = words + (size_t)(48 + j) * kAmaxWordUints;
    // the heads of regions 1 .. R - 1 (style regions): words of a block of their own, which the closure clears; an unlisted one has none
    for (int r = 1; r < kMaxRegions; ++r) {
        for (StyleHead& h : p->region_head[r - 1]) h.s_amax = nullptr;
        for (int j = 0; p->region_amax && j < p->n_style; ++j)
            p->region_head[r - 1][p->style_op[j]].s_amax = p->region_amax + (size_t)((r - 1) * 16 + j) * kAmaxWordUints;
    }
}
// region r's head of kProgram[op] (style regions; region 0's is the position's own)
inline StyleHead& region_head_at(st_plan* p, int region, int op) { return region == 0 ? p->head[op] : p->region_head[region - 1][op]; }
inline const StyleHead& region_head_at(const st_plan* p, int region, int op) { return region_head_at(const_cast<st_plan*>(p), region, op); }

constexpr int kHaloTrailer = 16;            // floats; word 0 = the sender's max |row| (raw bits), the rest unused (64-byte alignment)

// ---- st_closure.hip
int plan_alloc(st_plan* p, float** out, size_t floats);
// ... as the heads' allocator (st_head_core.h): a buffer that is there stays, so a call that failed half way can be made again
struct PlanAlloc { st_plan* p; int operator()(float** out, size_t floats) const { return *out ? 0 : plan_alloc(p, out, floats); } };
int conv_launch_profiled(st_plan* p, const ConvProblem& prob, hipStream_t s, double flops_fraction = 1.0);
template <class F>
int hbm_profiled(st_plan* p, int cat, double bytes, hipStream_t s, F&& launch) {
    if (!p->profiling) return launch();
    if (p->hbm_used == p->hbm_events.size()) {
        HbmEvent ev{};
        ST_HIP(hipEventCreate(&ev.start));
        ST_HIP(hipEventCreate(&ev.stop));
        p->hbm_events.push_back(ev);
    }
    HbmEvent& ev = p->hbm_events[p->hbm_used++];
    ev.cat = cat;
    ev.bytes = bytes;
    ST_HIP(hipEventRecord(ev.start, s));
    const int rc = launch();
    ST_HIP(hipEventRecord(ev.stop, s));
    return rc;
}

void invalidate_graph(st_plan* p);
int ensure_streams(st_plan* p, hipStream_t caller = nullptr);
int ensure_moment_alloc(st_plan* p, StyleHead& h);      // what st_plan_moments needs (StyleHead::allocated)
int ensure_style_alloc(st_plan* p, StyleHead& h, int kind);   // ... and what a head of that style kind needs
int ensure_grad_alloc(st_plan* p);
HeadSite head_site(st_plan* p, int j);
void mask_head_site(const st_plan* p, HeadSite& at, int op);   // the style mask's level of kProgram[op], if one is in force
int moments_of_tap(st_plan* p, const HeadSite& at, float* mean_out, float* srm_out, hipStream_t s, float* cov_out = nullptr);
int moment_sums_of_tap(st_plan* p, int j, float* sums, hipStream_t s);
int style_head(st_plan* p, const HeadSite& at, hipStream_t s);
int style_head_chain(st_plan* p, const HeadSite& at, hipStream_t s, bool cov_ready = false);
int style_head_gradient(st_plan* p, const HeadSite& at, hipStream_t s);
int join_head_for_conv(st_plan* p, int conv_index, hipStream_t s);
int require_targets(const st_plan* p);
int run_forward(st_plan* p, const float* image, int last_layer, hipStream_t s, bool fork_heads = false);
int loss_and_grad(st_plan* p, const float* image, float* grad_out, float* losses_out, hipStream_t s);
int closure_entry(st_plan* p, const float* image, float* grad_out, float* losses_out, hipStream_t s);
int closure_eager(st_plan* p, const float* image, float* grad_out, float* losses_out, hipStream_t s);
// the trunk's 3x3 launches, described once for both closures and the range guard (kProgram[i] is a conv, i > 0)
bool pool_follows(const st_plan* p, int i, int last_layer);
void forward_conv(const st_plan* p, int i, ConvProblem& c);
bool fuse_pool(ConvProblem& c, Node& n, bool fork_heads, const PcOverlap* cut);
void dgrad_conv(const st_plan* p, int i, ConvProblem& c);
// st_plan_backward: seed[i] = the external gradient of kProgram[i]'s tap, or null.  onto_image (general closure): grad_image
// holds the TV gradient and is added to, with the step's update folded in where the plan asks for it (st_plan::fold_update).
int run_tap_backward(st_plan* p, const float* const* seed, float* grad_image, hipStream_t s, bool onto_image = false);

// ---- st_taps.hip
bool general_taps(const st_plan* p);
int general_loss_and_grad(st_plan* p, const float* image, float* grad_out, float* losses_out, hipStream_t s);
int tap_position(int layer);          // kProgram position of features[layer], -1: not one of the 17 taps
int closure_top_op(const st_plan* p); // the deepest kProgram position the plan's closure runs
bool targets_ready(const st_plan* p);
float* loss_terms(st_plan* p);        // the array the closure's weighted terms go to, in SumLoss order
int sliced_projections_of(const st_plan* p, int j);      // P of sliced entry j: its option, or the tap's channels
// sliced entry j's directions at `epoch` and, from its stored style vectors, its target (st_plan_set_style_sliced_vectors, and every
// general closure while the entry resamples)
int sliced_refresh(st_plan* p, int j, unsigned long long epoch, hipStream_t s);
float style_eps_of(const st_plan* p, int j);   // effective eps of style entry j / content entry i (mse: -1)
float content_eps_of(const st_plan* p, int i);
int alloc_kind_of(const st_plan* p, int j);    // what ensure_style_alloc is asked for entry j: its kind, 2 for a diagonal W2 entry, 3 for a marginal one, 4 for a nearest one

// ---- st_laplacian.hip
// the plan's Laplacian terms on `image`, behind the TV launch that wrote `grad` and `slot`: each pool size's term onto the
// slot and its gradient onto grad, in list order
int laplacian_terms(st_plan* p, const float* image, float* grad, float* slot, hipStream_t s);

// ---- st_mask.hip
// style regions in force: the heads of regions 1 .. R - 1 for these style positions under these kinds (st_plan_set_style_regions,
// and st_plan_set_taps / the kinds setters BEFORE they change the plan: a failed allocation leaves it as it was)
int ensure_region_heads(st_plan* p, int regions, const int* style_ops, int n_style, const int* kinds);

// ---- st_strip.hip
int halo_alloc(st_plan* p, float** out, size_t floats);

// ---- st_range_guard.hip
int range_guard(st_net* net, int conv, const float* weight_dev, int cin, int cout);

}  // namespace st
