/*
 * st_amd.h - C ABI of libst_amd.so, the MI355X (gfx950) implementation of the per-iteration hot path
 * of crowsonkb/style-transfer-pytorch.
 *
 * The reference has no FFI layer: its hot path sits behind the Python class `StyleTransfer`
 * (reference style_transfer/style_transfer.py:309-499).  This header is the seam a maintainer binds
 * from that class (ctypes).  Every entry point below names the reference code it
 * replaces.  Conventions:
 *   - plain C, no C++/torch types; all tensors are raw DEVICE pointers to dense fp32, batch 1,
 *     channel-major [C][H][W] (the memory of a contiguous torch NCHW tensor with N == 1);
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls are asynchronous
 *     on that stream unless stated otherwise;
 *   - return value 0 = success, non-zero = failure with text available from st_last_error();
 *     no C++ exception crosses the boundary;
 *   - handles are opaque and owned by the caller (create/destroy pairs); not thread-safe per handle;
 *   - alignment: a tensor pointer need only be 4-byte aligned (a dense fp32 tensor: `batch[1]` of a [2][3][45][54] batch is 8
 *     bytes past a 16-byte boundary) unless its entry says otherwise - the launchers take their 16-byte paths only when the
 *     shape and every pointer of the launch allow them, and the scalar paths otherwise.  Where an entry demands more - the
 *     standalone heads' feat / state / grad_feat, the L-BFGS state, the `scratch` of the sort, nearest and sliced entries
 *     and the nearest entries' `prepared` - a pointer that violates it is refused (non-zero, st_last_error() names the
 *     argument) before anything is launched or written.  tests/test_caller_buffers_gpu.py holds the entries to this.
 */
#ifndef ST_AMD_H
#define ST_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

#define ST_AMD_ABI_VERSION 2

/* VGG-19 `features` indices of the taps (style_transfer.py:316-317). */
#define ST_NUM_CONVS 13
#define ST_NUM_STYLE_LAYERS 5
#define ST_CONTENT_LAYER 22
#define ST_NUM_LOSS_TERMS 7 /* SumLoss order: content, style relu1_1..relu5_1, tv (style_transfer.py:455) */

enum st_pooling { ST_POOL_MAX = 0, ST_POOL_AVERAGE = 1, ST_POOL_L2 = 2 }; /* style_transfer.py:21-22 */

typedef struct st_net st_net;   /* frozen VGG-19 trunk weights, pre-arranged for the kernels      */
typedef struct st_plan st_plan; /* every device buffer for one image size ("one handle per scale") */

/* Text of the last failure on the calling thread ("" if none). */
const char* st_last_error(void);
int st_abi_version(void);
/* Name of the gfx target the kernels were compiled for ("gfx950"). */
const char* st_compiled_arch(void);
/* Size limit.  ONE number bounds every map the library is handed: an image, a strip, a tap or a feature map holds at most
 * st_max_pixels() = 2^24 - 1 = 16 777 215 pixels (height * width, or npix), whatever its channel count - 4095 x 4097 is the
 * largest near-square image.  It is the size up to which every 32-bit byte offset, buffer-resource size and out-of-range
 * offset constant of the kernels is proven (profiles/size_limits.md: one row per entry point) and tested
 * (tests/test_size_limits_gpu.py).  Every entry point that takes a height and a width, or a pixel count - st_plan_create,
 * st_plan_create_strip (the strip's rows x width), st_head_create, st_op_conv3x3 and its _dgrad / _strip / _strip_ex forms,
 * st_op_conv1x1, st_op_pool2x2 and its backward, st_op_tv_loss / st_op_tv_value / st_op_tv_loss_backward,
 * st_op_channel_moments, st_op_w2_diag_loss and its backward, st_op_laplacian_* - refuses a larger map with a message
 * that names the limit, before it allocates or launches anything.  The calls on a plan (st_plan_forward, _backward,
 * _loss_and_grad, _step, the mask and region setters) take their size from the plan and inherit its check.  Entries that
 * take an element COUNT (st_op_mse_loss, st_op_scaled_mse_loss and their backwards) index with 64-bit integers and have no
 * limit of their own.  Larger images: cut them into row strips (st_plan_create_strip), each strip within the limit. */
long long st_max_pixels(void);
/* Build flavour: 1 when the library was built with `build.py --experiments` - it then also holds the code that no default path
 * executes (persistent Newton-Schulz chain kernel, Winograd convolution = conv precision code 5, reproducer and measurement-only
 * kernels) and reads EVERY ST_* switch from the environment; 0 for the default build (the hot path and nothing else). */
int st_has_experiments(void);
/* The ST_* switches a default build reads from the environment (the documented ones, tools/README.md): fills
 * names[0 .. min(count, capacity)) with static strings and returns count.  Every other switch answers to st_set_option only. */
int st_env_switches(const char** names, int capacity);
/*
 * Run-time override of one of the library's ST_* switches (the same names as the environment variables the
 * A/B experiments use: ST_CONV_PC, ST_CONV_PC_XL, ST_NS_FULL_BACKWARD, ...).  Overrides win over the
 * environment; clear != 0 removes the override again.  No counterpart in the reference: it exists so that the
 * parity tests can compare two kernel variants on identical operands inside one process (e.g. the
 * producer / consumer convolution against the single-role kernel, bit for bit).  Not thread-safe with respect
 * to launches in flight on other host threads.
 */
int st_set_option(const char* name, int value, int clear);

/*
 * VGGFeatures.__init__ (style_transfer.py:24-49): truncated vgg19.features[:30], conv1_1 with
 * replicate padding (:39), pooling flavour (:41-46), weights frozen (:48-49).
 * weights[i]: device ptr [Cout][Cin][3][3]; biases[i]: device ptr [Cout]; i = 0..12 in network order.
 * The arrays of pointers themselves live in host memory.  Synchronous (returns after the re-layout).
 */
int st_net_create(st_net** out, const float* const* weights, const float* const* biases, int pooling);
/*
 * As st_net_create, with the arithmetic of the twelve 3x3 trunk convolutions (forward and data gradient):
 *   0 = exact fp32 MFMA (default; bitwise an fp32 FMA chain),
 *   3 = "bf16x6": fp32 operands as three bf16 planes, six bf16 MFMA products, fp32 accumulation (fp32-class accuracy),
 *   2 = "bf16x3": two planes, three products (per-product relative error <= ~2^-16),
 *   4 = "fp16x3": two fp16 planes (22 significant bits: residual <= 2^-24 |x| with round-to-nearest), three
 *       fp16 MFMA products, fp32 accumulation; both operands are pre-scaled by a power of two taken from the
 *       tensor's max |x| (measured on device before each launch), undone exactly in the epilogue: fp32-class
 *       accuracy at half the matrix work of bf16x6.
 * Everything else (conv1_1, Gram, sqrtm chains, losses, optimiser) is fp32 in every mode.
 */
int st_net_create_ex(st_net** out, const float* const* weights, const float* const* biases, int pooling,
                     int conv_precision);
/* fp16x3 networks (conv_precision 4): which of the 13 convolutions the dynamic-range guard moved to bf16x6 (three bf16
 * planes, no per-tensor scale) - forward13[i] / backward13[i] = 1 for conv i's forward / data gradient.  A layer is
 * flagged when one of its input (forward) / output (data gradient) channels carries weights more than 2^8 above the
 * layer's median channel: the signature of weights that compensate a tiny-valued operand channel, which two fp16
 * planes under one scale per tensor cannot hold.  All zero for normalised weights (the synthetic ones included). */
int st_net_wide_layers(const st_net* net, int* forward13, int* backward13);

/* Activation-aware part of the same guard (round 4; no reference counterpart - the reference computes in fp32).  On the
 * cold path, once per scale and image: every unflagged trunk convolution of `plan`'s network is evaluated in bf16x6 on
 * exactly the operand the shipped fp16x3 pass feeds it - forward on the maps of a forward pass over `image`
 * ([3][H][W], the plan's size), data gradient on the gradients of one closure (needs the plan's targets; without them
 * only the forward is checked) - and a layer whose fp16x3 result differs by more than 1e-5 rel-L2 over the map, or on any
 * output channel by more than 16 x what the exact-fp32 kernel differs there, runs bf16x6 from then on (sticky for the NETWORK; st_net_wide_layers shows
 * the union).  forward13 / backward13 receive the layers flagged by THIS call.  Synchronous; unsharded plans. */
int st_plan_range_guard(st_plan* plan, const float* image, int* forward13, int* backward13, void* stream);
/* Adds layers to the network's bf16x6 set from outside (flags only ever accumulate).  Strip-sharded runs: every rank runs the
 * guard on its own rows and the ranks take the union, so that all of them compute a layer in the same arithmetic. */
int st_net_mark_wide(st_net* net, const int* forward13, const int* backward13);
int st_net_destroy(st_net* net);

/* Buffers for an H x W image.  VGGFeatures.forward's size check (:81-83): fails if min(H, W) < 16. */
int st_plan_create(st_plan** out, const st_net* net, int height, int width);
int st_plan_destroy(st_plan* plan);
/* Bytes of device memory held by the plan (for STIterate.gpu_ram style reporting). */
long long st_plan_device_bytes(const st_plan* plan);

/*
 * VGGFeatures.forward (style_transfer.py:78-90), forward only, up to and including `last_layer`
 * (a features index 1..29).  `image` is [3][H][W] in [0,1] (un-normalised; Normalize is fused, :85).
 */
int st_plan_forward(st_plan* plan, const float* image, int last_layer, void* stream);
/* Borrow a tap (any ReLU/pool index computed by the last forward): dense [C][h][w] device pointer. */
int st_plan_feature(const st_plan* plan, int layer, const float** data, int* channels, int* height, int* width);
/*
 * The backward of VGGFeatures.forward (style_transfer.py:78-90) - what loss.backward() in the closure
 * (style_transfer.py:472-476: feats = self.model(self.image); loss = crit(feats); loss.backward()) runs through the trunk -
 * for gradients that arrive at the taps from OUTSIDE: the vector-Jacobian product of the last st_plan_forward on this plan.
 * A loss of the caller's own (StyleLoss, ContentLoss, a second content layer, feature inversion, ...) is evaluated on the
 * taps by the caller; this entry carries its gradient to the pixels.
 *   layers[i], i < count: a features index that st_plan_feature accepts (a ReLU output 1, 3, 6, 8, 11, 13, 15, 17, 20, 22,
 *       24, 26, 29 or a pool output 4, 9, 18, 27), at most the last forward's last_layer, each named once;
 *   grads[i]: device pointer, dense [C][h][w] fp32, the gradient with respect to that tap - read only; it must stay
 *       untouched until the launches have run (the array of pointers itself lives in host memory);
 *   grad_image [3][H][W]: WRITTEN, not accumulated into; the backward of Normalize (:85) and the fold of conv1_1's
 *       replicate padding (:39) are included, as in the closure.
 * The pass starts at the deepest layer named, every gradient is masked by its producer (threshold_backward once, on the
 * total that has arrived at a ReLU), and a tap's own gradient and the one from the layers above it are added in the tap's
 * gradient buffer.  Every launch goes on `stream`; the call does not wait for the device.
 * It fails when no st_plan_forward is current on the plan - none has run, or a closure (st_plan_loss_and_grad,
 * st_plan_step, st_plan_lbfgs_step, st_plan_range_guard) has run since, whose fused pools leave argmax codes instead of
 * maps: run st_plan_forward again - when a layer lies beyond that forward's last_layer, is no ReLU or pool output or is
 * named twice, when count < 1, and on strip plans.  Not to be captured into a hipGraph.
 * Memory: the gradient buffers (one per activation) are allocated by the first call, as by the first closure: it roughly
 * doubles the plan's activation memory (st_plan_device_bytes shows it).
 */
int st_plan_backward(st_plan* plan, int count, const int* layers, const float* const* grads, float* grad_image,
                     void* stream);

/*
 * StyleLossW2.get_target (style_transfer.py:162-168) on a tap of the last forward:
 * mean_out[C] = spatial mean, srm_out[C*C] = F F^T / (h*w).  `layer`: any features index that st_plan_feature accepts
 * (C = 64, 128, 256 or 512); on strip plans one of {1,6,11,20,29}.
 */
int st_plan_moments(st_plan* plan, int layer, float* mean_out, float* srm_out, void* stream);

/*
 * A spatial mask for the style statistics: which pixels of the plan's image the style terms see.  The reference has no such
 * control; the semantics are fixed here.  `mask` is [H][W] fp32 on the device with values in [0, 1], at the plan's image
 * size; NULL clears it.  A pyramid of five levels is kept: level 0 is the mask, level k + 1 the plain mean of the 2 x 2 cells
 * of level k at floor sizes (avg_pool2d(m, 2): the geometry of the trunk's pools, whatever the pooling mode), and a tap takes
 * the level of the number of pools at or before it - features 1, 3: level 0; 4, 6, 8: 1; 9 ... 17: 2; 18 ... 26: 3; 27, 29: 4.
 * While a mask is in force, with m the tap's level and M the sum of m, every style head takes the WEIGHTED moments
 *     mean = sum_p m_p f_p / M,   srm = sum_p m_p f_p f_p^T / M
 * in the place of StyleLossW2.get_target(input) inside StyleLossW2.forward (style_transfer.py:175-181) and of F F^T / N
 * inside StyleLoss.forward (:141-142), and its gradient is that of those formulas: dF = (Ssym F + b 1^T) diag(m) with M in
 * the place of N in (Ssym, b).  Targets, eps, weights, the Newton-Schulz chains and their backward are untouched; the content
 * and TV terms see no mask.  It applies to every closure and step (st_plan_loss_and_grad, st_plan_step, st_plan_lbfgs_step,
 * st_plan_range_guard) and to st_plan_moments - which is how the style of only a part of a style image is taken: set the
 * mask on the style plan, take the moments, clear it.  A masked plan runs the general closure (csrc/st_taps.hip), on the
 * default configuration too, and launches eagerly; a plan whose mask is cleared is, bit for bit, one that never had one.
 * The lists, kinds, eps, weights and targets all stay.  The call is synchronous (the levels' sums are read back here, once:
 * no closure reads anything back) and invalidates a captured graph.  It fails, naming the cause, on a strip plan, for a NaN
 * or a value outside [0, 1], and when a level sums to 0 (the level is named: a mask can be non-zero only in a row or column
 * that a floor-sized level drops); a refused mask leaves the plan without one.
 */
int st_plan_set_style_mask(st_plan* plan, const float* mask_or_null, void* stream);
/* Borrow level `level` (0 .. 4) of the mask in force, as the plan keeps it: the SQUARE ROOT of the level, dense [h][w] fp32 on
 * the device, with the level's sum M.  Any output pointer may be null.  Fails when no mask is set. */
int st_plan_style_mask(const st_plan* plan, int level, const float** sqrt_mask, int* h, int* w, double* sum);

/*
 * Several style regions, each with its own style (Gatys et al.'s guided transfer: sky from one painting, ground from
 * another).  The reference has no such control; the semantics are fixed here.  R regions, 1 <= R <= 4.  Region r has a mask
 * m_r - masks[r], [H][W] fp32 on the device with values in [0, 1], at the plan's image size, with the style mask's pyramid
 * (above) of its own -, one target per listed style layer (st_plan_set_region_style_target) and a weight rho_r
 * (st_plan_set_region_weights; 1 / R each after every successful call here).  With M_r the sum of m_r at the tap's level,
 * the term of (region r, style entry j) is the module of entry j's own kind and eps - StyleLossW2 or StyleLoss - on the
 * weighted moments
 *     mean = sum_p m_r,p f_p / M_r,   srm = sum_p m_r,p f_p f_p^T / M_r
 * against region r's target of that layer, times style_weight[j] * rho_r: the style mask's formulas, once per region.  The
 * style term of entry j (st_plan_term_losses, which keeps its shape) is the fp32 sum of its regions' terms in region order;
 * the feature gradient of the layer is sum_r (Ssym_r F + b_r 1^T) diag(m_r), accumulated in region order, and a content
 * term of the same layer is added after it.  Masks may overlap and need not sum to 1; a pixel in no region takes no style.
 * The content and TV terms, and st_plan_moments, see no region.
 * While regions are in force the plan runs the general closure (csrc/st_taps.hip), on the default configuration too, for
 * st_plan_loss_and_grad, st_plan_step, st_plan_lbfgs_step and st_plan_range_guard, on the caller's stream, launching
 * eagerly; two closures give equal bits (one owner per gradient element, no atomics).  n_regions == 0 clears them
 * (masks may be NULL then): the plan is then, bit for bit, one that never had any; and a plan with one region of weight 1
 * and mask m is, bit for bit, the plan with st_plan_set_style_mask(m).  Regions and a style mask exclude each other: either
 * setter fails, naming the other, while the other is in force - clear first.  The lists, kinds, eps, weights and the
 * targets already set stay (a region's targets are kept in heads of its own, which this call allocates for the listed
 * style layers; st_plan_set_taps and the kinds setters do so again - the masks and weights survive them, the targets do
 * not).  The call is synchronous - every region's level sums are read back here, in one read-back - and invalidates a
 * captured graph.  It fails, naming the cause, on a strip plan, for more than 4 regions, and for a region (named) whose
 * mask holds a NaN or a value outside [0, 1] or has a level (named) that sums to 0; a refused call leaves the plan without
 * regions.
 */
int st_plan_set_style_regions(st_plan* plan, int n_regions, const float* const* masks, void* stream);
/* Borrow level `level` (0 .. 4) of region `region`'s mask as the plan keeps it: the SQUARE ROOT of the level, dense [h][w]
 * fp32 on the device, with the level's sum M.  Any output pointer may be null.  Fails when no regions are set. */
int st_plan_style_region(const st_plan* plan, int region, int level, const float** sqrt_mask, int* h, int* w, double* sum);
/* st_plan_set_style_target for region `region` (0 .. R - 1) of the regions in force; region 0's target is the plan's own
 * (st_plan_set_style_target is this call with region 0, and the only region a plan without regions has). */
int st_plan_set_region_style_target(st_plan* plan, int region, int index, const float* mean, const float* srm, void* stream);
/* rho_r of the regions in force: R finite host floats, used as given (not normalised); NULL restores 1 / R each.  Fails when
 * no regions are set.  Invalidates a captured graph. */
int st_plan_set_region_weights(st_plan* plan, const float* weights_or_null);
/* The weighted terms of every (region, style entry) as the plan's last closure left them: *terms = device array
 * [*regions][*styles] of floats, owned by the plan.  regions and styles may be null.  Fails when no regions are set. */
int st_plan_region_terms(st_plan* plan, float** terms, int* regions, int* styles);

/*
 * Spatial weight maps for the content and the TV term: where the picture stays close to the content image, and where it is
 * smoothed.  The reference has neither; the semantics are fixed here.  `mask` is [H][W] fp32 on the device with values in
 * [0, 1], at the plan's image size; NULL clears the map.
 *
 * The content map w is averaged down to the trunk's five resolutions as the style mask is (level k + 1 = avg_pool2d(level k,
 * 2) at floor sizes, whatever the pooling mode), and the plan keeps the levels themselves.  A content layer takes the level
 * of the number of pools at or before it.  With d = F - T on a [C][h][w] tap, w_p the level's value at pixel p and cw the
 * entry's weight:
 *     kind mse (ContentLossMSE):     term = cw sum_{c,p} w_p d^2 / (C h w),        seed = cw (2 / (C h w)) w_p d
 *     kind scaled_mse (ContentLoss): S2 = sum w_p d^2, S1 = sum w_p |d| + eps, L = S2 / S1,
 *                                    term = cw L,                                 seed = cw w_p (2 d - L sgn d) / S1
 * The normaliser stays the element count, not the map's sum: a map of ones gives the unweighted term, and a smaller map
 * lowers the term where less was asked for.  One map serves every content layer, each at its own level, and every eps.
 *
 * The TV map w is used at the image's size only, as given.  Each squared difference of the nine-point TVLoss
 * (style_transfer.py:184-195) is weighed by the mean of the map at the difference's two end points, the map
 * replicate-padded as the image is; the counts in the denominators are unchanged.  With P and Wp the padded image and map
 * and s1 .. s4 the reference's slices,
 *     q(a, b) = mean(((Wp[a] + Wp[b]) / 2) (P[a] - P[b])^2)
 *     tv = 2 (q((s1,s2),(s1,s1)) / 3 + q((s2,s1),(s1,s1)) / 3 + q((s4,s4),(s3,s3)) / 12 + q((s4,s3),(s3,s4)) / 12)
 * the term is tv_weight times that, and the gradient is the gradient of exactly that.  A map of ones is TVLoss.
 *
 * The two maps are independent of each other and of the style mask and the style regions: all may be in force together.  A
 * plan with either map runs the general closure (csrc/st_taps.hip), on the default configuration too, for
 * st_plan_loss_and_grad, st_plan_step, st_plan_lbfgs_step and st_plan_range_guard, launching eagerly; there are no
 * floating-point atomics, so two closures give equal bits.  A plan whose maps are cleared is, bit for bit, one that never had
 * any.  Setting or clearing a map keeps the lists, kinds, eps, weights and every target (a content target does not depend on
 * the map) and invalidates a captured graph.  The setters are synchronous: the map is validated on the device in the pass
 * that builds the levels, and the result is read back once.  They fail, naming the cause, on a strip plan, for a NaN or a
 * value outside [0, 1], and for a map that is zero everywhere; a refused map leaves the plan without that map.
 */
int st_plan_set_content_mask(st_plan* plan, const float* mask_or_null, void* stream);
/* Borrow level `level` (0 .. 4) of the content map in force as the plan keeps it: the level itself, dense [h][w] fp32 on the
 * device.  Any output pointer may be null.  Fails when no content map is set. */
int st_plan_content_mask(const st_plan* plan, int level, const float** map, int* h, int* w);
int st_plan_set_tv_mask(st_plan* plan, const float* mask_or_null, void* stream);
/* Borrow the TV map in force: a bit-exact copy of what was given, dense [H][W] fp32 on the device.  Any output pointer may be
 * null.  Fails when no TV map is set. */
int st_plan_tv_mask(const st_plan* plan, const float** map, int* h, int* w);

/*
 * A Laplacian loss on average-pooled images (Li et al., "Laplacian-Steered Neural Style Transfer"): the content image's edges
 * and fine structure survive the style.  The reference has none; the semantics are fixed here.  x is the un-normalised
 * [3][H][W] image in [0, 1] that the TV term sees, c the content image at the same size, `pools` 1 to 4 distinct integers
 * p >= 1.  Per pool size p:
 *     Q_p(x) = avg_pool2d(x, p): kernel and stride p, floor sizes h_p = H / p, w_p = W / p, the trailing rows and columns
 *              dropped; for p = 1 it is x itself.  A window is summed row-major in fp32 and divided by p^2.
 *     L(Q)[i][j] = 4 Q[i][j] - Q[i-][j] - Q[i+][j] - Q[i][j-] - Q[i][j+] per channel, the neighbour indices clamped to the map
 *              (the map replicate-padded, as TVLoss pads the image); the subtractions in that order.
 *     T_p = L(Q_p(c)), computed once by the setter with the very kernels the closure runs: x == c gives a residual of exactly 0.
 *     term_p = weight sum((L(Q_p(x)) - T_p)^2) / (3 h_p w_p)
 * A mean where the paper has a sum: every other term here is a mean, and a weight then means the same at every scale of the
 * multi-scale loop.  The Laplacian term is the fp32 sum of the term_p in list order, and the gradient is the gradient of
 * exactly that: pixel (y, x) with y < h_p p and x < w_p p receives (2 weight / (3 h_p w_p p^2)) (L^T r_p)[y / p][x / p], a pixel
 * in a dropped trailing row or column nothing from that pool size.  L^T folds the clamped neighbours back: a border
 * position's own row of L names it once more per side at the border - which, for this replicate-padded stencil, makes L^T
 * equal to L (the operator is symmetric).  Every p must leave a pooled map of at least 2 x 2 (H / p >= 2 and W / p >= 2): on a
 * 1-wide map the clamped Laplacian is identically zero.
 *
 * Accounting.  The 8-float loss array has no free slot in the reference's configuration, and a step's tail forms the total
 * as 0 + l[0] + ... + l[6].  So slot 6 - and the last entry of st_plan_term_losses, whose count stays n_content + n_style + 1 -
 * becomes the image-space slot: the TV launch writes tv there as before, then each pool size's final reduction adds its
 * term_p onto it, in list order, stream-ordered, from one thread: the slot holds fp32(((tv + term_p0) + term_p1) + ...).
 * st_plan_laplacian_terms reads [tv alone, term_p0, term_p1, ...] of the last closure.  Without a Laplacian nothing changes,
 * bit for bit.
 *
 * st_plan_set_laplacian is synchronous; it allocates Q, r and T per pool size and builds the targets from `content_image`
 * ([3][H][W] fp32 on the device, at the plan's size; not kept).  NULL clears the Laplacian (the other arguments are then
 * ignored).  It fails, naming the cause, on a strip plan, for n_pools outside 1 .. 4, a repeated or non-positive p, a p that
 * leaves less than 2 x 2, and a weight that is not finite and > 0; a refused call leaves the plan without a Laplacian.
 * Setting or clearing keeps the lists, kinds, eps, weights, masks, maps and every target and invalidates a captured graph.  A
 * plan with a Laplacian runs the general closure (csrc/st_taps.hip), on the default configuration too, for
 * st_plan_loss_and_grad, st_plan_step, st_plan_lbfgs_step and st_plan_range_guard: three launches per pool size (pool,
 * residual and value, gradient add) right behind the TV launch, no floating-point atomics, so two closures give equal bits.
 * A plan whose Laplacian is cleared is, bit for bit, one that never had one.  It is independent of the style mask, the
 * regions and the content / TV maps: all may be in force together.  Out of scope: a spatial map on this term, strips.
 */
int st_plan_set_laplacian(st_plan* plan, const float* content_image_or_null, int n_pools, const int* pools, float weight,
                          void* stream);
/* Borrow T of the k-th pool size (list order): dense [3][h][w] fp32 on the device.  Any output pointer may be null.  Fails when
 * no Laplacian is set. */
int st_plan_laplacian(const st_plan* plan, int k, const float** target, int* h, int* w);
/* The last closure's [tv alone, term_p0, term_p1, ...]: *count = 1 + n_pools device floats owned by the plan.  Fails when no
 * Laplacian is set. */
int st_plan_laplacian_terms(st_plan* plan, float** terms, int* count);

/*
 * StyleTransfer.content_layers / style_layers (style_transfer.py:315-317, read by every scale at :425-453): the layers the
 * plan's closure puts its ContentLossMSE and StyleLossW2 terms on.  Each entry is a features index that st_plan_feature
 * accepts - the 13 ReLU outputs 1 3 6 8 11 13 15 17 20 22 24 26 29 and the 4 pool outputs 4 9 18 27; the reference also
 * accepts pre-ReLU convolution outputs, which the fused trunk does not keep.  Each list holds 0 to 16 entries (the plan
 * has 16 bound words for its heads), each named once per list; together they name at least one layer; a layer may be in both.
 * A plan that was never configured, or is configured with content [22], style [1 6 11 20 29], runs the closure built for
 * that configuration; every other one runs a general closure (csrc/st_taps.hip: plain forward to the deepest layer named,
 * one head per layer, st_plan_backward's pass from the heads' gradients onto the TV gradient) through the same entries:
 * st_plan_loss_and_grad, st_plan_step, st_plan_lbfgs_step, st_plan_range_guard.  Such a plan always launches eagerly
 * (st_plan_set_graph has no effect on it).  The call drops every target set before, invalidates a captured graph and
 * allocates what the configuration needs (the five heads of the default lists too, which a plan that was never configured
 * allocates when their targets are set).  Weights: a plan on the default lists that is given the default lists again keeps
 * its weights; every other call resets them to the new lists' defaults - content 0.015 / n_content each (:366) and style
 * 1 / n_style each, or, for the default lists, the weights of a fresh plan (0.015; 256/341 ... 1/341) - so set the weights
 * after the layers.  Fails on strip plans.  Synchronous.
 */
int st_plan_set_taps(st_plan* plan, int n_content, const int* content_layers, int n_style, const int* style_layers);
/* Scale factors of the configured lists (style_transfer.py:320-322,366,376,429,453): content_weights[n_content],
 * style_weights[n_style], tv.  The general form of st_plan_set_loss_weights, which serves the default configuration only. */
int st_plan_set_tap_weights(st_plan* plan, const float* content_weights, const float* style_weights, float tv_weight);

/*
 * WHAT the terms are: one loss kind per list, for every layer of that list (per layer: st_plan_set_layer_loss_kinds below).
 *   content_kind  0 (default)  ContentLossMSE (style_transfer.py:119-126): mean((F - T)^2)
 *                 1            ContentLoss (:109-116): ScaledMSELoss (:93-106) of the features,
 *                              sum d^2 / (sum |d| + 1e-8) with d = F - T
 *   style_kind    0 (default)  StyleLossW2 (:149-181)
 *                 1            StyleLoss (:129-142), the Gatys loss: the same scaled MSE with d = F F^T / N - G_t, N the tap's
 *                              GLOBAL position count
 * The default kinds leave every configuration on the closure it has.  Any other kind sends every configuration - the
 * default lists too - through the general closure (csrc/st_taps.hip), by the same entries: st_plan_loss_and_grad,
 * st_plan_step, st_plan_lbfgs_step, st_plan_range_guard; such a plan always launches eagerly.  A Gram head runs no
 * Newton-Schulz chain and allocates no workspace for one.  The terms keep SumLoss order and the 8-float array its layout
 * (st_plan_term_losses).  The call drops every target set before (a style target is kept in the form its kind reads),
 * deals the heads' bound words again and invalidates a captured graph; the lists and all weights stay, and the kinds
 * survive a later st_plan_set_taps.  Fails for an unknown code, and on strip plans for any kind but the defaults.  Synchronous.
 * Every eps returns to its kind's default (st_plan_set_loss_eps).  st_plan_loss_kinds reports -1 for a list whose entries
 * differ (st_plan_set_layer_loss_kinds).
 */
int st_plan_set_loss_kinds(st_plan* plan, int content_kind, int style_kind);
int st_plan_loss_kinds(const st_plan* plan, int* content_kind, int* style_kind);

/*
 * The same per LAYER, as the reference builds one loss module per layer (style_transfer.py:425-429 the content modules,
 * :442-453 the style modules): content_kinds[n_content] and style_kinds[n_style] hold the codes above in list order; a null
 * pointer is allowed for an empty list.  Lists whose entries agree are st_plan_set_loss_kinds' setting, bit for bit.  A plan
 * whose entries are all of the default kinds, with every eps at its default, stays on the closure it has; any other runs
 * the general closure, each head by its own kind - a W2 head its Newton-Schulz chains, a Gram head its four launches - and
 * each head allocates what its own kind needs.  Everything else is as for st_plan_set_loss_kinds: the call drops every
 * target, deals the heads' bound words again, invalidates a captured graph and resets every eps; the lists and weights
 * stay; a failed allocation leaves the plan as it was; strip plans take the defaults only.  A later st_plan_set_taps keeps
 * the kind of a list whose entries agree and returns a mixed list to kind 0.  st_plan_layer_loss_kinds writes n_content /
 * n_style codes (either pointer may be null).
 * Order of configuration: layers (st_plan_set_taps), kinds, eps (st_plan_set_loss_eps), diagonal (st_plan_set_w2_diagonal),
 * marginal (st_plan_set_w2_marginal), nearest (st_plan_set_style_nearest), sliced (st_plan_set_style_sliced and its options and
 * seed), weights, then the targets.
 */
int st_plan_set_layer_loss_kinds(st_plan* plan, const int* content_kinds, const int* style_kinds);
int st_plan_layer_loss_kinds(const st_plan* plan, int* content_kinds, int* style_kinds);

/*
 * The eps of each layer's loss module: content_eps[n_content], style_eps[n_style] in list order.
 *   w2          StyleLossW2(target, eps=1e-4) (style_transfer.py:152): cov + eps I, in the target's covariance and root
 *               (st_plan_set_style_target) and in the input's covariance of every closure
 *   gram        StyleLoss(target, eps=1e-8) (:130) and
 *   scaled_mse  ContentLoss(target, eps=1e-8) (:110): ScaledMSELoss's sum |d| + eps (:97,:103)
 *   mse         ContentLossMSE (:119-126) has none
 * A negative value means the kind's default, and so does a value equal to it as a float; a null pointer sets every entry
 * of that list to its default.  Any other value runs the general closure, on the default lists too.  The call drops every
 * target set before (a W2 target's root depends on its eps) and invalidates a captured graph; either kinds setter and
 * st_plan_set_taps return every eps to the default, so set the eps after the kinds and before the targets.  Fails for a
 * non-negative eps on an mse content entry, for a NaN or an infinity, and on strip plans for any value but the defaults.
 * st_plan_loss_eps writes the effective values, -1 for an mse entry (either pointer may be null).
 */
int st_plan_set_loss_eps(st_plan* plan, const float* content_eps, const float* style_eps);
int st_plan_loss_eps(const st_plan* plan, float* content_eps, float* style_eps);

/*
 * StyleLossW2 with BOTH covariances restricted to their diagonals, per W2 style layer: flags[n_style], 0 or 1 in list order;
 * a null pointer clears all.  For two Gaussians with diagonal covariances W2^2 = sum_c (mu - mu_t)^2 + sum_c (sigma - sigma_t)^2:
 * the mean / standard-deviation (batch-norm statistics) loss of Li et al., "Demystifying Neural Style Transfer", and the
 * statistic AdaIN matches.  It is an OPTION of a w2 layer - the kind names and codes do not change - and the reference has no
 * such module, so the semantics are fixed here.  On the tap F [C][h w] of flagged entry j, with pixel weights m_p and
 * M = sum_p m_p (no style mask: m = 1, M = N; a mask or regions: the level and sum the entry's head already reads):
 *   mu_c  = sum_p m_p f_cp / M          q_c = sum_p m_p f_cp^2 / M
 *   v_c   = max(q_c - mu_c^2, 0) + eps  sigma_c = sqrt(v_c)             (eps: the layer's style eps, default 1e-4, as for W2)
 *   target, from the SAME (mean, srm) that st_plan_set_style_target / st_plan_set_region_style_target are given:
 *   mut_c = mean_c,  vt_c = max(srm_cc - mean_c^2, 0) + eps,  sigmat_c = sqrt(vt_c)   (only srm's diagonal is read; no sqrtm runs)
 *   term_j = w_j (sum_c (mu_c - mut_c)^2 + sum_c (sigma_c - sigmat_c)^2) / C
 *   dF_cp  = w_j (m_p / M) ((2 / C) (mu_c - mut_c) + 2 g_c (f_cp - mu_c)),  g_c = (1 - sigmat_c / sigma_c) / C, 0 where sigma_c = 0
 * This is StyleLossW2.forward with cov -> diag(cov).  The variance term is (sigma - sigma_t)^2, not v + v_t - 2 sqrt(v v_t),
 * which cancels near the target: the first form gives exactly 0 and an exactly zero gradient there.  With regions the entry's
 * weight is style_weight[j] rho_r, the term lands in slot (r, j), region 0 writes the seed and regions r >= 1 add onto it in
 * region order; a content term of the same layer is added after, as for every head.
 * A flagged head is two memory-bound launches (csrc/st_w2diag.hip) - no Gram pass, no Newton-Schulz chain, no 1x1 step, no
 * fp16x3 operand bound - and allocates 2 C target floats, the partial sums, 2 C coefficients and a ticket: no C x C buffer.
 * Any set flag runs the general closure (csrc/st_taps.hip), on the default lists too; a plan whose flags are all 0 is, bit
 * for bit, one on which this was never called, and the default configuration stays on its own closure.  Like
 * st_plan_set_loss_eps the call drops every target set before and invalidates a captured graph; either kinds setter and
 * st_plan_set_taps clear the flags.  Fails for a flag on a gram entry, for a value other than 0 or 1, and for any set flag on
 * a strip plan.  st_plan_term_losses, st_plan_region_terms and the 8-float array keep their shapes.
 * Order of configuration: layers, kinds, eps, diagonal, weights, then the targets.
 */
int st_plan_set_w2_diagonal(st_plan* plan, const int* flags);
int st_plan_w2_diagonal(const st_plan* plan, int* flags);

/*
 * The exact per-channel Wasserstein (sorted) option of a W2 style layer: flags[n_style], 0 or 1 in list order; a null pointer
 * clears all.  Every other style statistic of a plan is a second moment of the tap; this one is the W2 distance between the
 * exact one-dimensional marginals of the tap's channels and of the style's - Risser et al.'s histogram loss in its exact form,
 * the sliced Wasserstein loss of Heitz et al. ("A Sliced Wasserstein Loss for Neural Texture Synthesis") taken along the channel
 * axes.  The diagonal head above is the same distance between the marginals' Gaussian fits.  It is an OPTION of a w2 layer - the
 * kind names and codes do not change - and the reference has no such module, so the semantics are fixed here.  For flagged
 * entry j with tap F [C][N], N = h w, and target T [C][N], every row non-decreasing:
 *   pi_c    the stable ascending order of row c: ties are broken by ascending pixel index and -0.0 compares equal to +0.0
 *           (torch.sort(f + 0.0, stable=True))
 *   term_j = w_j sum_c sum_k (f_c,pi_c(k) - T_c,k)^2 / (C N)
 *   dF_c,pi_c(k) = w_j (2 / (C N)) (f_c,pi_c(k) - T_c,k)
 * The permutation is a constant of the gradient: the a.e. derivative, which autograd gives for sort.  Inputs are finite; with a
 * NaN the result is unspecified, but the launches end (no loop's trip count depends on a comparison of values).  There is no
 * eps.  The term is exactly 0 with an exactly zero gradient when the tap is the target's source.
 * Target: Q [C][n_q], the quantile function of a style tap - its rows sorted - resampled to the plan's N by
 *   T_c,i = lerp(Q_c, u),  u = clamp((i + 1/2) n_q / N - 1/2, 0, n_q - 1) evaluated in double,
 * linear between floor(u) and floor(u) + 1 in fp32 (midpoint convention: order statistic k sits at (k + 1/2) / n_q); n_q == N is
 * a copy, bit for bit.  Several style images blend as their resampled quantile functions, weighted - in one dimension the
 * Wasserstein barycentre, as blending (mean, srm) is for the moments.
 * A flagged head (csrc/st_sort.hip) is a segmented stable sort of the tap's rows on 64-bit keys (value image | pixel index: one
 * LDS bitonic launch over chunks of st_op_sort_chunk() keys and ceil(log2(N / chunk)) merge passes) and a residual pass that writes
 * the gradient through the permutation (a content term of the same layer adds after it) and reduces the term by per-block fp32
 * partials, a ticket and the last block's index-order sum in double.  Integer atomics only: two runs give the same bits.  It
 * allocates the C N target, two buffers of C N keys, the partials and a ticket; no C x C buffer, no Newton-Schulz workspace.
 * Any set flag runs the general closure (csrc/st_taps.hip), on the default lists too; flags that are all 0, or set and then
 * cleared, leave, bit for bit, a plan on which this was never called.  Like st_plan_set_w2_diagonal the call drops every target
 * set before and invalidates a captured graph; either kinds setter and st_plan_set_taps clear the flags.
 * Fails for a flag on a gram entry, on an entry flagged diagonal (and st_plan_set_w2_diagonal refuses an entry flagged here), on
 * an entry with a non-default eps (and st_plan_set_loss_eps refuses one for an entry flagged here), for a value other than 0 or
 * 1, for any set flag on a strip plan, and while a style mask or style regions are set (their setters refuse while a flag is
 * set): weighted quantiles are not implemented.  st_plan_term_losses and the 8-float array keep their shapes.
 * Order of configuration: layers, kinds, eps, diagonal, marginal, weights, then the targets.
 */
int st_plan_set_w2_marginal(st_plan* plan, const int* flags);
int st_plan_w2_marginal(const st_plan* plan, int* flags);
/* The target of flagged style entry `index`: q [C][n_q], sorted rows (device memory), resampled to the plan's N as above.  Fails
 * on an entry that is not flagged; st_plan_set_style_target fails on a flagged one. */
int st_plan_set_style_quantiles(st_plan* plan, int index, const float* q, long long n_q, void* stream);
/* Borrows the resampled target of flagged entry `index`: *target [C][N] floats of the plan's, valid until the plan is destroyed. */
int st_plan_style_quantiles(st_plan* plan, int index, float** target, int* channels, long long* n);

/*
 * The nearest-neighbour feature-matching option of a W2 style layer: flags[n_style], 0 or 1 in list order; a null pointer clears
 * all.  Every other style statistic of a plan is a SUMMARY of the tap - second moments, or the per-channel distributions; this one
 * says that each pixel's feature vector should look like some particular feature vector of the style image: the MRF /
 * neural-neighbour family of style losses (Li & Wand, "Combining Markov Random Fields and Convolutional Neural Networks for Image
 * Synthesis"; Kolkin et al., "Neural Neighbor Style Transfer"; the contextual loss), which copies local structure that moment
 * matching smears.  It is an OPTION of a w2 layer - the kind names and codes do not change - and the reference has no such
 * module, so the semantics are fixed here.  For flagged entry j with tap F [C][N], columns f_i, and the style's feature vectors
 * S [C][M], columns s_k (M need not equal N; nothing is resampled):
 *   k*(i)  = argmin_k |f_i - s_k|^2 = argmax_k (<f_i, s_k> - |s_k|^2 / 2),   ties: the lowest k
 *   term_j = w_j sum_i |f_i - s_k*(i)|^2 / (C N)
 *   dF_ci  = w_j (2 / (C N)) (f_ci - s_c,k*(i))
 * The match is a constant of the gradient: the a.e. derivative of min_k, so the gradient is the true gradient of the term.  The
 * term is the quantity the search minimises - the one-sided Chamfer distance from the tap to the style set - under the default
 * L2 metric and, with its own term, under the cosine and centred-cosine metrics of st_plan_set_nearest_metric below.  There is
 * no eps.  Inputs are finite; with a NaN the result is unspecified, but every launch
 * ends (no loop's trip count depends on a comparison of values, and an index is clamped into [0, M) before it is an address).
 * bias_k = -|s_k|^2 / 2 is formed once by st_plan_set_style_vectors, in double, and rounded to fp32.  The search
 * (csrc/st_nearest.hip) runs in the trunk's fp16x3 arithmetic with fp32 accumulation - S^T [M_pad][C] against the tap, both
 * scaled by a power of two under their bounds and split into two fp16 planes while they are staged - so a match is optimal up
 * to that arithmetic: |f_i - s_k*(i)|^2 exceeds the minimum by at most a few 2^-21 C max|F| max|S| (tests/test_style_nearest_gpu.py
 * derives the bound), and at the style's own tap the term is at most that, not promised to be exactly 0.  The scores are never
 * written: a workgroup owns 128 pixels and a contiguous range of k tiles, keeps a running (score, k) per lane, and writes one
 * (score, k) per pixel and split; the split count depends on the shape alone.  The finish pass merges the splits in split order
 * under the same rule (greater, or equal and lower k), gathers s_k* as a row of S^T, WRITES dF to the tap's seed buffer (a
 * content term of the same layer adds after it), keeps the matches (st_plan_nearest_indices) and reduces the term by per-block
 * fp32 partials, a ticket and the last block's index-order sum in double.  No floating-point atomics: two closures give the same
 * bits, indices included.  A flagged head allocates S^T, the bias, the split partials, N indices, the partials and a ticket; no
 * C x C buffer, no Newton-Schulz workspace.  The cost is 2 C N M flop per iteration (three times that on the 16-bit pipe).
 * Several style images give the UNION of their vectors: the caller concatenates them in image order.  An image of weight 0 is
 * left out; otherwise the per-image weights do not enter (a union has no weights).
 * Any set flag runs the general closure (csrc/st_taps.hip), on the default lists too; flags that are all 0, or set and then
 * cleared, leave, bit for bit, a plan on which this was never called.  Like st_plan_set_w2_diagonal the call drops every target
 * set before and invalidates a captured graph; either kinds setter and st_plan_set_taps clear the flags.
 * Fails for a flag on a gram entry, on an entry flagged diagonal or marginal (and their setters refuse an entry flagged here), on
 * an entry with a non-default eps (and st_plan_set_loss_eps refuses one for an entry flagged here), on an entry whose channel
 * count is no multiple of 32, for a value other than 0 or 1, for any set flag on a strip plan, and while a style mask or style
 * regions are set (their setters refuse while a flag is set).  st_plan_term_losses and the 8-float array keep their shapes.
 * Order of configuration: layers, kinds, eps, diagonal, marginal, nearest, weights, then the targets.
 */
int st_plan_set_style_nearest(st_plan* plan, const int* flags);
int st_plan_style_nearest(const st_plan* plan, int* flags);
/* The target of flagged style entry `index`: feat [C][m], the style's feature vectors as columns (device memory; a style tap as
 * it lies in a plan, or several side by side).  Transposed once into S^T [M_pad][C] with zero rows and a bias of -inf in the
 * padding, so padding never wins.  A set that needs larger buffers than the entry holds allocates new ones; the former stay
 * the plan's until it is destroyed (st_plan_device_bytes counts them), a smaller or equal set allocates nothing.  Until the call
 * has succeeded the entry holds no target.  Fails on an entry that is not flagged; st_plan_set_style_target and
 * st_plan_set_style_quantiles fail on a flagged one. */
int st_plan_set_style_vectors(st_plan* plan, int index, const float* feat, long long m, void* stream);
/* Borrows the matches of the last closure for flagged entry `index`: *idx [n] ints of the plan's (device memory), k*(i) in
 * [0, m), valid until the plan is destroyed and rewritten by every closure. */
int st_plan_nearest_indices(st_plan* plan, int index, const int** idx, long long* n);
/*
 * What a flagged entry is matched on: metrics[n_style] in list order, a null pointer means all 0.
 *   0 'l2'               the head above, bit for bit
 *   1 'cosine'           the neural-neighbour family's own metric (the contextual loss, STROTSS): a ReLU tap's vectors differ in
 *                        length by an order of magnitude across a picture, and under L2 a dim region is pulled to the style's
 *                        shortest vectors whatever their direction
 *   2 'centered_cosine'  cosine after subtracting the style set's mean feature (NNST)
 * The reference has no such module, so the semantics are fixed here.  eps = 1e-8, under both square roots below (as ContentLoss's
 * 1e-8, it is not an argument).  For metrics 1 and 2, with the style vectors S [C][M] handed to st_plan_set_style_vectors (after
 * any selection the caller made) and the tap F [C][N]:
 *   mu     = 0 (metric 1), or mu_c = (1/M) sum_k s_ck (metric 2): summed in double in ascending k, rounded to fp32 once
 *   s^_k   = (s_k - mu) / sqrt(|s_k - mu|^2 + eps): formed in double by the setter and rounded to fp32 once; a zero vector stays zero
 *   b_k    = -<mu, s^_k>: from the rounded s^_k and the rounded mu, summed in double in channel order, rounded once (0 for metric
 *            1); in the padding rows b_k = -inf and the row is zero
 *   g_i    = f_i - mu,   p_i(k) = <g_i, s^_k>,   r_i = sqrt(|g_i|^2 + eps)
 *   k*(i)  = argmax_k p_i(k) = argmax_k (<f_i, s^_k> + b_k),   ties: the lowest k
 *   term_j = w_j sum_i (1 - p_i(k*(i)) / r_i) / N            (divided by N, not by C; in [0, 2 w_j])
 *   dF_ci  = (w_j / N) (-s^_c,k*(i) / r_i + p_i(k*(i)) g_ci / r_i^3)
 * r_i > 0 does not depend on k, so k*(i) also maximises the cosine p_i(k) / r_i: the term is exactly what the search minimises.
 * The match and mu are constants of the gradient, which is the true gradient of the term almost everywhere.  At a tap pixel that
 * equals mu exactly the gradient is -(w_j / N) s^_k* / sqrt(eps).
 * The search is the L2 head's, unchanged, on the rows s^^T [M_pad][C] and the bias b: the prepared buffer is laid out as L2's -
 * bound word (max |s^|, measured, at most 1), bias, rows - with mu [C], padded to 64 floats, behind it.  The finish pass
 * (csrc/st_nearest.hip) is its own: one launch in which a workgroup owns 64 pixels and all their channels, merges the splits,
 * gathers s^_k*, recomputes p_i and |g_i|^2 in fp32 from g = f - mu (never the search's score) in a fixed channel order, WRITES
 * dF and the indices and reduces the term as every head does (per-block fp32 partials, the write-through hand-over to the last
 * block, its index-order sum in double).  No floating-point atomics: two closures give the same bits, indices included.  A match
 * is optimal up to the search's arithmetic (tests/test_nearest_cosine_gpu.py derives the bound on p_i(k_best) - p_i(k*)).
 * There is no user eps: an entry with a custom style eps cannot be flagged, as above.  Several style images give the union of
 * their vectors, and mu is the mean of that union.  Inputs are finite; with a NaN the result is unspecified, but every launch
 * ends and an index is clamped into [0, M) before it is an address.
 * Call it after st_plan_set_style_nearest - which resets every metric to 0, so existing callers see no change - and before the
 * weights and targets: st_plan_set_style_vectors prepares by the entry's metric and sizes the prepared and scratch buffers by it
 * (st_plan_device_bytes counts them).  Like the other option setters the call drops every target set before and invalidates a
 * captured graph; either kinds setter and st_plan_set_taps clear the metrics, as they clear the flags.  Metrics that are all 0, or
 * set and then cleared, leave, bit for bit, the plan with the same flags and no metric call.
 * Fails for a value outside 0..2 and for a non-zero metric on an entry that is not flagged.
 * Order of configuration, in full: layers, kinds, eps, diagonal, marginal, nearest, nearest metric, sliced (flags, options, seed),
 * weights, then the targets.
 */
int st_plan_set_nearest_metric(st_plan* plan, const int* metrics);
int st_plan_nearest_metric(const st_plan* plan, int* metrics);

/*
 * The sliced Wasserstein option of a W2 style layer: flags[n_style], 0 or 1 in list order; a null pointer clears all.  The
 * second-moment heads see two moments of the tap, the marginal head the exact one-dimensional distributions along the C channel
 * axes only, the nearest head single vectors.  This one is the W2 distance between the projections of the tap and of the style
 * onto P random unit directions, with new directions at every evaluation, so that over a run it sees the whole C-dimensional
 * distribution (Heitz et al., "A Sliced Wasserstein Loss for Neural Texture Synthesis").  It is an OPTION of a w2 layer - the
 * kind names and codes do not change - and the reference has no such module, so the semantics are fixed here.  For flagged
 * entry j with tap F [C][N], the style images' feature vectors S_i [C][M_i] in image order with blend weights a_i (the image's
 * weight over the sum of the weights; an image of weight 0 is left out) and directions R [P][C], every row of unit length:
 *   Y      = R F;  pi_p the stable ascending order of row p of Y + 0.0: ties by ascending pixel index, -0.0 equal to +0.0 (the
 *            marginal head's rule)
 *   T      = sum_i a_i resample_N(sort_rows(R S_i)),  resample_N: st_op_resample_quantiles' midpoint rule, M_i == N a copy; per
 *            direction the one-dimensional Wasserstein barycentre.  Image 0 writes a_0 q, image i > 0 adds a_i q, in fp32
 *   term_j = w_j sum_p sum_k (Y_p,pi_p(k) - T_p,k)^2 / (P N)
 *   dF     = w_j (2 / (P N)) R^T G,   G_p,pi_p(k) = Y_p,pi_p(k) - T_p,k
 * R and the permutations are constants of the gradient.  There is no eps.  With R = I and P = C the term is the marginal
 * head's term; the division is by P N, so a weight means the same for any P.  Inputs are finite; with a NaN the result is
 * unspecified, but every launch ends (no loop's trip count depends on a comparison of values).
 * Directions are generated on the device (csrc/st_sliced.hip), a wave per row.  Row p of entry j at epoch e is a vector of C
 * standard normals divided by its norm:
 *   mix(z):  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9;  z = (z ^ (z >> 27)) * 0x94d049bb133111eb;  z ^ (z >> 31)   (64-bit words:
 *            splitmix64's finaliser)
 *   key    = mix(mix(mix(seed ^ 0x9e3779b97f4a7c15) ^ (j + 1)) ^ e)
 *   h      = mix(key ^ (p << 32 | c))                      one hash word per element: a counter-based generator, no state
 *   u1     = ((h >> 41) + 1/2) 2^-23  in (0, 1),   u2 = ((h & 0xffffffff) >> 8) 2^-24  in [0, 1)
 *   z_pc   = sqrt(-2 ln u1) cos(2 pi u2)                   (Box-Muller, fp32; the device's fast log and cosine)
 *   r_pc   = z_pc / sqrt(sum_c z_pc^2): the sum in double, lane l of the wave adds c = l, l + 64, ... in ascending order and the
 *            64 sums meet in an xor butterfly (offsets 32, 16, ..., 1); the quotient in double, rounded once
 * Bit-equality with a host implementation is not promised (the device's log and cosine); st_plan_sliced_directions borrows R.
 * The same launch writes R [P][C] and R^T [C][P], the two weight layouts of the 1x1 step.  P is a multiple of 64 in [64, 512],
 * by default C (st_plan_set_sliced_options).
 * Epoch: one plan-wide counter, the epoch at which the NEXT evaluation of the general closure draws its directions.  While any
 * flagged entry resamples, every evaluation of the general closure advances it by one: st_plan_loss_and_grad, both native steps
 * and the range guard.  It is a HOST counter handed to the direction kernel as an argument: the general closure is never
 * captured into a graph (st_plan_set_graph replays the default closure only), so no replay can reuse an epoch.
 * st_plan_set_sliced_seed sets the seed and returns the epoch to 0.  An entry whose resampling is off draws its directions at
 * epoch 0, once, in st_plan_set_style_sliced_vectors, where its target is derived once too.  The same seed and the same sequence
 * of calls give the same bits; with resampling off two closures give the same bits.  No floating-point atomics anywhere.
 * A flagged head: with resampling on the direction kernel and, per style image, the target's share - R S_i through the 1x1 step,
 * the segmented sort of csrc/st_sort.hip on P rows, unpack, resample to N, blend; then Y = R F through the 1x1 step, the sort
 * and the residual pass on P rows, which writes G to a buffer of the head, and dF = R^T G through the 1x1 step (C_in = P,
 * C_out = C), WRITTEN to the tap's seed buffer (a content term of the same layer adds after it).  On an fp16x3 network the
 * three products run in fp16x3: the bound of R is 1 by construction, the tap's is the word its producer left, an image's is
 * measured once by the setter, and max |G| is measured on the device by the integer atomicMax pass that measures every other
 * operand (no host read); on an fp32 network they run on the exact fp32 MFMA.  At the style's own tap (M = N, one image) the
 * term is below 1e-10 of mean(Y^2) but not promised to be exactly 0: the tap's projection is scaled by its producer's bound, the
 * style's by a measured one, and the two can differ by a power of two.
 * It allocates R and R^T (for P = 512), T [P][N], the S_i, Y and G [P][max(N, max M_i)], two buffers of P max(N, max M_i)
 * keys, the partials, a ticket and the bound words; no C x C buffer, no Newton-Schulz workspace.
 * Any set flag runs the general closure (csrc/st_taps.hip), on the default lists too; flags that are all 0, or set and then
 * cleared, leave, bit for bit, a plan on which this was never called.  Like st_plan_set_style_nearest the call drops every
 * target set before and invalidates a captured graph; it also returns the flagged entries' options to their defaults and the
 * epoch to 0; either kinds setter and st_plan_set_taps clear the flags.
 * Fails for a flag on a gram entry, on an entry flagged diagonal, marginal or nearest (and their setters refuse an entry flagged
 * here), on an entry with a non-default eps (and st_plan_set_loss_eps refuses one for an entry flagged here), on an entry whose
 * channel count is no multiple of 64, for a value other than 0 or 1, for any set flag on a strip plan, and while a style mask or
 * style regions are set (st_plan_set_style_mask and st_plan_set_style_regions refuse while a flag is set): weighted quantiles
 * are not implemented.  st_plan_term_losses and the 8-float array keep their shapes.
 * Order of configuration: layers, kinds, eps, diagonal, marginal, nearest, sliced (flags, options, seed), weights, then the targets.
 */
int st_plan_set_style_sliced(st_plan* plan, const int* flags);
int st_plan_style_sliced(const st_plan* plan, int* flags);
/* Flagged entry `index`: `projections` directions (0: the tap's C; else a multiple of 64 in [64, 512]) and whether every closure
 * draws new ones (`resample` 1, the default) or the entry keeps those of epoch 0 (0).  Drops that entry's target.  Fails on an
 * entry that is not flagged. */
int st_plan_set_sliced_options(st_plan* plan, int index, int projections, int resample);
/* The seed of every flagged entry's directions (default 0); the epoch returns to 0 and the flagged entries' targets are dropped:
 * set it before the style vectors. */
int st_plan_set_sliced_seed(st_plan* plan, unsigned long long seed);
/* The target of flagged style entry `index`: n_images style images, feats[i] = S_i [C][ms[i]] in device memory (a style tap as it
 * lies in a plan), weights[i] >= 0 (host; null: equal weights).  The vectors are copied into the plan, each image's bound is
 * measured, and the directions of the current epoch and the target under them are derived on `stream`.  At most 16 images of
 * weight > 0, each of 1 to 2^24 - 1 vectors.  A set that needs larger buffers than the entry holds allocates new ones; the
 * former stay the plan's until it is destroyed (st_plan_device_bytes counts them).  Until the call has succeeded the entry holds
 * no target.  Fails on an entry that is not flagged; st_plan_set_style_target, st_plan_set_style_quantiles and
 * st_plan_set_style_vectors fail on a flagged one. */
int st_plan_set_style_sliced_vectors(st_plan* plan, int index, int n_images, const float* const* feats, const long long* ms,
                                     const float* weights, void* stream);
/* Borrows the directions the last closure used for flagged entry `index` (before any closure: those the setter drew):
 * *r [P][C] floats of the plan's (device memory), rewritten by every closure while the entry resamples; *epoch: theirs. */
int st_plan_sliced_directions(st_plan* plan, int index, const float** r, int* projections, int* channels, unsigned long long* epoch);
/* Borrows the target under those directions: *target [P][N] floats of the plan's (device memory). */
int st_plan_sliced_target(st_plan* plan, int index, const float** target, int* projections, long long* n);

/* ContentLossMSE target (style_transfer.py:425-429): copies feat [512][H/8][W/8] into the plan (a configured plan: the
 * target of content layer 0, shaped like that layer). */
int st_plan_set_content_target(st_plan* plan, const float* feat, void* stream);
/* The same for content layer `index` of the configured list (:425-429, one ContentLossMSE per layer): feat is [C][h][w] of that
 * layer. */
int st_plan_set_content_target_at(st_plan* plan, int index, const float* feat, void* stream);
/*
 * StyleLossW2.__init__ (style_transfer.py:152-160) for style layer `index` of the configured list (default: 0..4 =
 * relu1_1..relu5_1): cov = srm - mean mean^T + 1e-4 I, cov_sqrt = sqrtm_ns(cov, 12) (sqrtm.py:9-25).
 * mean[C], srm[C*C] are the (already blended, :442-450) targets.
 * The 1e-4 is the layer's eps (st_plan_set_loss_eps).
 * With style kind 1 on that layer (st_plan_set_loss_kinds, st_plan_set_layer_loss_kinds) the target is StyleLoss.get_target's (:136-139): srm is stored as the Gram
 * target G_t, mean is not read and no square root runs.
 */
int st_plan_set_style_target(st_plan* plan, int index, const float* mean, const float* srm, void* stream);
/* Scale factors (style_transfer.py:320-322,366,376,429,453): content, 5 style layers, tv.  Default configuration only. */
int st_plan_set_loss_weights(st_plan* plan, float content_weight, const float* style_layer_weights, float tv_weight);

/*
 * closure() (style_transfer.py:472-476): forward, SumLoss, backward to the pixels.
 * grad_out [3][H][W]; losses_out: DEVICE array of 8 floats = 7 weighted terms (SumLoss order) + total.
 */
int st_plan_loss_and_grad(st_plan* plan, const float* image, float* grad_out, float* losses_out, void* stream);

/*
 * One full iteration of the hot loop (style_transfer.py:479-486) on caller-owned state:
 *   closure; torch.optim.Adam single-tensor step (betas, eps as given, no weight decay / amsgrad,
 *   bias corrections in double from `step`, torch/optim/adam.py:414-547); image.clamp_(0,1) (:485);
 *   EMA.update (:250-253) with decay `ema_decay` rounded to fp32.
 * `step` is the 1-based Adam step number of THIS update.  All four tensors are [3][H][W], updated in
 * place.  losses_out as above (may be NULL).
 */
int st_plan_step(st_plan* plan, float* image, float* exp_avg, float* exp_avg_sq, float* ema_value,
                 long long step, double lr, double beta1, double beta2, double eps, double ema_decay,
                 float* losses_out, void* stream);

/*
 * Only the optimiser update of st_plan_step (Adam + clamp + EMA) on an externally supplied gradient
 * (used by the strip-sharded driver, where the closure is run phase by phase).
 */
int st_plan_apply_update(st_plan* plan, float* image, const float* grad, float* exp_avg, float* exp_avg_sq,
                         float* ema_value, long long step, double lr, double beta1, double beta2, double eps,
                         double ema_decay, void* stream);

/*
 * optimizer='lbfgs' (style_transfer.py:464-465, 479-486): torch.optim.LBFGS(params, max_iter=1, history_size=10) with its
 * defaults lr=1, tolerance_grad=1e-7, tolerance_change=1e-9, line_search_fn=None - one quasi-Newton update per call, fixed
 * step length - as three launches and no host decision (csrc/st_lbfgs.hip).  torch/optim/lbfgs.py `step`, case by case:
 *   |g|_inf <= tolerance_grad: return (n_iter is not advanced, nothing of the state moves);
 *   first iteration: d = -g, t = min(1, 1 / |g|_1); afterwards t = 1 and d from the two-loop recursion over the pairs
 *   (y = g - g_prev, s = t d) that passed `ys > 1e-10` (at most 10, oldest dropped), H_diag = ys / y.y of the newest;
 *   g.d > -tolerance_change: d, t and g_prev are recorded, the parameter does not move;   otherwise p.add_(d, alpha=t).
 * The recursion is evaluated on the Gram matrix of [s_i | y_i | g] in double; every launch adds in a fixed order, so a
 * sequence of steps is bit-identical from run to run.
 *
 * State: ONE caller-owned device buffer of st_lbfgs_state_bytes(count) bytes for a parameter of `count` floats, 16-byte
 * aligned (control block, per-workgroup partial sums, 2 * 11 + 1 parameter-sized slots: the ring of pairs with the candidate's
 * spare slot, and g_prev).  A buffer whose first 4096 bytes are zero is a fresh optimiser (st_lbfgs_reset zeroes them on
 * `stream`); the reference makes a new LBFGS per scale (:464-465).  Between the first and the second launch the three new
 * rows of the Gram matrix and |g|_1 are one contiguous block of 70 doubles at byte 192 of the state, |g|_inf the double
 * behind them: when the parameter is cut into strips their place is taken by an all-gather of per-rank records, summed in
 * rank order (st_qn_strip_* below).
 * Alignment: `state` must be 16-byte aligned - st_lbfgs_reset, st_lbfgs_update, st_plan_lbfgs_step and the st_qn_strip_* entries
 * refuse it otherwise; image, grad and ema_value may be merely 4-byte aligned (the scalar kernels then run).
 */
long long st_lbfgs_state_bytes(long long count);
int st_lbfgs_reset(void* state, long long count, void* stream);
/*
 * One LBFGS.step on an externally supplied gradient, then - when ema_value is not NULL - EMA.update(image) (:250-253,
 * decay rounded to fp32 as in st_plan_step); no clamp (:482-483).  The L-BFGS counterpart of st_plan_apply_update.
 * image, grad, ema_value: `count` floats each; grad must stay untouched until the call's last launch has run.
 */
int st_lbfgs_update(void* state, long long count, float* image, const float* grad, float* ema_value, double ema_decay,
                    void* stream);
/*
 * One full iteration of the hot loop for optimizer='lbfgs' (style_transfer.py:472-486): closure, LBFGS.step, EMA.update.
 * The counterpart of st_plan_step; `state` was sized for 3 * H * W floats.  losses_out as in st_plan_loss_and_grad (may be
 * NULL); the loss is the one at the iterate BEFORE the move, as LBFGS.step returns it.
 */
int st_plan_lbfgs_step(st_plan* plan, float* image, void* state, float* ema_value, double ema_decay, float* losses_out,
                       void* stream);
/*
 * Read-back of the optimiser's counters after the work on `stream` has finished (synchronous; tests and diagnostics):
 * n_iter and history = len(old_dirs) of LBFGS's state; of the LAST step: exit_code (0 = moved, 1 = the tolerance_grad
 * return, 2 = the tolerance_change break), accepted (its pair entered the history), t and gtd = g.d.  Any pointer may be NULL.
 */
int st_lbfgs_info(const void* state, long long count, int* n_iter, int* history, int* exit_code, int* accepted, double* t,
                  double* gtd, void* stream);

/*
 * Spatial strip sharding (replaces the reference's 2-device layer split, style_transfer.py:326-333).
 * A strip plan owns image rows [row_begin, row_end) of a global_height x width image; row_begin and
 * row_end must be multiples of 16 (row_end may instead equal global_height).  Its closure is a sequence
 * of compute phases separated by exchanges that the caller performs between st_plan_closure_next calls:
 *   kind 1 (halo): send `count` floats at send_up to the rank above (it receives them at ITS recv_down)
 *                  and send_down to the rank below (ITS recv_up); NULL pointers = no neighbour there (the message is
 *                  one boundary row of every channel plus a 16-float trailer that carries the sender's max |row| for the
 *                  receiver's fp16x3 operand scale - opaque to the transport);
 *   kind 2 (all-reduce): sum `count` floats at `buffer` over all ranks, in place;
 *   kind 4 (reduce): sum `count` floats at `buffer` over all ranks into rank `root`'s buffer (the others' contents
 *                  are undefined afterwards);   kind 5 (broadcast): rank `root`'s `buffer` to every rank;
 *   kind 6 (all-gather): every rank contributes `count` opaque 32-bit words at buffer + rank * count and receives all
 *                  world * count words at `buffer` (in place; the transport copies and does not compute - st_qn_strip_dots
 *                  issues it, the phase machine does not).  The in-library transport issues it on ONE rank too (kinds 2, 4
 *                  and 5 return at once there): one RCCL call per iteration that RCCL turns into the identity, so that a
 *                  one-rank run and st_fabric_selftest execute the call the multi-rank step depends on;
 *   kind 3: nothing to exchange, call again;   kind 0: closure finished.
 * Ordering (ABI version 2): the exchange must be ordered on HIP stream `stream` - behind everything enqueued on it so
 * far, ahead of everything enqueued on it later - or, when `stream` is NULL, on the stream passed to
 * st_plan_closure_next.  The plan's own events tie those streams to the compute stream: a halo exchange travels on a
 * communication stream while the interior rows of the convolution that consumes it are computed (a halo exchange whose
 * consumer is ONE launch has nothing to overlap with and names no stream: it is issued in line, between the kernel that
 * packed the rows and the consumer - round 6), a style head's reduce / broadcast on that head's side stream.  A transport that is not stream-ordered (host-synchronous, or the
 * single-process emulation) may instead complete every exchange before it calls st_plan_closure_next again.
 * `channel`: exchanges on different channels (0 trunk, 1 style heads) must not be serialised against each other by
 * the transport (separate communicators), or a head's broadcast would hold back the trunk's halos.
 * All pointers are device memory owned by the plan, valid until the plan is destroyed.
 */
typedef struct st_exchange {
    int kind;
    long long count;
    float* send_up;
    float* send_down;
    float* recv_up;
    float* recv_down;
    float* buffer;
    int root;
    int channel;
    void* stream;
} st_exchange;
int st_plan_create_strip(st_plan** out, const st_net* net, int global_height, int width, int row_begin,
                         int row_end);
/* Position of this strip among the ranks (default 0 of 1).  With world > 1 each style head's C x C work - covariance,
 * both Newton-Schulz chains (sqrtm.py:9-47), d cov - runs on ONE owner rank ((4 - head) % world) and (Ssym, b, loss
 * term) are broadcast; with world == 1 every plan runs every chain on the all-reduced moments. */
int st_plan_set_rank(st_plan* plan, int rank, int world);
int st_plan_closure_begin(st_plan* plan, const float* image, float* grad_out);
int st_plan_closure_next(st_plan* plan, st_exchange* exchange, void* stream);

/* ---- in-library transport (round 4; csrc/st_fabric.hip): the exchanges of the phase machine issued as RCCL operations by
 * the library itself, on the streams the descriptors name.  Replaces the `.to(devices[i])` transfers of
 * style_transfer.py:87,208 like the descriptor form above, without a Python round trip and a torch.distributed call per
 * exchange, and with the RCCL kernels on the library's own (probed) communication / head streams - c10d launches them on an
 * internal stream that ROCm may deal to the trunk's hardware queue (measured: nothing overlapped).
 * st_fabric_unique_id: 128 opaque bytes from ncclGetUniqueId - call it TWICE on rank 0 (trunk channel, heads' channel)
 * and hand both to every rank (e.g. torch.distributed.broadcast of a byte tensor over any backend).
 * st_fabric_create: ncclCommInitRank of the two communicators (collective over the `world` ranks; the calling thread's
 * current HIP device is the rank's GPU).  self_halo = 1 (world must be 1): the rank is its own upper and lower neighbour -
 * the point-to-point path on one GPU, for tests and measurements.
 * st_plan_closure_run: after st_plan_closure_begin (or st_plan_forward_begin), every remaining phase of the sequence and
 * every exchange between them, enqueued in ONE call; `stream` as in st_plan_closure_next. */
typedef struct st_fabric st_fabric;
int st_fabric_unique_id(unsigned char* id128);
int st_fabric_create(st_fabric** out, const unsigned char* id_trunk128, const unsigned char* id_heads128, int rank, int world,
                     int self_halo);
int st_fabric_destroy(st_fabric* fabric);
/* The same for a fabric whose operations may never complete (a rank left the run early): ncclCommAbort, no waiting. */
int st_fabric_abort(st_fabric* fabric);
/* Pre-flight of a fresh fabric: every operation kind the library issues (neighbour send / recv group, all-reduce, reduce,
 * broadcast, all-gather) once per communicator on 4-float messages with known answers, enqueued on `stream`, awaited on the HOST with a
 * deadline.  0 = the transport works; otherwise st_last_error() says which operation gave what, or that nothing completed
 * within `timeout_ms` (the fabric is then only good for st_fabric_destroy, which aborts its communicators).  Collective:
 * every rank calls it.  No reference counterpart (the reference's `.to(device)` cannot hang). */
int st_fabric_selftest(st_fabric* fabric, void* stream, int timeout_ms);
/* After st_plan_closure_begin (or st_plan_forward_begin): every remaining phase of the plan and every exchange between them,
 * enqueued in one call - the loop over st_plan_closure_next with the exchanges issued on `fabric`.  Operations of one
 * communicator must not run concurrently: the call refuses a stream layout in which the heads' exchanges name different
 * streams (ST_STREAMS_COMPACT=0; use the descriptor form there). */
int st_plan_closure_run(st_plan* plan, st_fabric* fabric, void* stream);
/*
 * The optimizer='lbfgs' step (st_lbfgs_* above) on a parameter that is cut into strips, one per rank (st_qn_*: quasi-Newton).
 * Every rank holds `count` elements of the parameter, of the gradient and of the
 * curvature pairs; what an iteration needs from the other ranks is their share of the 70 sums and the one maximum above,
 * and that is ALL that crosses the fabric: each rank writes a RECORD of 72 doubles (the sums, |g|_inf, padding), one
 * all-gather (exchange kind 6) hands every rank every record, and every rank adds them in rank order in double before
 * its scalar work.  No sum is formed by the transport, so step length, coefficients and the exit taken are bit-identical on
 * all ranks whatever algorithm it uses; no decision is taken on the host.  With world == 1 the step is st_lbfgs_update bit
 * for bit when image, grad and ema_value are 16-byte aligned or count is no multiple of 4: st_qn_strip_dots chooses
 * between the 16-byte and the scalar kernels from count, state and grad alone (it is not handed the other two), so with
 * an aligned grad and a misaligned image or ema_value its partial sums are formed in another order than
 * st_lbfgs_update's scalar pass - equally valid, not bit-identical.
 * State: st_qn_strip_state_bytes(count, world) bytes, 16-byte aligned: the layout of st_lbfgs_state_bytes(count) with
 * `world` records behind it, so st_lbfgs_reset and st_lbfgs_info work on it as they are.  0 for count < 1 or world outside
 * 1 .. 8.
 * st_qn_strip_dots: the first launch on this rank's elements; fills `gather` with the kind-6 exchange the caller must
 * perform (ordered on `stream`) before st_qn_strip_apply: the scalar work and the move (+ EMA.update when ema_value is not
 * NULL) - st_lbfgs_update's second and third launch.  grad must stay untouched until the last launch has run.
 */
long long st_qn_strip_state_bytes(long long count, int world);
int st_qn_strip_dots(void* state, long long count, int rank, int world, const float* grad, st_exchange* gather,
                     void* stream);
int st_qn_strip_apply(void* state, long long count, int world, float* image, const float* grad, float* ema_value,
                      double ema_decay, void* stream);
/* One full optimizer='lbfgs' iteration on a strip, enqueued in ONE call that does not wait for the device - the strips'
 * counterpart of st_plan_lbfgs_step: st_plan_closure_begin(image, grad), st_plan_closure_run, st_qn_strip_dots, an
 * ncclAllGather of the records on the trunk communicator on `stream`, st_qn_strip_apply.  image, grad, ema_value: this
 * rank's [3][rows][W]; `state` sized by st_qn_strip_state_bytes(3 * rows * W, world) with the plan's and the fabric's
 * (equal) rank and world.  The losses are the plan's (st_plan_losses), at the iterate BEFORE the move. */
int st_plan_qn_strip_step(st_plan* plan, st_fabric* fabric, float* image, float* grad, void* state, float* ema_value,
                          double ema_decay, void* stream);
/* Device array of 8 floats (7 weighted terms + total) written by the closure of this plan.  A plan configured with other
 * layers than the reference's (st_plan_set_taps) has another number of terms; there the array - and losses_out of the
 * closure entries - holds [0] the sum of the content terms, [1] the sum of the style terms, [2..5] zero, [6] tv, [7] total. */
int st_plan_losses(st_plan* plan, float** losses);
/* SumLoss's terms (style_transfer.py:455: content losses in list order, style losses in list order, tv), weighted, as the
 * plan's last closure left them: *terms = device array of *count = n_content + n_style + 1 floats, owned by the plan (for
 * the default configuration the first 7 floats of st_plan_losses). */
int st_plan_term_losses(st_plan* plan, float** terms, int* count);
/* Target construction on strips: forward phases only (halo exchanges), then per-layer raw moment sums. */
int st_plan_forward_begin(st_plan* plan, const float* image, int last_layer);
/* Raw (un-normalised) moments of a style tap of this strip: sums[C*C + C] = [F F^T | F 1] over local pixels.
 * All-reduce them and divide by the global pixel count to obtain (srm, mean). */
int st_plan_moment_sums(st_plan* plan, int layer, float* sums, void* stream);

/*
 * The closure's ~430 launches are captured into a hipGraph the second time it is called with the same
 * (image, grad, losses) pointers and replayed afterwards.  Default OFF (measured slower than eager
 * multi-stream launches on ROCm 7.2); 1 = enable, 0 = always launch eagerly.
 */
int st_plan_set_graph(st_plan* plan, int enable);

/*
 * Measurement hooks (bench.py `roofline`): when enabled, every launch of the 3x3 trunk convolution (forward and data
 * gradient; its split-K reduce pass included) is bracketed by hipEvents on its stream.  st_plan_profile_read blocks until the recorded
 * events have completed and returns accumulated {launches, milliseconds, algorithmic FLOPs}.
 */
int st_plan_profile_enable(st_plan* plan, int enable);
int st_plan_profile_read(st_plan* plan, long long* launches, double* millis, double* flops);
/* The same for the step's HBM-bound kernels (bench.py `roofline_hbm`): category 0 conv1_1 forward (+ Normalize),
 * 1 conv1_1 data gradient (+ pad-ring fold), 2 max-pool backward, 3 Adam + clamp + EMA, 4 TV loss + gradient,
 * 5 relu1_1 Gram + mean, 6 content MSE + gradient, 7 the style heads' 1x1 gradient step dF = Ssym F + b (all five taps).
 * Returns {launches, milliseconds, algorithmic bytes} accumulated since
 * the last st_plan_profile_read (call this first: st_plan_profile_read recycles the events). */
int st_plan_profile_read_hbm(st_plan* plan, int category, long long* launches, double* millis, double* bytes);

/* Standalone operators exported for kernel-level parity tests (same code the plan uses). */
/* sqrtm_ns (sqrtm.py:9-25): root[n*n] = NS-12 square root of a[n*n]; n in {64,128,256,512}. */
int st_op_sqrtm_ns(const float* a, float* root, int n, void* stream);
/* _MatrixSquareRootNSLyap.backward (sqrtm.py:36-47): grad_a from root and grad_root. */
int st_op_sqrtm_ns_backward(const float* root, const float* grad_root, float* grad_a, int n, void* stream);
/* The same backward for grad_root = grad_diag * I - the case of StyleLossW2 (style_transfer.py:180: the loss
 * depends on the root through its trace only).  This is the code path the plan runs: the reduced recurrence
 * (the commutator of sqrtm.py:44 vanishes) and, for n = 512, fp16x3 products (csrc/st_nsgemm.hip). */
int st_op_sqrtm_ns_backward_diag(const float* root, float grad_diag, float* grad_a, int n, void* stream);
/* TVLoss (style_transfer.py:187-195) value (device scalar, unweighted) and gradient [3][H][W]. */
int st_op_tv_loss(const float* image, int height, int width, float* loss_out, float* grad_out, void* stream);
/* 3x3 stride-1 zero-padded convolution + bias (+ReLU): the K3/K4 kernel on arbitrary tensors.
 * weight [Cout][Cin][3][3] torch layout (re-laid-out internally, synchronous). Cin % 8 == 0, Cout % 64 == 0. */
int st_op_conv3x3(const float* in, const float* weight, const float* bias, float* out, int cin, int cout,
                  int height, int width, int relu, int precision, void* stream);
/* Data gradient of the same convolution: grad_in[Cin][H][W] from grad_out[Cout][H][W]; if relu_out is
 * non-NULL the incoming gradient is first masked by (relu_out > 0) (threshold_backward). */
int st_op_conv3x3_dgrad(const float* grad_out, const float* relu_out, const float* weight, float* grad_in,
                        int cin, int cout, int height, int width, int precision, void* stream);
/* The same convolution (dgrad == 0: forward with bias / ReLU; dgrad != 0: data gradient, `in` = grad_out with
 * `cout` channels, bias and relu ignored) on a ROW STRIP of a taller tensor, as the strip-sharded plan runs it
 * (SURVEY.md 8(e)): rows -1 and `height` of the operand come from `halo` = [2][C][W] (the neighbour's last row, then
 * the other neighbour's first row; C = the operand's channel count); has_up / has_down == 0 means that side is the
 * global border (zero padding, the halo row is not read). */
int st_op_conv3x3_strip(const float* in, const float* halo, int has_up, int has_down, const float* weight,
                        const float* bias, float* out, int cin, int cout, int height, int width, int relu, int dgrad,
                        int precision, void* stream);
/* The same with the epilogue options of the plan's data-gradient launches - accumulate != 0: out += result (out is
 * read), out_mask (optional [C_out][H][W]): out = out_mask > 0 ? out : 0 afterwards - and, with overlap != 0, in the
 * strip plans' TWO-launch form: the interior rows first (they read no halo row; in a plan the halo exchange is in
 * flight meanwhile), then the first and last rows in one launch behind it (csrc/st_conv_pc.hip, overlap_part).  Fails
 * when the producer / consumer kernel does not take the problem or the strip is too short to cut. */
int st_op_conv3x3_strip_ex(const float* in, const float* halo, int has_up, int has_down, const float* weight,
                           const float* bias, float* out, const float* out_mask, int cin, int cout, int height, int width,
                           int relu, int dgrad, int accumulate, int overlap, int precision, void* stream);

/* 1x1 convolution + bias over [Cin][npix] -> [Cout][npix], weight [Cout][Cin] (no re-layout): the style heads'
 * gradient step dF = Ssym F + b 1^T, i.e. the backward of the einsum / mean in StyleLossW2.get_target
 * (style_transfer.py:162-168).  precision 0 = exact fp32 MFMA, 4 = fp16x3 (operand bounds measured on the
 * device first; the plan gets them from the producing kernels).  Cin % 32 == 0, Cout % 64 == 0.  Synchronous. */
int st_op_conv1x1(const float* in, const float* weight, const float* bias, float* out, int cin, int cout,
                  long long npix, int precision, void* stream);

/* 2x2 / stride-2 pooling of [C][H][W] -> [C][H/2][W/2] (floor mode: a trailing odd row / column is dropped), mode 0 =
 * MaxPool2d(2), 1 = Scale(AvgPool2d(2), 2.0), 2 = Scale(LPPool2d(2, 2), 0.78) (style_transfer.py:21-22,41-46).  The
 * plan's launcher: the 4-wide kernels when W % 4 == 0 and both pointers are 16-byte aligned, else the scalar ones.
 * H, W >= 2. */
int st_op_pool2x2(const float* in, float* out, int channels, int height, int width, int mode, void* stream);
/* Its backward: grad_in [C][H][W] from grad_out [C][H/2][W/2] and the pool's input, masked by (in > 0) (the
 * threshold_backward of the ReLU that produced `in`); the dropped row / column get 0.  The 4-wide kernel also needs
 * an even H. */
int st_op_pool2x2_backward(const float* in, const float* grad_out, float* grad_in, int channels, int height, int width,
                           int mode, void* stream);

/* ==================================================================================================================
 * NATIVE LOSS MODULES - what style_transfer/losses.py runs on an eligible HIP tensor instead of torch kernels: the
 * reference's loss modules (style_transfer.py:93-195) outside any st_plan, inside autograd.  Each entry is the value OR the
 * gradient of one module; the gradient entries take autograd's grad_output as a DEVICE scalar `upstream` (the product of
 * Scale / SumLoss, style_transfer.py:198-221) and never read it on the host.  No float atomics: the same arguments give
 * the same bits.  Every launch goes on `stream`; none of these entries allocates or synchronises, except st_head_create
 * (allocates, synchronises) and st_head_destroy (hipFree synchronises the device).
 * ================================================================================================================== */

/* A standalone style head: StyleLossW2 (kind 0, style_transfer.py:149-181) or StyleLoss (kind 1, :129-142) on a dense
 * [channels][height][width] fp32 tensor that no trunk kernel produced - signed values, all zeros and a single pixel
 * included.  kind 2 is a MOMENTS-ONLY head: st_head_moments alone, none of the workspaces a forward or backward needs.
 * channels in {64, 128, 256, 512}; height, width >= 1; precision 0 = exact fp32 MFMA, 4 = fp16x3 (the codes of
 * st_op_conv1x1; fp16x3 measures max |feat| of the tensor it is given, where a plan gets the bound from the producer).
 * precision governs the two steps that touch the tensor - the Gram moments and the 1x1 step dF = Ssym F + b 1^T; the C x C
 * work is the plan's in every mode (fp32 products and forward chain; for C >= 256 the Lyapunov backward chain in fp16x3,
 * csrc/st_nsgemm.hip).  Of the 1x1 step only a tap with more than 320 workgroups of 64 channels x 128 pixels runs the
 * fp16x3 kernel; smaller ones split K (or take the small-tap kernel) on the exact fp32 MFMA in either mode.
 * The head owns its workspaces - Gram partials, the 1x1 step's split-K scratch, the scaled (Ssym, b) of a backward, the
 * reduction scratch and ticket of a Gram head, the covariance / chain matrices and Newton-Schulz workspace of a W2 head
 * (a Gram head allocates none of those) - allocated here, freed by st_head_destroy, counted by st_head_device_bytes.
 * Calls on one head are ordered by the stream they are given; a head serves one stream at a time.
 * Alignment: feat, state and grad_feat must be 16-byte aligned (st_head_moments, st_head_forward and st_head_backward refuse
 * them otherwise); mean_out, srm_out, loss_out, upstream and the targets may be merely 4-byte aligned. */
typedef struct st_head st_head;
int st_head_create(st_head** out, int kind, int channels, int height, int width, int precision);
int st_head_destroy(st_head* head);
long long st_head_device_bytes(const st_head* head);
/* Floats of the per-call state st_head_forward leaves for st_head_backward: Ssym [C*C] | b [C] | the tensor's fp16x3
 * operand bound.  The caller owns it (autograd: a tensor saved on the node), so a head may run forward any number of
 * times before any backward. */
long long st_head_state_floats(const st_head* head);
/* StyleLossW2.get_target (style_transfer.py:162-168): mean_out [C] (may be NULL) and srm_out [C*C] = F F^T / (h w), exactly
 * symmetric; srm_out alone is StyleLoss.get_target (:135-138).  Either kind of head. */
int st_head_moments(st_head* head, const float* feat, float* mean_out, float* srm_out, void* stream);
/* How st_head_create + st_head_moments split the pixel range of a [channels][npix] tap in `precision` (0 or 4), by the shape and
 * the process's switches alone - no device call: *splits partial Grams (the launch's grid, what the head's workspace is sized
 * for), split s over the pixels [s * *per_split, min((s + 1) * *per_split, npix)) - *per_split is a multiple of 4, so the last
 * splits may be short or empty - and *wide = 1 where the pass runs its 128 x 128-tile kernel (fp16x3 only).  Any output may be
 * NULL.  Refuses the shapes st_head_create refuses. */
int st_op_gram_split_plan(int channels, long long npix, int precision, int* splits, long long* per_split, int* wide);
/* The module's forward, UNWEIGHTED, into loss_out[0] (device).  Targets are read in place - the module's own buffers:
 * kind 0: mean_t [C], cov_t [C*C] (eps I included, :156), root_t [C*C] = sqrtm(cov_t); kind 1: gram_t [C*C]; the other
 * kind's pointers are ignored.  eps: StyleLossW2's covariance eps (:152) or ScaledMSELoss's (:97).  state != NULL: also
 * everything the gradient needs, dF = Ssym F + b 1^T, as (Ssym, b) into `state` (st_head_state_floats floats); NULL (no
 * gradient will be asked for): the Lyapunov chain, the d cov products and (Ssym, b) are skipped.  The sequence is the
 * plan's style head's with weight 1 (csrc/st_closure.hip style_head_chain, csrc/st_taps.hip gram_head). */
int st_head_forward(st_head* head, const float* feat, const float* mean_t, const float* cov_t, const float* root_t,
                    const float* gram_t, float eps, float* loss_out, float* state, void* stream);
/* grad_feat [C][h][w] = upstream[0] * (Ssym F + b 1^T) from the state of a forward on the same `feat`.  upstream is folded
 * into the C x C stage - (Ssym, b) and the fp16x3 bound of Ssym are scaled by one C-workgroup launch - so the tap-sized
 * data is read once and written once, by the 1x1 step. */
int st_head_backward(st_head* head, const float* feat, const float* state, const float* upstream, float* grad_feat,
                     void* stream);

/* Pointwise terms on `count` floats.  Reduction scratch is the CALLER's, per call: `scratch` = st_op_reduce_scratch_floats()
 * floats that nothing else touches until the call's launches have run (two launches: per-workgroup partial sums, then one
 * workgroup adds them in index order; no ticket word, nothing to keep zeroed). */
long long st_op_reduce_scratch_floats(void);
/* nn.MSELoss (ContentLossMSE, style_transfer.py:119-126): loss_out[0] = sum (x - t)^2 / count ... */
int st_op_mse_loss(const float* x, const float* target, long long count, float* scratch, float* loss_out, void* stream);
/* ... and grad[i] = upstream[0] * 2 (x - t)[i] / count. */
int st_op_mse_loss_backward(const float* x, const float* target, long long count, const float* upstream, float* grad,
                            void* stream);
/* ScaledMSELoss (style_transfer.py:93-106; ContentLoss :109-116) with d = x - t: totals[0] = S2 = sum d^2, totals[1] = S1 =
 * sum |d| + eps, loss_out[0] = L = S2 / S1.  The two totals are what the gradient needs (autograd: saved on the node) ... */
int st_op_scaled_mse_loss(const float* x, const float* target, long long count, float eps, float* scratch, float* totals,
                          float* loss_out, void* stream);
/* ... grad[i] = upstream[0] * (2 d - L sgn d)[i] / S1, sgn 0 = 0: where every d is zero the gradient is zero, not NaN. */
int st_op_scaled_mse_loss_backward(const float* x, const float* target, long long count, const float* totals,
                                   const float* upstream, float* grad, void* stream);
/* The diagonal W2 head of st_plan_set_w2_diagonal on ONE dense fp32 tensor feat [C][npix], any C >= 1 (at most 65535) and
 * npix >= 1, at weight 1 and without a mask, by the same kernels.  `scratch`: st_op_channel_stats_scratch_floats(C, npix)
 * floats of the caller's, per call (16 bytes for the last-block ticket, which the call zeroes, and two partials per channel
 * and split of the pixel range; the split count depends on npix alone).  Two calls on the same data give the same bits. */
long long st_op_channel_stats_scratch_floats(int channels, long long npix);
/* mean_out[c] = sum_p f_cp / npix, srm_diag_out[c] = sum_p f_cp^2 / npix: the diagonal of StyleLossW2.get_target's second raw
 * moment, linear in the statistics like it. */
int st_op_channel_moments(const float* feat, int channels, long long npix, float* scratch, float* mean_out, float* srm_diag_out,
                          void* stream);
/* loss_out[0] = (sum_c (mu_c - mean_t[c])^2 + sum_c (sigma_c - std_t[c])^2) / C with sigma_c = sqrt(max(q_c - mu_c^2, 0) + eps);
 * coeffs_out [2 C] = [a | b], what the gradient needs (autograd: saved on the node) ... */
int st_op_w2_diag_loss(const float* feat, int channels, long long npix, const float* mean_t, const float* std_t, float eps,
                       float* scratch, float* coeffs_out, float* loss_out, void* stream);
/* ... grad[c][p] = upstream[0] * (a_c f_cp + b_c); upstream: a DEVICE scalar. */
int st_op_w2_diag_loss_backward(const float* feat, int channels, long long npix, const float* coeffs, const float* upstream,
                                float* grad, void* stream);
/* The marginal W2 head of st_plan_set_w2_marginal on ONE dense fp32 tensor feat [C][n], by the same kernels: C >= 1 rows of
 * 1 <= n <= 2^32 - 1 elements; a shape that needs more than 2^31 - 1 workgroups in one launch is refused, never wrapped.
 * st_op_sort_chunk(): the keys one workgroup sorts in LDS (a row of at most that many elements needs no merge pass).
 * `scratch`: st_op_sort_scratch_bytes(C, n) bytes of the caller's, 256-byte aligned, per call.
 * st_op_channel_sort: per row the stable ascending order of feat + 0.0f - sorted_out [C][n] the values, perm_out [C][n] the
 * element indices; either may be null.  Two calls on the same data give the same bits.
 * Alignment: `scratch` must be 256-byte aligned (64-bit keys lie behind its header) - st_op_channel_sort and
 * st_op_w2_marginal_loss refuse it otherwise; every tensor pointer may be merely 4-byte aligned. */
int st_op_sort_chunk(void);
long long st_op_sort_scratch_bytes(int channels, long long n);
int st_op_channel_sort(const float* feat, int channels, long long n, void* scratch, float* sorted_out, unsigned int* perm_out,
                       void* stream);
/* out [C][n_out] = the quantile functions q [C][n_in] at the n_out midpoints (st_plan_set_w2_marginal's target formula). */
int st_op_resample_quantiles(const float* q, int channels, long long n_in, long long n_out, float* out, void* stream);
/* loss_out[0] = sum_c sum_k (f_c,pi_c(k) - target_c,k)^2 / (C n) at weight 1, target [C][n] with sorted rows;
 * unit_grad_out [C][n] = d loss / d feat (autograd: saved on the node) ... */
int st_op_w2_marginal_loss(const float* feat, int channels, long long n, const float* target, void* scratch, float* unit_grad_out,
                           float* loss_out, void* stream);
/* ... grad[i] = upstream[0] * unit_grad[i], i < count; upstream: a DEVICE scalar. */
int st_op_w2_marginal_loss_backward(const float* unit_grad, long long count, const float* upstream, float* grad, void* stream);
/* The nearest head of st_plan_set_style_nearest on ONE dense fp32 tensor feat [C][n], by the same kernels: C a multiple of
 * st_op_nearest_k_chunk() (32), n >= 1 pixels against m >= 1 style vectors.  st_op_nearest_pixel_tile() / _k_tile(): the pixels a
 * workgroup owns and the style vectors of one k tile (128 each); st_op_nearest_splits(n, m): the splits of the k range, by the
 * shape alone.
 * st_op_nearest_prepare: vectors [C][m] -> prepared, st_op_nearest_prepared_floats(C, m) floats of the caller's, 256-byte aligned:
 * S^T, the bias, the bound on max |S|.
 * `scratch`: st_op_nearest_scratch_floats(C, n, m) floats of the caller's, 256-byte aligned, per call.
 * st_op_nearest_search: idx_out [n] = k*(i), score_out [n] (optional) = <f_i, s_k*> - |s_k*|^2 / 2 as the search saw it.
 * Two calls on the same data give the same bits.
 * Alignment: `prepared` and `scratch` must be 256-byte aligned - st_op_nearest_prepare, st_op_nearest_search and
 * st_op_nearest_loss refuse them otherwise; vectors, feat and every output may be merely 4-byte aligned. */
int st_op_nearest_k_chunk(void);
int st_op_nearest_pixel_tile(void);
int st_op_nearest_k_tile(void);
int st_op_nearest_splits(long long n, long long m);
long long st_op_nearest_prepared_floats(int channels, long long m);
long long st_op_nearest_scratch_floats(int channels, long long n, long long m);
int st_op_nearest_prepare(const float* vectors, int channels, long long m, float* prepared, void* stream);
int st_op_nearest_search(const float* feat, int channels, long long n, const float* prepared, long long m, float* scratch, int* idx_out,
                         float* score_out, void* stream);
/* loss_out[0] = sum_i |f_i - s_k*(i)|^2 / (C n) at weight 1; idx_out [n] the matches; unit_grad_out [C][n] = d loss / d feat
 * (autograd: saved on the node) ... */
int st_op_nearest_loss(const float* feat, int channels, long long n, const float* prepared, long long m, float* scratch, int* idx_out,
                       float* unit_grad_out, float* loss_out, void* stream);
/* The cosine (centered = 0) and centred-cosine (centered = 1) metrics of st_plan_set_nearest_metric on ONE dense fp32 tensor, by
 * the same kernels and for the same shapes: C a multiple of 32, n >= 1 pixels against m >= 1 style vectors, n and m at most
 * st_max_pixels() (refused before any work).  st_op_nearest_cosine_prepare: vectors [C][m] -> prepared,
 * st_op_nearest_cosine_prepared_floats(C, m) floats of the caller's: L2's layout with the unit rows, b and the bound on max |s^|,
 * then mu [C] padded to 64 floats - so st_op_nearest_search runs on it as on an L2 one and serves all three metrics (its score
 * is then <f_i, s^_k*> + b_k*).  `scratch`: st_op_nearest_cosine_scratch_floats(C, n, m) floats, per call.
 * st_op_nearest_cosine_loss: loss_out[0] = sum_i (1 - p_i(k*(i)) / r_i) / n at weight 1; idx_out [n] the matches;
 * unit_grad_out [C][n] = d loss / d feat.  st_op_nearest_loss_backward serves the backward.  Two calls give the same bits.
 * Alignment: `prepared` and `scratch` must be 256-byte aligned (refused otherwise); every other buffer may be merely 4-byte
 * aligned. */
long long st_op_nearest_cosine_prepared_floats(int channels, long long m);
long long st_op_nearest_cosine_scratch_floats(int channels, long long n, long long m);
int st_op_nearest_cosine_prepare(const float* vectors, int channels, long long m, int centered, float* prepared, void* stream);
int st_op_nearest_cosine_loss(const float* feat, int channels, long long n, const float* prepared, long long m, float* scratch,
                              int* idx_out, float* unit_grad_out, float* loss_out, void* stream);
/* ... grad[i] = upstream[0] * unit_grad[i], i < count; upstream: a DEVICE scalar. */
int st_op_nearest_loss_backward(const float* unit_grad, long long count, const float* upstream, float* grad, void* stream);
/* The sliced head of st_plan_set_style_sliced on ONE dense fp32 tensor feat [C][n], by the same kernels: C a multiple of 32, P a
 * multiple of 64 in [64, 512], rows of 1 to 2^24 - 1 elements.  The directions are ARGUMENTS - r [P][C] and its transpose
 * rt [C][P], both layouts of the 1x1 step - so a caller's own work as well as st_op_sliced_directions' (rows of at most unit
 * length are not required: max |r| is measured).  Both products run in fp16x3 with max |feat|, max |r| and max |G| measured on the
 * device (the option ST_SLICED_FP32 = 1: on the exact fp32 MFMA).
 * st_op_sliced_directions: r_out [P][C], rt_out [C][P] of (seed, entry, epoch), the generator written down above.
 * `scratch`: st_op_sliced_scratch_bytes(C, P, n) bytes of the caller's, 256-byte aligned, per call, n the longest row of the call
 * (st_op_sliced_target: max(m, n_out)).
 * st_op_sliced_target: one style image's share, target [P][n_out] = (accumulate ? target : 0) + weight resample_n_out(sort_rows(r feat)),
 * feat [C][m].  Two calls on the same data give the same bits.
 * Alignment: `scratch` must be 256-byte aligned - st_op_sliced_target, st_op_sliced_project and st_op_sliced_loss refuse it
 * otherwise; feat, r, rt, target and every output may be merely 4-byte aligned (a product whose operands are not 16-byte
 * aligned runs on the exact fp32 MFMA instead of the fp16x3 kernel). */
int st_op_sliced_directions(unsigned long long seed, int entry, unsigned long long epoch, int projections, int channels, float* r_out,
                            float* rt_out, void* stream);
long long st_op_sliced_scratch_bytes(int channels, int projections, long long n);
int st_op_sliced_target(const float* feat, int channels, long long m, const float* r, const float* rt, int projections, long long n_out,
                        void* scratch, float* target, int accumulate, float weight, void* stream);
/* y_out [P][n] = r feat, bit for bit the projection st_op_sliced_loss sorts (the same launch under the same measured bounds): its
 * stable order is the permutation the gradient goes through, which can differ from the float64 order of r feat at near-ties. */
int st_op_sliced_project(const float* feat, int channels, long long n, const float* r, const float* rt, int projections, void* scratch,
                         float* y_out, void* stream);
/* loss_out[0] = sum_p sum_k (Y_p,pi_p(k) - target_p,k)^2 / (P n) at weight 1, Y = r feat, target [P][n] with sorted rows;
 * unit_grad_out [C][n] = d loss / d feat = (2 / (P n)) rt G (autograd: saved on the node) ... */
int st_op_sliced_loss(const float* feat, int channels, long long n, const float* r, const float* rt, int projections, const float* target,
                      void* scratch, float* unit_grad_out, float* loss_out, void* stream);
/* ... grad[i] = upstream[0] * unit_grad[i], i < count; upstream: a DEVICE scalar. */
int st_op_sliced_loss_backward(const float* unit_grad, long long count, const float* upstream, float* grad, void* stream);
/* TVLoss (style_transfer.py:184-195) on a [3][H][W] image, H, W >= 1: the value alone (st_op_tv_loss writes the unit
 * gradient with it) ... */
int st_op_tv_value(const float* image, int height, int width, float* scratch, float* loss_out, void* stream);
/* ... and grad [3][H][W] = upstream[0] * d TVLoss / d image. */
int st_op_tv_loss_backward(const float* image, int height, int width, const float* upstream, float* grad, void* stream);
/* The closure's ONE-launch forms of the content MSE and TV terms (value and gradient in the launch that streams the data;
 * the last workgroup by ticket adds the per-workgroup partial sums in index order), by the plan's own kernels:
 *   st_op_mse_term:  loss_out[0] = weight sum (x - t)^2 / count, grad_out[i] = weight 2 (x - t)[i] / count; x, target and
 *                    grad_out 16-byte aligned
 *   st_op_tv_term:   loss_out[0] = weight TVLoss(image), grad_out [3][H][W] = weight d TVLoss / d image
 * `scratch`: st_op_reduce_scratch_floats() floats of the caller's; `ticket`: ONE device word of the caller's that is zero
 * before the first call - every call leaves it zero, so calls on one stream may share scratch and ticket back to back.
 * ST_LAST_BLOCK_FENCE (st_set_option) chooses how the partial sums are handed to the last workgroup; the bits do not depend
 * on it. */
int st_op_mse_term(const float* x, const float* target, long long count, float weight, float* scratch, unsigned int* ticket,
                   float* loss_out, float* grad_out, void* stream);
int st_op_tv_term(const float* image, int height, int width, float weight, float* scratch, unsigned int* ticket, float* loss_out,
                  float* grad_out, void* stream);
/* The Laplacian loss of st_plan_set_laplacian for ONE pool size on a [C][H][W] image, C >= 1, at weight 1, by the same
 * kernels.  `scratch`: st_op_laplacian_scratch_floats(C, H, W, pool) floats of the caller's, per call.  The target
 * [C][H / pool][W / pool] = L(Q(image)) ... */
long long st_op_laplacian_scratch_floats(int channels, int height, int width, int pool);
int st_op_laplacian_target(const float* image, int channels, int height, int width, int pool, float* scratch, float* target_out,
                           void* stream);
/* ... the value loss_out[0] = sum r^2 / (C h w) with the residual r = L(Q(image)) - target written to residual_out [C][h][w]
 * (autograd: saved on the node) ... */
int st_op_laplacian_value(const float* image, const float* target, int channels, int height, int width, int pool, float* scratch,
                          float* residual_out, float* loss_out, void* stream);
/* ... and grad [C][H][W] = upstream[0] * d value / d image from that residual: zero in the dropped trailing rows and columns. */
int st_op_laplacian_backward(const float* residual, int channels, int height, int width, int pool, const float* upstream,
                             float* grad, void* stream);

/* ==================================================================================================================
 * MEASUREMENT AIDS - not part of the drop-in surface (no reference counterpart; a binding of the reference does not
 * need them).  They time the product's own kernels in isolation for tools/ and profiles/: st_op_sqrtm_time,
 * st_op_conv3x3_time, st_op_mfma_rate, st_op_mfma_valu_rate, st_op_grid_barrier_time (and the st_plan_profile_* hooks
 * above, which bench.py's `roofline` uses).
 * ================================================================================================================== */

/* Microbenchmark of the two 12-step recurrences on an n x n SPD matrix (workspace preallocated, HIP events
 * on `stream`): average microseconds per full sqrtm_ns forward chain and per Lyapunov backward chain. */
int st_op_sqrtm_time(int n, int iters, double* fwd_us, double* bwd_us, void* stream);

/* Kernel microbenchmark: average microseconds of `iters` back-to-back launches of the convolution
 * (forward if dgrad == 0, masked data gradient otherwise) on device-resident random operands, timed with
 * HIP events on `stream`; same launch path (tile choice, split-K) as the plan uses. */
int st_op_conv3x3_time(int cin, int cout, int height, int width, int dgrad, int precision, int iters,
                       double* avg_us, void* stream);

/* Measurement aid (csrc/st_diag.hip), no reference counterpart: the rate the 16-bit matrix pipe sustains on this
 * chip under the consumer pattern of the XL convolution tile - one persistent workgroup of `waves` waves per CU, every
 * wave `steps` times {lds_reads (0, 4 or 8) ds_read_b128 operand fetches; 12 v_mfma_f32_32x32x16_f16} - as
 * TFLOP/s (HIP events over `launches` launches on `stream`) and the shader clock it held (MHz).  The roofline in
 * bench.py is quoted against the nominal 2.5 PFLOP/s; this is the measured ceiling next to it. */
int st_op_mfma_rate(int lds_reads, int waves, int steps, int launches, double* tflops, double* mhz, void* stream);

/* The same with `valu_waves` extra waves per CU that execute nothing but fp32 VALU work (32 v_fma_f32 per step,
 * `valu_steps` steps; valu_prio bit 1: at s_setprio 3, bit 2: as the workgroup's first = oldest waves) - the position of the convolution tile's staging waves.  cycles[0] =
 * shader cycles per VALU instruction that wave achieved beside the MFMA streams, cycles[1] = cycles per MFMA of an MFMA
 * wave. */
int st_op_mfma_valu_rate(int lds_reads, int waves, int steps, int launches, int valu_waves, int valu_steps,
                         int valu_prio, double* tflops, double* mhz, double* cycles, void* stream);

/* Measurement aid (csrc/st_diag.hip, profiles/r05_winograd.md), no reference counterpart: the 16-bit matrix rate (TFLOP/s of
 * executed MFMA work) a CU sustains in the consumer pattern of a Winograd F(2x2, 3x3) fp16x3 tile - four waves per CU, per step
 * 16 ds_read_b128 of fresh operands for 12 v_mfma_f32_32x32x16_f16 (0.75 MFMAs per read; the shipped direct tile: 1.5). */
int st_op_winograd_consumer_rate(int steps, int launches, double* tflops, void* stream);

/* Diagnostic (tests/test_tv_hazard_gpu.py), no reference counterpart: after a device synchronise, copy `count` floats of an
 * internal buffer of the plan to the host.  what = 0: the TV kernels' per-workgroup partial sums (4 floats per workgroup:
 * the sums of squares of D1 .. D4 of style_transfer.py:189-192, tv_interior_kernel's workgroups first).
 *
 * what = 2 (tests/test_operand_bounds_gpu.py), count = 64: the plan's 64 fp16x3 operand bounds, one float per bound word - the
 * maximum over the word's slots, reinterpreted as a float, which is what a consumer scales its fp16 planes by (only the
 * exponent counts: the consumer assumes max |operand| < 2^(floor(log2 b) + 1)).  A word no launch has raised reads 0.
 *     words  0 .. 12   max |y| of the 13 convolutions' ReLU outputs (relu1_1 ... relu5_1)
 *     words 16 .. 28   max |g| of the gradients of those outputs, as staged: already multiplied by the ReLU mask
 *     words 32 .. 35   max |g| of the gradients of the 4 pooled maps
 *     words 48 .. 63   the style heads' bounds on their C x C matrix Ssym: the j-th listed style layer owns word 48 + j
 *     every other word is unused and reads 0
 * Two sharing rules: a pooled map has no y word of its own, its consumer reads the word of the convolution that feeds the pool
 * (average and L2 pooling may exceed that bound by less than one binade, which the fp16 scale leaves spare); and a convolution
 * that feeds a pool has no g word of its own, its gradient is bounded by that pool's word (32 .. 35), which therefore covers
 * both tensors - words 17, 19, 23 and 27 are never written.  The bounds are those of the LAST pass: a forward clears
 * all 64 at its start, a backward the g words at its start; st_plan_step and st_plan_lbfgs_step clear all 64 in their tail
 * for the next pass, so read them after st_plan_forward, st_plan_backward or st_plan_loss_and_grad, not after a step.
 *
 * what = 16 + i, i = 0 .. 16, count = C h w of that map: the gradient map of the i-th of the 17 taps in network order (relu1_1,
 * relu1_2, pool1, relu2_1, ...) as the last backward or closure left it - the tensor its g word bounds. */
int st_plan_debug_read(st_plan* plan, int what, float* out, int count);

/* Measurement aid (csrc/st_diag.hip), no reference counterpart: microseconds per round of `rounds` device-wide barriers
 * inside ONE launch of `workgroups` co-resident workgroups (<= the CU count), each round writing `payload_floats` floats
 * per workgroup before the barrier and checking another workgroup's (another XCD's) after it; *errors counts stale reads.
 * groups = 0: one counter for all workgroups; groups = G: two levels (workgroup w arrives at group w % G, the last of a
 * group at the top counter, release through per-group flags) - the form the persistent Newton-Schulz chain kernel uses. */
int st_op_grid_barrier_time(int workgroups, int rounds, int payload_floats, int groups, double* us_per_round, int* errors,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ST_AMD_H */
