// The fp16x3 mode's dynamic-range guards: the weights-only one at st_net_create and the activation-aware one of
// st_plan_range_guard, with the networks' bf16x6 planes they switch layers to.
#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

#include "st_plan.h"

using namespace st;

namespace {

// ST_CONV_RANGE_GUARD=0: neither guard (a network's layers stay in the arithmetic it was created with)
bool range_guard_on() {
    static Option opt("ST_CONV_RANGE_GUARD", 1);
    return opt.get() != 0;
}

// ---- activation-aware dynamic-range guard of the fp16x3 mode (round 4) ----------------------------------------------------
// The weights-only heuristic (range_guard) cannot see a DATA-dependent low-energy operand: channels that a particular
// image drives orders of magnitude below the tensor's maximum (dead-ish ReLU channels, which a trained VGG-19 has) sit at
// the bottom of fp16x3's one-scale-per-tensor window.  So the decision is measured on the image itself, once per scale,
// on the cold path: every unflagged trunk convolution is evaluated in bf16x6 (three bf16 planes, 8-bit exponents, no
// scale) on exactly the operand the shipped pass feeds it, and compared with what the shipped arithmetic produced -
// forward on the maps of a plain forward pass, data gradient on the gradients of one closure (same forward, same heads:
// the Newton-Schulz chains would amplify any forward difference, so the two modes never see different inputs).  A layer
// whose results differ by more than 1e-5 rel-L2 over the map, or on any output channel by more than 16 x what the exact-
// fp32 MFMA kernel differs there (range_mismatch), is flagged for that direction: it runs bf16x6 from then on (sticky, per network: merged with st_net_wide_layers; half the
// matrix rate on that layer).  After a flag the pass is repeated, because later layers then see different operands.
// Zero cost in the hot loop; the seeded synthetic weights flag nothing.
__global__ __launch_bounds__(256) void range_diff_kernel(const float* __restrict__ test, const float* __restrict__ exact,
                                                         const float* __restrict__ ref, long long per_channel,
                                                         float* __restrict__ sums) {
    // channel c = blockIdx.y, block b = blockIdx.x: sums[(c gridDim.x + b) 3 + {0, 1, 2}] = this block's sums of (test - ref)^2,
    // (exact - ref)^2, ref^2 - per-block partials that the host adds up in index order (float atomics from up to 64 blocks made
    // a score near 1.0 flip from run to run, and with it the arithmetic of the whole trajectory: ADVICE r4)
    __shared__ float scratch[4];
    const size_t base = (size_t)blockIdx.y * per_channel;
    float d2 = 0.f, x2 = 0.f, r2 = 0.f;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < per_channel; i += (long long)gridDim.x * 256) {
        const float r = ref[base + i], d = test[base + i] - r, x = exact[base + i] - r;
        d2 += d * d;
        x2 += x * x;
        r2 += r * r;
    }
    d2 = block_sum_256(d2, scratch);
    x2 = block_sum_256(x2, scratch);
    r2 = block_sum_256(r2, scratch);
    if (threadIdx.x == 0) {
        float* mine = sums + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3;
        mine[0] = d2; mine[1] = x2; mine[2] = r2;
    }
}
constexpr int kRangeBlocks = 64;                           // blocks per channel of range_diff_kernel (at most)
constexpr size_t kRangeSumFloats = (size_t)3 * 512 * kRangeBlocks;

// How far is `test` (the shipped fp16x3 result) from `ref` (bf16x6), measured (a) over the whole map against 1e-5 rel-L2
// and (b) per output channel against what the EXACT-fp32 MFMA kernel's own distance from bf16x6 is on that channel - the
// rounding noise any fp32-class arithmetic carries there, cancellation-dominated channels included.  A channel of tiny
// magnitude matters as much as any other when the next layer's weights for it are large, so (b) has no energy cut-off: a
// channel is off when its fp16x3 deviation exceeds 16 x the fp32 kernel's AND 2e-6 of its own norm.  score > 1: flag.
int range_mismatch(const float* test, const float* exact, const float* ref, int channels, long long per_channel,
                   float* dev_sums, hipStream_t s, double* score, double* map_rel) {
    ST_REQUIRE(channels <= 512, "range guard: more than 512 channels");
    const int bx = (int)std::min<long long>((per_channel + 255) / 256, kRangeBlocks);
    hipLaunchKernelGGL(range_diff_kernel, dim3(bx, channels), dim3(256), 0, s, test, exact, ref, per_channel, dev_sums);
    ST_LAUNCH_CHECK();
    std::vector<float> part((size_t)3 * channels * bx);
    ST_HIP(hipMemcpyAsync(part.data(), dev_sums, part.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    ST_HIP(hipStreamSynchronize(s));
    std::vector<double> h((size_t)3 * channels, 0.0);      // the blocks of a channel in index order: the same verdict every run
    for (int c = 0; c < channels; ++c)
        for (int b = 0; b < bx; ++b)
            for (int k = 0; k < 3; ++k) h[3 * c + k] += part[((size_t)c * bx + b) * 3 + k];
    double d2 = 0, r2 = 0;
    for (int c = 0; c < channels; ++c) { d2 += h[3 * c]; r2 += h[3 * c + 2]; }
    const double whole = r2 > 0 ? std::sqrt(d2 / r2) : 0.0;
    double worst = whole / 1e-5;
    for (int c = 0; c < channels; ++c) {
        const double dt = h[3 * c], dx = h[3 * c + 1], e = h[3 * c + 2];
        if (!(e > 0) || !(dt > 0)) continue;
        const double allowed = 256.0 * dx + 4e-12 * e;             // (16 x the fp32 kernel's deviation)^2 + (2e-6 |ref_c|)^2
        worst = std::max(worst, std::sqrt(dt / allowed));
    }
    *score = worst;
    *map_rel = whole;
    return 0;
}

int ensure_wide_planes(st_net* net, int conv, bool dgrad) {
    void*& slot = dgrad ? net->wsx_bwd[conv] : net->wsx_fwd[conv];
    if (slot) return 0;
    const OpDesc* op = nullptr;
    for (const OpDesc& o : kProgram)
        if (o.kind == 0 && o.index == conv) op = &o;
    ST_REQUIRE(op && net->w_torch[conv], "range guard: the network keeps no source weights for conv %d", conv);
    ST_HIP(hipMalloc(&slot, split_weight_bytes(op->cin, op->cout, 3)));
    if (launch_relayout_split(net->w_torch[conv], slot, op->cin, op->cout, dgrad ? 1 : 0, 3, 0, nullptr)) return 1;
    ST_HIP(hipDeviceSynchronize());
    return 0;
}

// the shipped launch of an unflagged layer (forward_conv / dgrad_conv), written to `out` in the guard's `mode`: 1 as
// shipped (fp16x3), 0 bf16x6 on the `wide` planes, 2 exact fp32; never a bound of the plan's nodes
void guard_mode(ConvProblem& c, int mode, void* wide, float* out) {
    c.out = out;
    c.out_amax = nullptr;
    if (mode == 1) return;
    c.wgt_split = mode == 0 ? wide : nullptr;
    c.planes = mode == 0 ? 3 : 0;
    c.elem = 0;
    c.amax_word = nullptr;
}

int plan_range_guard(st_plan* p, const float* image, hipStream_t s, int* new_fwd, int* new_bwd) {
    st_net* net = const_cast<st_net*>(p->net);                    // (flags and planes are added under the lock below)
    for (int i = 0; i < 13; ++i) new_fwd[i] = new_bwd[i] = 0;
    if (net->conv_elem != 1 || net->conv_planes != 2 || !range_guard_on() || p->strip) return 0;
    static std::mutex guard;
    std::lock_guard<std::mutex> lock(guard);
    if (ensure_grad_alloc(p) || ensure_streams(p, s)) return 1;
    const bool log = option_env("ST_RANGE_LOG") != nullptr;
    // three maps of the largest activation + the partial sums: allocated ONCE per plan (the guard runs several times per scale)
    // and owned by it - freed with the plan on every path, an error in the middle of this function included
    // (keyed on the LAST allocation: a call that failed half-way is repeated from the first missing buffer - advisor, round 5.
    // The three maps stay resident with the plan - 4.8 GB at 2896 x 2172, counted in st_plan_device_bytes.)
    if (!p->guard_sums) {
        size_t biggest = 0;
        for (const Node& n : p->conv) biggest = std::max(biggest, n.count());
        for (int k = 0; k < 3; ++k)
            if (!p->guard_scratch[k] && plan_alloc(p, &p->guard_scratch[k], biggest)) return 1;
        if (plan_alloc(p, &p->guard_sums, kRangeSumFloats)) return 1;
    }
    float *alt = p->guard_scratch[0], *cur = p->guard_scratch[1], *exact = p->guard_scratch[2], *sums = p->guard_sums;
    int rc = 0;
    auto finish = [&](int code) { return code; };

    // ---- forward: the maps of a plain forward pass (every map written: no argmax codes, no fused-pool-only layers) ----
    for (int pass = 0; pass < 13 && rc == 0; ++pass) {
        if (run_forward(p, image, 29, s)) return finish(1);
        bool flagged = false;
        for (int i = 0; i < kNumOps && !flagged; ++i) {
            const OpDesc& op = kProgram[i];
            const Node& n = node_at(p, i);
            if (op.kind == 0 && op.index > 0 && !net->wide_fwd[op.index]) {
                if (ensure_wide_planes(net, op.index, false)) return finish(1);
                // (pre-activations: with the ReLU in place a nearly dead channel differs between any two arithmetics in WHICH
                // pixels survive, and the per-channel comparison would flag rounding noise)
                for (int mode = 0; mode < 3; ++mode) {
                    ConvProblem c{};
                    forward_conv(p, i, c);
                    c.relu = 0;
                    guard_mode(c, mode, net->wsx_fwd[op.index], mode == 1 ? cur : (mode == 2 ? exact : alt));
                    if (launch_conv(c, s)) return finish(1);
                }
                double score = 0, whole = 0;
                if (range_mismatch(cur, exact, alt, n.c, (long long)n.h * n.w, sums, s, &score, &whole)) return finish(1);
                if (log) fprintf(stderr, "[range] forward conv %2d: fp16x3 vs bf16x6 rel-L2 %.2e, score %.2f\n", op.index, whole, score);
                if (score > 1.0) {
                    net->wide_fwd[op.index] = net->guard_fwd[op.index] = new_fwd[op.index] = 1;
                    flagged = true;
                }
            }
        }
        if (!flagged) break;
    }
    if (!targets_ready(p)) return finish(0);

    // ---- data gradients: the gradients of one closure; both arithmetics on the same operand ----
    int lowest_checked = 13;                                       // layers >= this index are settled
    for (int pass = 0; pass < 13; ++pass) {
        if (closure_eager(p, image, p->grad_img, nullptr, s)) return finish(1);
        ST_HIP(hipStreamSynchronize(s));
        bool flagged = false;
        // (a configured plan's closure stops at its deepest layer: no gradient exists above it)
        for (int i = closure_top_op(p); i >= 0 && !flagged; --i) {
            const OpDesc& op = kProgram[i];
            if (op.kind != 0 || op.index == 0 || op.index >= lowest_checked) continue;
            const Node& in = node_at(p, i - 1);
            if (net->wide_bwd[op.index]) { lowest_checked = op.index; continue; }
            if (ensure_wide_planes(net, op.index, true)) return finish(1);
            for (int mode = 0; mode < 3; ++mode) {
                ConvProblem c{};
                dgrad_conv(p, i, c);
                c.mask = nullptr; c.out_mask = nullptr; c.accumulate = 0;
                guard_mode(c, mode, net->wsx_bwd[op.index], mode == 1 ? cur : (mode == 2 ? exact : alt));
                if (launch_conv(c, s)) return finish(1);
            }
            double score = 0, whole = 0;
            if (range_mismatch(cur, exact, alt, in.c, (long long)in.h * in.w, sums, s, &score, &whole)) return finish(1);
            if (log) fprintf(stderr, "[range] data gradient of conv %2d: fp16x3 vs bf16x6 rel-L2 %.2e, score %.2f\n", op.index, whole, score);
            if (score > 1.0) {
                net->wide_bwd[op.index] = net->guard_bwd[op.index] = new_bwd[op.index] = 1;
                flagged = true;                                    // shallower layers now see another gradient: again
            }
            lowest_checked = op.index;
        }
        if (!flagged) break;
    }
    return finish(0);
}

}  // namespace

namespace st {

// Dynamic-range guard of the fp16x3 mode.  Two fp16 planes under ONE power-of-two scale per tensor keep 22 bits only
// for elements within ~28 binades of the tensor's maximum.  A network may carry feature-map channels that are orders of
// magnitude smaller than their neighbours and are multiplied by correspondingly LARGE weights (any per-channel rescaling
// of a ReLU network is function-preserving, and trained VGG-19s are not normalised): those products matter as much as the
// others but their operands sit at the bottom of the window (tests/test_hot_path_gpu.py,
// test_closure_with_six_decades_of_channel_scales: content term off by 6e-3).  Only the weights are known here, and
// such compensation shows in them: an input channel (forward) / output channel (data gradient) whose largest weight lies
// far above the layer's MEDIAN channel.  Layers flagged that way run bf16x6 (conv_split_kernel, three bf16 planes, half
// the matrix rate of fp16x3, no scale).  ST_CONV_RANGE_GUARD=0 disables the guard, ST_CONV_RANGE_LOG2 (default 8) is the
// max / median ratio, as a power of two, beyond which a layer is flagged.
int range_guard(st_net* net, int conv, const float* weight_dev, int cin, int cout) {
    static Option log2_opt("ST_CONV_RANGE_LOG2", 8);
    if (!range_guard_on()) return 0;
    const size_t wcount = (size_t)cout * cin * 9;
    std::vector<float> w(wcount);
    ST_HIP(hipMemcpy(w.data(), weight_dev, wcount * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<float> by_in(cin, 0.f), by_out(cout, 0.f);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < 9; ++t) {
                const float a = std::fabs(w[((size_t)co * cin + ci) * 9 + t]);
                by_in[ci] = std::max(by_in[ci], a);
                by_out[co] = std::max(by_out[co], a);
            }
    auto spread = [](std::vector<float> v) {
        std::sort(v.begin(), v.end());
        const float med = v[v.size() / 2];
        return med > 0.f ? v.back() / med : 0.f;
    };
    const float limit = std::ldexp(1.f, log2_opt.get());
    net->wide_fwd[conv] = spread(by_in) > limit;
    net->wide_bwd[conv] = spread(by_out) > limit;
    const size_t bytes = split_weight_bytes(cin, cout, 3);
    if (net->wide_fwd[conv]) {
        ST_HIP(hipMalloc(&net->wsx_fwd[conv], bytes));
        if (launch_relayout_split(weight_dev, net->wsx_fwd[conv], cin, cout, 0, 3, 0, nullptr)) return 1;
    }
    if (net->wide_bwd[conv]) {
        ST_HIP(hipMalloc(&net->wsx_bwd[conv], bytes));
        if (launch_relayout_split(weight_dev, net->wsx_bwd[conv], cin, cout, 1, 3, 0, nullptr)) return 1;
    }
    return 0;
}

}  // namespace st

extern "C" {

int st_net_wide_layers(const st_net* net, int* forward13, int* backward13) {
    ST_REQUIRE(net && forward13 && backward13, "st_net_wide_layers: null argument");
    for (int i = 0; i < 13; ++i) {
        forward13[i] = net->wide_fwd[i];
        backward13[i] = net->wide_bwd[i];
    }
    return 0;
}

int st_net_mark_wide(st_net* net, const int* forward13, const int* backward13) {
    ST_REQUIRE(net && forward13 && backward13, "st_net_mark_wide: null argument");
    if (net->conv_elem != 1 || net->conv_planes != 2) return 0;          // only fp16x3 networks have a second arithmetic
    for (int i = 1; i < 13; ++i) {
        if (forward13[i] && !net->wide_fwd[i]) {
            if (ensure_wide_planes(net, i, false)) return 1;
            net->wide_fwd[i] = net->guard_fwd[i] = 1;
        }
        if (backward13[i] && !net->wide_bwd[i]) {
            if (ensure_wide_planes(net, i, true)) return 1;
            net->wide_bwd[i] = net->guard_bwd[i] = 1;
        }
    }
    return 0;
}

int st_plan_range_guard(st_plan* p, const float* image, int* forward13, int* backward13, void* stream) {
    ST_REQUIRE(p && image && forward13 && backward13, "st_plan_range_guard: null argument");
    return plan_range_guard(p, image, static_cast<hipStream_t>(stream), forward13, backward13);
}

}  // extern "C"
