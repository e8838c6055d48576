// C ABI of libst_amd.so (include/st_amd.h): error text, runtime switches, and the handles - networks, plans, targets,
// weights, one optimiser iteration.  No autograd: the closure (st_closure.hip, strip plans: st_strip.hip) and the Adam +
// clamp + EMA update are explicit kernel launches on the caller's stream.
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "st_plan.h"

namespace st {

static thread_local std::string g_error;
void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
}
const char* get_error() { return g_error.c_str(); }

// runtime switches (st_common.h): overrides set through st_set_option win over the environment
static std::mutex g_option_mutex;
static std::vector<std::pair<std::string, int>> g_option_override;
static std::atomic<unsigned> g_option_gen{1};
unsigned option_generation() { return g_option_gen.load(std::memory_order_relaxed); }
int option_lookup(const char* name, int dflt) {
    {
        std::lock_guard<std::mutex> lock(g_option_mutex);
        for (const auto& kv : g_option_override)
            if (kv.first == name) return kv.second;
    }
    const char* v = option_env(name);
    return (v && *v) ? atoi(v) : dflt;
}
// The switches a default build reads from the environment (documented in tools/README.md; tests/test_abi_cpu.py compares the
// two lists).  Everything else is an A/B or diagnostic switch: st_set_option only, or any build with --experiments.
static const char* const kEnvSwitches[] = {
    "ST_AMD_TIMELINE",      // time stamps of the closure's phases
    "ST_STREAM_LOG",        // the stream / hardware-queue layout the probe chose
    "ST_RANGE_LOG",         // what the activation-aware range guard measured
    "ST_CONV_RANGE_GUARD",  // 0: no weights-only range guard at st_net_create
    "ST_CONV_RANGE_LOG2",   // its threshold (log2 of the channel gain that flags a layer)
    "ST_NS_F16",            // 0: every Newton-Schulz chain on the fp32 matrix pipe
    "ST_GRAM_F32",          // 1: Gram matrices on the fp32 matrix pipe
    "ST_HEAD_1X1_F32",      // 1: the heads' 1 x 1 gradient step on the fp32 matrix pipe
    "ST_STRIP_OVERLAP",     // strip plans: 0 never / 1 by the cost model / 2 always split a convolution for halo overlap
    "ST_STRIP_OVERLAP_US",  // ... the exchange latency the split may cost
    "ST_STRIP_SPARE_CUS",   // ... CUs left free for RCCL's point-to-point kernels beside an interior launch
    "ST_STRIP_NS_OWNER",    // ... the rank that owns relu5_1's chains
    "ST_STREAM_PROBE",      // 0: skip the hardware-queue probe (fixed stream layout)
};
const char* option_env(const char* name) {
    if (!kExperiments) {
        bool listed = false;
        for (const char* k : kEnvSwitches) listed = listed || strcmp(k, name) == 0;
        if (!listed) return nullptr;
    }
    return getenv(name);
}
static void option_set(const char* name, int value, bool clear) {
    std::lock_guard<std::mutex> lock(g_option_mutex);
    for (size_t i = 0; i < g_option_override.size(); ++i)
        if (g_option_override[i].first == name) {
            if (clear) g_option_override.erase(g_option_override.begin() + i);
            else g_option_override[i].second = value;
            g_option_gen.fetch_add(1);
            return;
        }
    if (!clear) g_option_override.emplace_back(name, value);
    g_option_gen.fetch_add(1);
}

namespace {
// the update's host-side scalars exactly as torch computes them (Python doubles; torch/optim/adam.py:476-547)
AdamScalars adam_scalars(long long step, double lr, double beta1, double beta2, double eps, double ema_decay) {
    const double bc1 = 1.0 - std::pow(beta1, (double)step);
    const double bc2 = 1.0 - std::pow(beta2, (double)step);
    AdamScalars sc{};
    sc.lerp_w = (float)(1.0 - beta1);
    sc.beta2 = (float)beta2;
    sc.one_m_beta2 = (float)(1.0 - beta2);
    sc.step_size = (float)(lr / bc1);
    sc.bc2_sqrt = (float)std::sqrt(bc2);
    sc.eps = (float)eps;
    sc.decay = (float)ema_decay;             // torch.tensor(decay): fp32 buffer (style_transfer.py:243)
    sc.one_m_decay = 1.0f - sc.decay;        // (1 - self.decay) evaluated in fp32 (:253)
    return sc;
}
}  // namespace
}  // namespace st

using namespace st;

// =================================================================================================
extern "C" {

const char* st_last_error(void) { return st::get_error(); }
int st_abi_version(void) { return ST_AMD_ABI_VERSION; }
const char* st_compiled_arch(void) { return "gfx950"; }
long long st_max_pixels(void) { return st::kMaxPixels; }
int st_has_experiments(void) { return st::kExperiments ? 1 : 0; }
int st_env_switches(const char** names, int capacity) {
    const int n = (int)(sizeof(st::kEnvSwitches) / sizeof(st::kEnvSwitches[0]));
    for (int i = 0; i < n && i < capacity; ++i) names[i] = st::kEnvSwitches[i];
    return n;
}
int st_set_option(const char* name, int value, int clear) {
    ST_REQUIRE(name && name[0] == 'S' && name[1] == 'T' && name[2] == '_', "st_set_option: switch names start with ST_");
    st::option_set(name, value, clear != 0);
    return 0;
}

static int net_fill(st_net* net, const float* const* weights, const float* const* biases);

int st_net_create(st_net** out, const float* const* weights, const float* const* biases, int pooling) {
    return st_net_create_ex(out, weights, biases, pooling, 0);
}

int st_net_create_ex(st_net** out, const float* const* weights, const float* const* biases, int pooling,
                     int conv_precision) {
    ST_REQUIRE(out && weights && biases, "st_net_create: null argument");
    ST_REQUIRE(pooling >= 0 && pooling <= 2, "st_net_create: unknown pooling %d", pooling);
    ST_REQUIRE(conv_precision_valid(conv_precision),
               "st_net_create: conv_precision must be 0 (fp32), 2 (bf16x3), 3 (bf16x6) or 4 (fp16x3)");
    st_net* net = new st_net();
    net->pooling = pooling;
    net->conv_planes = conv_precision_planes(conv_precision);
    net->conv_elem = conv_precision_elem(conv_precision);
    if (net_fill(net, weights, biases)) {      // error text already set; release what was allocated so far
        st_net_destroy(net);
        return 1;
    }
    *out = net;
    return 0;
}

static int net_fill(st_net* net, const float* const* weights, const float* const* biases) {
    int conv = 0;
    for (int i = 0; i < kNumOps; ++i) {
        const OpDesc& op = kProgram[i];
        if (op.kind != 0) continue;
        const size_t wcount = (size_t)op.cout * op.cin * 9;
        ST_HIP(hipMalloc(&net->bias[conv], op.cout * sizeof(float)));
        ST_HIP(hipMemcpy(net->bias[conv], biases[conv], op.cout * sizeof(float), hipMemcpyDeviceToDevice));
        if (conv == 0) {
            ST_HIP(hipMalloc(&net->w_first, wcount * sizeof(float)));
            ST_HIP(hipMemcpy(net->w_first, weights[0], wcount * sizeof(float), hipMemcpyDeviceToDevice));
            std::vector<float> hw(wcount), hb(op.cout);
            ST_HIP(hipMemcpy(hw.data(), weights[0], wcount * sizeof(float), hipMemcpyDeviceToHost));
            ST_HIP(hipMemcpy(hb.data(), biases[0], op.cout * sizeof(float), hipMemcpyDeviceToHost));
            for (int co = 0; co < op.cout; ++co) {
                float l1 = 0.f;
                for (int k = 0; k < 27; ++k) l1 += std::fabs(hw[(size_t)co * 27 + k]);
                net->w_first_l1max = std::max(net->w_first_l1max, l1);
                net->b_first_max = std::max(net->b_first_max, std::fabs(hb[co]));
            }
        } else {
            ST_HIP(hipMalloc(&net->w_fwd[conv], wcount * sizeof(float)));
            ST_HIP(hipMalloc(&net->w_bwd[conv], wcount * sizeof(float)));
            if (launch_relayout_fwd(weights[conv], net->w_fwd[conv], op.cin, op.cout, nullptr)) return 1;
            if (launch_relayout_dgrad(weights[conv], net->w_bwd[conv], op.cin, op.cout, nullptr)) return 1;
            if (net->conv_planes > 0) {
                const size_t bytes = split_weight_bytes(op.cin, op.cout, net->conv_planes);
                ST_HIP(hipMalloc(&net->ws_fwd[conv], bytes));
                ST_HIP(hipMalloc(&net->ws_bwd[conv], bytes));
                if (launch_relayout_split(weights[conv], net->ws_fwd[conv], op.cin, op.cout, 0, net->conv_planes,
                                          net->conv_elem, nullptr) ||
                    launch_relayout_split(weights[conv], net->ws_bwd[conv], op.cin, op.cout, 1, net->conv_planes,
                                          net->conv_elem, nullptr))
                    return 1;
                if (net->conv_elem == 1) {
                    ST_HIP(hipMalloc(&net->w_torch[conv], wcount * sizeof(float)));
                    ST_HIP(hipMemcpy(net->w_torch[conv], weights[conv], wcount * sizeof(float), hipMemcpyDeviceToDevice));
                    if (range_guard(net, conv, weights[conv], op.cin, op.cout)) return 1;
                }
            }
        }
        ++conv;
    }
    ST_HIP(hipDeviceSynchronize());
    return 0;
}

int st_net_destroy(st_net* net) {
    if (!net) return 0;
    hipFree(net->w_first);
    for (int i = 0; i < 13; ++i) {
        hipFree(net->bias[i]);
        hipFree(net->w_fwd[i]);
        hipFree(net->w_bwd[i]);
        hipFree(net->ws_fwd[i]);
        hipFree(net->ws_bwd[i]);
        hipFree(net->wsx_fwd[i]);
        hipFree(net->wsx_bwd[i]);
        hipFree(net->w_torch[i]);
    }
    delete net;
    return 0;
}

static size_t moment_floats(const StyleHead& h) { return (size_t)h.n * h.n + h.n; }      // [F F^T | F 1]

static int plan_create_common(st_plan** out, const st_net* net, int local_height, int width, int global_height,
                              int row0, bool strip_mode) {
    st_plan* p = new st_plan();
    p->net = net;
    p->H = local_height;
    p->W = width;
    p->Hg = global_height;
    p->dp_parts = conv_first_dgrad_parts(global_height, width);
    p->row0 = row0;
    p->strip = strip_mode;
    p->has_up = p->strip && row0 > 0;
    p->has_down = p->strip && row0 + local_height < global_height;
    int h = local_height, w = width, hg = global_height;
    for (int i = 0; i < kNumOps; ++i) {
        const OpDesc& op = kProgram[i];
        Node& n = node_at(p, i);
        if (op.kind == 1) { h /= 2; w /= 2; hg /= 2; }
        n.c = op.cout; n.h = h; n.w = w; n.hg = hg;
        if (plan_alloc(p, &n.y, n.count())) { st_plan_destroy(p); return 1; }
        if (p->strip) {
            const bool feeds_conv = (i + 1 < kNumOps) && kProgram[i + 1].kind == 0;
            if (feeds_conv && halo_alloc(p, &n.yhalo, (size_t)2 * n.c * n.w)) { st_plan_destroy(p); return 1; }
            if (op.kind == 0 && halo_alloc(p, &n.ghalo, (size_t)2 * n.c * n.w)) { st_plan_destroy(p); return 1; }
        }
    }
    // convs whose output only the following max pool consumes (relu1_2, 2_2, 3_4, 4_4): in the closure their epilogue
    // leaves the pooled map + one code byte per window instead of the full-resolution map
    for (int i = 0; i + 1 < kNumOps; ++i) {
        if (kProgram[i].kind != 0 || kProgram[i + 1].kind != 1 || net->pooling != 0) continue;
        Node& n = p->conv[kProgram[i].index];
        if (n.h % 2 != 0 || n.w % 4 != 0) continue;
        float* mem = nullptr;
        if (plan_alloc(p, &mem, ((size_t)n.c * (n.h / 2) * (n.w / 2) + 3) / 4)) { st_plan_destroy(p); return 1; }
        n.pool_code = reinterpret_cast<unsigned char*>(mem);
    }
    for (int op = 0; op < kNumOps; ++op) {
        const Node& tap = node_at(p, op);
        p->head[op].n = tap.c;
        p->head[op].npix = (long long)tap.hg * tap.w;
        p->head[op].npix_local = (long long)tap.h * tap.w;
    }
    float* ticket_mem = nullptr;
    if (plan_alloc(p, &ticket_mem, 256) || hipMemset(ticket_mem, 0, 256 * sizeof(float)) != hipSuccess) {
        st_plan_destroy(p);
        return 1;
    }
    p->tickets = reinterpret_cast<unsigned int*>(ticket_mem);
    if (plan_alloc(p, &p->losses, 64) || plan_alloc(p, &p->red_partials, 5 * kStreamBlocks) ||
        plan_alloc(p, &p->conv_scratch, kConvScratchFloats) ||
        plan_alloc(p, &p->dp_scratch, (size_t)3 * (local_height + 2) * (width + 2) * p->dp_parts) || plan_alloc(p, &p->amax_word, (size_t)64 * kAmaxWordUints) ||
        plan_alloc(p, &p->content_target[p->content_op[0]], node_at(p, p->content_op[0]).count())) {
        st_plan_destroy(p);
        return 1;
    }
    {
        unsigned int* words = reinterpret_cast<unsigned int*>(p->amax_word);
        for (int i = 0; i < kNumOps; ++i) {
            const OpDesc& op = kProgram[i];
            if (op.kind == 0) {
                p->conv[op.index].y_amax = words + (size_t)op.index * kAmaxWordUints;
                p->conv[op.index].g_amax = words + (size_t)(16 + op.index) * kAmaxWordUints;
            } else {
                Node& src = p->conv[kProgram[i - 1].index];          // a pool always follows a conv
                p->pool[op.index].y_amax = src.y_amax;
                p->pool[op.index].g_amax = words + (size_t)(32 + op.index) * kAmaxWordUints;
                src.g_amax = p->pool[op.index].g_amax;
            }
        }
    }
    assign_head_bounds(p);
    if (p->strip) {
        float* hb = nullptr;
        if (plan_alloc(p, &hb, kAmaxWordUints)) { st_plan_destroy(p); return 1; }
        p->halo_bound = reinterpret_cast<unsigned int*>(hb);
        float* ps = nullptr;
        if (halo_alloc(p, &p->img_halo, (size_t)6 * width) || plan_alloc(p, &p->send_up, (size_t)64 * width + kHaloTrailer) ||
            plan_alloc(p, &p->send_down, (size_t)64 * width + kHaloTrailer) || plan_alloc(p, &p->lossbuf, 64) ||
            plan_alloc(p, &ps, kPackScratchUints)) {
            st_plan_destroy(p);
            return 1;
        }
        p->pack_scratch = reinterpret_cast<unsigned int*>(ps);
        if (hipMemset(ps, 0, kPackScratchUints * sizeof(unsigned int)) != hipSuccess ||
            hipMemset(p->send_up, 0, ((size_t)64 * width + kHaloTrailer) * sizeof(float)) != hipSuccess ||
            hipMemset(p->send_down, 0, ((size_t)64 * width + kHaloTrailer) * sizeof(float)) != hipSuccess) {
            set_error("hipMemset of the halo send buffers failed");
            st_plan_destroy(p);
            return 1;
        }
        // raw moment sums of the five heads in ONE block: a single all-reduce per closure
        size_t total = 0;
        for (int k = 0; k < p->n_style; ++k) total += moment_floats(p->head[p->style_op[k]]);
        float* block = nullptr;
        if (plan_alloc(p, &block, total)) { st_plan_destroy(p); return 1; }
        p->gram_total = (long long)total;
        for (int k = 0; k < p->n_style; ++k) {
            const size_t floats = moment_floats(p->head[p->style_op[k]]);
            p->gram_raw[k] = block;
            block += floats;
            if (plan_alloc(p, &p->head_result[k], floats + 64)) {
                st_plan_destroy(p);
                return 1;
            }
        }
    }
    *out = p;
    return 0;
}

int st_plan_create(st_plan** out, const st_net* net, int height, int width) {
    ST_REQUIRE(out && net, "st_plan_create: null argument");
    // VGGFeatures.forward size check for taps up to features[29] (style_transfer.py:61-69,81-83)
    ST_REQUIRE(height >= 16 && width >= 16, "Input is %dx%d but must be at least 16x16", height, width);
    ST_REQUIRE_PIXELS("st_plan_create", (long long)height * width);
    return plan_create_common(out, net, height, width, height, 0, false);
}

int st_plan_create_strip(st_plan** out, const st_net* net, int global_height, int width, int row_begin,
                         int row_end) {
    ST_REQUIRE(out && net, "st_plan_create_strip: null argument");
    ST_REQUIRE(global_height >= 16 && width >= 16, "Input is %dx%d but must be at least 16x16", global_height,
               width);
    ST_REQUIRE(row_begin >= 0 && row_end > row_begin && row_end <= global_height, "strip rows out of range");
    ST_REQUIRE(row_begin % 16 == 0 && (row_end % 16 == 0 || row_end == global_height),
               "strip boundaries must be multiples of 16 rows (all four 2x2 poolings stay strip-local)");
    ST_REQUIRE(row_end - row_begin >= 16, "a strip needs at least 16 rows");
    ST_REQUIRE_PIXELS("st_plan_create_strip (the strip)", (long long)(row_end - row_begin) * width);
    return plan_create_common(out, net, row_end - row_begin, width, global_height, row_begin, true);
}

int st_plan_destroy(st_plan* p) {
    if (!p) return 0;
    for (void* a : p->allocations) hipFree(a);
    for (ProfileEvent& e : p->events) {
        hipEventDestroy(e.start);
        hipEventDestroy(e.stop);
    }
    for (HbmEvent& e : p->hbm_events) {
        hipEventDestroy(e.start);
        hipEventDestroy(e.stop);
    }
    invalidate_graph(p);
    if (p->streams_ready) {
        if (p->main_stream) { hipStreamSynchronize(p->main_stream); hipStreamDestroy(p->main_stream); }
        for (hipStream_t j : p->junk_streams) hipStreamDestroy(j);
        hipEventDestroy(p->bridge_in);
        hipEventDestroy(p->bridge_out);
        if (p->aux_stream) { hipStreamSynchronize(p->aux_stream); hipStreamDestroy(p->aux_stream); }
        for (int i = 0; i < 5; ++i)
            if (p->head_stream[i]) {
                hipStreamSynchronize(p->head_stream[i]);
                if (p->head_stream_owned[i]) hipStreamDestroy(p->head_stream[i]);
            }
        for (hipEvent_t e : {p->aux_in, p->aux_fwd, p->tv_done, p->content_done})
            if (e) hipEventDestroy(e);
        for (int i = 0; i < 5; ++i) {
            hipEventDestroy(p->moments_ready[i]);
            hipEventDestroy(p->chain_done[i]);
            hipEventDestroy(p->tap_ready[i]);
            hipEventDestroy(p->head_done[i]);
        }
    }
    if (p->comm_stream) {
        hipStreamSynchronize(p->comm_stream);
        if (!p->comm_stream_borrowed) hipStreamDestroy(p->comm_stream);
        hipEventDestroy(p->pack_done);
        hipEventDestroy(p->halo_landed);
    }
    delete p;
    return 0;
}

long long st_plan_device_bytes(const st_plan* p) { return p ? p->bytes : 0; }

int st_plan_forward(st_plan* p, const float* image, int last_layer, void* stream) {
    ST_REQUIRE(p && image, "st_plan_forward: null argument");
    ST_REQUIRE(last_layer >= 1 && last_layer <= 29, "st_plan_forward: last_layer %d out of range", last_layer);
    if (run_forward(p, image, last_layer, static_cast<hipStream_t>(stream))) return 1;
    p->fwd_last_layer = last_layer;
    return 0;
}

int st_plan_backward(st_plan* p, int count, const int* layers, const float* const* grads, float* grad_image, void* stream) {
    ST_REQUIRE(p, "st_plan_backward: null plan");
    ST_REQUIRE(!p->strip, "st_plan_backward: strip plans are not supported (a strip's backward needs its neighbours' halo rows)");
    ST_REQUIRE(count >= 1, "st_plan_backward: count is %d, at least one tap gradient is needed", count);
    ST_REQUIRE(layers && grads && grad_image, "st_plan_backward: null argument");
    ST_REQUIRE(p->fwd_last_layer > 0,
               "st_plan_backward: no st_plan_forward is current on this plan (none has run, or a closure - st_plan_loss_and_grad, "
               "st_plan_step, ... - has run since and left pooling codes instead of maps): run st_plan_forward first");
    const float* seed[kNumOps] = {};
    for (int k = 0; k < count; ++k) {
        const int at = tap_position(layers[k]);
        ST_REQUIRE(at >= 0, "st_plan_backward: features[%d] is not a ReLU or pooling output", layers[k]);
        ST_REQUIRE(layers[k] <= p->fwd_last_layer, "st_plan_backward: features[%d] lies beyond the last forward's last_layer %d",
                   layers[k], p->fwd_last_layer);
        ST_REQUIRE(seed[at] == nullptr, "st_plan_backward: features[%d] is named twice", layers[k]);
        ST_REQUIRE(grads[k] != nullptr, "st_plan_backward: null gradient for features[%d]", layers[k]);
        seed[at] = grads[k];
    }
    if (ensure_grad_alloc(p)) return 1;
    return run_tap_backward(p, seed, grad_image, static_cast<hipStream_t>(stream));
}

int st_plan_feature(const st_plan* p, int layer, const float** data, int* channels, int* height, int* width) {
    ST_REQUIRE(p && data, "st_plan_feature: null argument");
    const int op = tap_position(layer);
    ST_REQUIRE(op >= 0, "st_plan_feature: features[%d] is not a ReLU or pooling output", layer);
    const Node* n = &node_at(p, op);
    *data = n->y;
    if (channels) *channels = n->c;
    if (height) *height = n->h;
    if (width) *width = n->w;
    return 0;
}

int st_plan_moments(st_plan* p, int layer, float* mean_out, float* srm_out, void* stream) {
    ST_REQUIRE(p && mean_out && srm_out, "st_plan_moments: null argument");
    const int op = tap_position(layer);
    ST_REQUIRE(op >= 0, "st_plan_moments: features[%d] is not a ReLU or pooling output", layer);
    int j = -1;
    for (int k = 0; k < p->n_style; ++k)
        if (p->style_op[k] == op) j = k;
    ST_REQUIRE(j >= 0 || !p->strip, "st_plan_moments: strip plans take the reference's style layers only");
    // the workspace of the position's head; a layer of the reference's lists: the default closure's head of that index, whose
    // Gram conv1_1's launch may have left (run_forward)
    HeadSite at;
    at.h = &p->head[op];
    at.tap = &node_at(p, op);
    if (j >= 0 && p->reference_taps) at = head_site(p, j);
    mask_head_site(p, at, op);       // (a style mask in force: the weighted moments, st_plan_set_style_mask)
    if (ensure_moment_alloc(p, *at.h)) return 1;
    return moments_of_tap(p, at, mean_out, srm_out, static_cast<hipStream_t>(stream));
}

int st_plan_set_content_target(st_plan* p, const float* feat, void* stream) {
    return st_plan_set_content_target_at(p, 0, feat, stream);
}

int st_plan_set_style_target(st_plan* p, int index, const float* mean, const float* srm, void* stream) {
    ST_REQUIRE(p && mean && srm, "st_plan_set_style_target: null argument");
    ST_REQUIRE(index >= 0 && index < p->n_style, "st_plan_set_style_target: index %d out of range (%d style layers)", index,
               p->n_style);
    return st_plan_set_region_style_target(p, 0, index, mean, srm, stream);
}

int st_plan_set_region_style_target(st_plan* p, int region, int index, const float* mean, const float* srm, void* stream) {
    ST_REQUIRE(p && mean && srm, "st_plan_set_region_style_target: null argument");
    ST_REQUIRE(region >= 0 && region < std::max(p->n_regions, 1),
               "st_plan_set_region_style_target: region %d out of range (%d style regions are set: st_plan_set_style_regions)", region,
               p->n_regions);
    ST_REQUIRE(index >= 0 && index < p->n_style, "st_plan_set_region_style_target: index %d out of range (%d style layers)", index,
               p->n_style);
    ST_REQUIRE(!p->style_marg[index],
               "st_plan_set_style_target: style layer %d is flagged marginal (st_plan_set_w2_marginal): its target is a quantile function, "
               "set by st_plan_set_style_quantiles", index);
    ST_REQUIRE(!p->style_near[index],
               "st_plan_set_style_target: style layer %d is flagged nearest (st_plan_set_style_nearest): its target is a set of style vectors, "
               "set by st_plan_set_style_vectors", index);
    ST_REQUIRE(!p->style_sliced[index],
               "st_plan_set_style_target: style layer %d is flagged sliced (st_plan_set_style_sliced): its target is derived from the style "
               "images' feature vectors, set by st_plan_set_style_sliced_vectors", index);
    hipStream_t s = static_cast<hipStream_t>(stream);
    StyleHead& h = region_head_at(p, region, p->style_op[index]);
    if (ensure_style_alloc(p, h, alloc_kind_of(p, index))) return 1;
    if (p->style_diag[index]) {         // a diagonal W2 entry (st_plan_set_w2_diagonal): (mu_t, sigma_t) from srm's diagonal; no root
        if (launch_diag_target(mean, srm, h.n, style_eps_of(p, index), h.diag_mean_t, h.diag_std_t, s)) return 1;
        h.target_set = true;
        return 0;
    }
    if (p->style_kind[index] == 1) {    // StyleLoss.get_target (:136-139): the second raw moment IS the Gram target; no root
        ST_HIP(hipMemcpyAsync(h.gram_t, srm, (size_t)h.n * h.n * sizeof(float), hipMemcpyDeviceToDevice, s));
        h.target_set = true;
        return 0;
    }
    ST_HIP(hipMemcpyAsync(h.mean_t, mean, h.n * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (launch_cov_from_moments(mean, srm, h.cov_t, h.n, style_eps_of(p, index), s)) return 1;
    if (ns_sqrt_forward(h.cov_t, h.root_t, h.n, h.ns, s)) return 1;
    h.target_set = true;
    return 0;
}

int st_plan_set_style_quantiles(st_plan* p, int index, const float* q, long long n_q, void* stream) {
    ST_REQUIRE(p && q, "st_plan_set_style_quantiles: null argument");
    ST_REQUIRE(index >= 0 && index < p->n_style, "st_plan_set_style_quantiles: index %d out of range (%d style layers)", index, p->n_style);
    ST_REQUIRE(!p->style_near[index], "st_plan_set_style_quantiles: style layer %d is flagged nearest (st_plan_set_style_nearest): its target "
               "is set by st_plan_set_style_vectors", index);
    ST_REQUIRE(!p->style_sliced[index], "st_plan_set_style_quantiles: style layer %d is flagged sliced (st_plan_set_style_sliced): its target "
               "is set by st_plan_set_style_sliced_vectors", index);
    ST_REQUIRE(p->style_marg[index], "st_plan_set_style_quantiles: style layer %d is not flagged marginal (st_plan_set_w2_marginal): its "
               "target is set by st_plan_set_style_target", index);
    ST_REQUIRE(n_q >= 1, "st_plan_set_style_quantiles: %lld order statistics per channel: at least one", n_q);
    StyleHead& h = p->head[p->style_op[index]];
    if (ensure_style_alloc(p, h, 3)) return 1;
    if (launch_resample_quantiles(q, h.n, n_q, h.npix_local, h.marg_t, static_cast<hipStream_t>(stream))) return 1;
    h.target_set = true;
    return 0;
}

int st_plan_style_quantiles(st_plan* p, int index, float** target, int* channels, long long* n) {
    ST_REQUIRE(p && target && channels && n, "st_plan_style_quantiles: null argument");
    ST_REQUIRE(index >= 0 && index < p->n_style, "st_plan_style_quantiles: index %d out of range (%d style layers)", index, p->n_style);
    const StyleHead& h = p->head[p->style_op[index]];
    ST_REQUIRE(p->style_marg[index] && h.target_set && h.marg_t,
               "st_plan_style_quantiles: style layer %d holds no quantile target (st_plan_set_w2_marginal, st_plan_set_style_quantiles)", index);
    *target = h.marg_t;
    *channels = h.n;
    *n = h.npix_local;
    return 0;
}

int st_plan_set_style_vectors(st_plan* p, int index, const float* feat, long long m, void* stream) {
    ST_REQUIRE(p && feat, "st_plan_set_style_vectors: null argument");
    ST_REQUIRE(index >= 0 && index < p->n_style, "st_plan_set_style_vectors: index %d out of range (%d style layers)", index, p->n_style);
    ST_REQUIRE(!p->style_sliced[index], "st_plan_set_style_vectors: style layer %d is flagged sliced (st_plan_set_style_sliced): its target "
               "is set by st_plan_set_style_sliced_vectors", index);
    ST_REQUIRE(p->style_near[index], "st_plan_set_style_vectors: style layer %d is not flagged nearest (st_plan_set_style_nearest): its "
               "target is set by st_plan_set_style_target", index);
    StyleHead& h = p->head[p->style_op[index]];
    if (nearest_check_shape("st_plan_set_style_vectors", h.n, h.npix_local, m)) return 1;
    // (a closure in flight may still read the former set: the buffers are rewritten behind it on the caller's stream)
    // the entry holds no target until the new set is written
    h.target_set = false;
    invalidate_graph(p);
    const int metric = p->style_near_metric[index];      // (st_plan_set_nearest_metric: the buffers and the prepare pass go by it)
    if (alloc_head_nearest(h, m, PlanAlloc{p}, metric)) return 1;
    ST_HIP(hipStreamSynchronize(nullptr));
    const NearestPrepared pr = nearest_prepared_of(h.near_prep, h.n, m);
    if (metric ? launch_nearest_cosine_prepare(feat, h.n, m, metric == 2, pr, static_cast<hipStream_t>(stream))
               : launch_nearest_prepare(feat, h.n, m, pr, static_cast<hipStream_t>(stream)))
        return 1;
    h.near_m = m;
    h.target_set = true;
    return 0;
}

int st_plan_nearest_indices(st_plan* p, int index, const int** idx, long long* n) {
    ST_REQUIRE(p && idx && n, "st_plan_nearest_indices: null argument");
    ST_REQUIRE(index >= 0 && index < p->n_style, "st_plan_nearest_indices: index %d out of range (%d style layers)", index, p->n_style);
    const StyleHead& h = p->head[p->style_op[index]];
    ST_REQUIRE(p->style_near[index] && h.target_set && h.near_idx,
               "st_plan_nearest_indices: style layer %d holds no matches (st_plan_set_style_nearest, st_plan_set_style_vectors)", index);
    *idx = h.near_idx;
    *n = h.npix_local;
    return 0;
}

int st_plan_set_style_sliced_vectors(st_plan* p, int index, int n_images, const float* const* feats, const long long* ms,
                                     const float* weights, void* stream) {
    ST_REQUIRE(p && feats && ms, "st_plan_set_style_sliced_vectors: null argument");
    ST_REQUIRE(index >= 0 && index < p->n_style, "st_plan_set_style_sliced_vectors: index %d out of range (%d style layers)", index,
               p->n_style);
    ST_REQUIRE(p->style_sliced[index], "st_plan_set_style_sliced_vectors: style layer %d is not flagged sliced (st_plan_set_style_sliced): "
               "its target is set by st_plan_set_style_target", index);
    ST_REQUIRE(n_images >= 1, "st_plan_set_style_sliced_vectors: %d style images: at least one", n_images);
    StyleHead& h = p->head[p->style_op[index]];
    const int proj = sliced_projections_of(p, index);
    // the images that enter: those of weight > 0 (a null list: every image, equal weights), their weights over their sum
    int kept[kSlicedMaxImages] = {};
    int n_kept = 0;
    long long total = 0, rows = h.npix_local;
    double sum = 0.0;
    for (int i = 0; i < n_images; ++i) {
        const float w = weights ? weights[i] : 1.f;
        ST_REQUIRE(w >= 0.f && w <= 3.0e38f, "st_plan_set_style_sliced_vectors: weight %g of style image %d: finite and not negative", (double)w, i);
        if (w == 0.f) continue;
        ST_REQUIRE(feats[i], "st_plan_set_style_sliced_vectors: null feature vectors for style image %d", i);
        ST_REQUIRE(n_kept < kSlicedMaxImages, "st_plan_set_style_sliced_vectors: more than %d style images of weight > 0", kSlicedMaxImages);
        if (sliced_check_shape("st_plan_set_style_sliced_vectors", h.n, proj, ms[i])) return 1;
        kept[n_kept++] = i;
        total += ms[i];
        rows = std::max(rows, ms[i]);
        sum += (double)w;
    }
    ST_REQUIRE(n_kept >= 1, "st_plan_set_style_sliced_vectors: every style image has weight 0");
    if (sliced_check_shape("st_plan_set_style_sliced_vectors", h.n, proj, h.npix_local)) return 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // (a closure in flight may still read the former set: the buffers are rewritten behind it on the caller's stream)
    // the entry holds no target until the new one is derived
    h.target_set = false;
    invalidate_graph(p);
    if (alloc_head_sliced(h, proj, total, rows, PlanAlloc{p})) return 1;
    ST_HIP(hipStreamSynchronize(nullptr));
    h.sl_rows = rows;
    h.sl_images = n_kept;
    unsigned int* bounds = reinterpret_cast<unsigned int*>(h.sl_bounds);
    ST_HIP(hipMemsetAsync(bounds + kAmaxWordUints, 0, (size_t)kSlicedMaxImages * kAmaxWordUints * sizeof(unsigned int), s));
    float* dst = h.sl_feats;
    for (int k = 0; k < n_kept; ++k) {
        const int i = kept[k];
        const size_t count = (size_t)h.n * (size_t)ms[i];
        ST_HIP(hipMemcpyAsync(dst, feats[i], count * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (launch_amax(dst, (long long)count, bounds + (size_t)(1 + k) * kAmaxWordUints, 0, s)) return 1;
        h.sl_m[k] = ms[i];
        h.sl_a[k] = (float)((double)(weights ? weights[i] : 1.f) / sum);
        dst += count;
    }
    // the directions of the epoch the next closure runs at - 0 for an entry that keeps its directions - and the target under them
    if (sliced_refresh(p, index, p->sliced_resample[index] ? p->sliced_epoch : 0ull, s)) return 1;
    h.target_set = true;
    return 0;
}

int st_plan_sliced_directions(st_plan* p, int index, const float** r, int* projections, int* channels, unsigned long long* epoch) {
    ST_REQUIRE(p && r && projections && channels && epoch, "st_plan_sliced_directions: null argument");
    ST_REQUIRE(index >= 0 && index < p->n_style, "st_plan_sliced_directions: index %d out of range (%d style layers)", index, p->n_style);
    const StyleHead& h = p->head[p->style_op[index]];
    ST_REQUIRE(p->style_sliced[index] && h.target_set && h.sl_r,
               "st_plan_sliced_directions: style layer %d holds no directions (st_plan_set_style_sliced, st_plan_set_style_sliced_vectors)", index);
    *r = h.sl_r;
    *projections = sliced_projections_of(p, index);
    *channels = h.n;
    *epoch = h.sl_epoch;
    return 0;
}

int st_plan_sliced_target(st_plan* p, int index, const float** target, int* projections, long long* n) {
    ST_REQUIRE(p && target && projections && n, "st_plan_sliced_target: null argument");
    ST_REQUIRE(index >= 0 && index < p->n_style, "st_plan_sliced_target: index %d out of range (%d style layers)", index, p->n_style);
    const StyleHead& h = p->head[p->style_op[index]];
    ST_REQUIRE(p->style_sliced[index] && h.target_set && h.sl_t,
               "st_plan_sliced_target: style layer %d holds no target (st_plan_set_style_sliced, st_plan_set_style_sliced_vectors)", index);
    *target = h.sl_t;
    *projections = sliced_projections_of(p, index);
    *n = h.npix_local;
    return 0;
}

int st_plan_set_loss_weights(st_plan* p, float content_weight, const float* style_layer_weights,
                             float tv_weight) {
    ST_REQUIRE(p && style_layer_weights, "st_plan_set_loss_weights: null argument");
    ST_REQUIRE(p->reference_taps, "st_plan_set_loss_weights: the plan's layers were configured (st_plan_set_taps): use st_plan_set_tap_weights");
    p->content_weight[0] = content_weight;
    for (int i = 0; i < 5; ++i) p->style_weight[i] = style_layer_weights[i];
    p->tv_weight = tv_weight;
    invalidate_graph(p);       // the weights are baked into kernel arguments
    p->phases.clear();         // (a strip's phase sequence is rebuilt by its next closure)
    return 0;
}

int st_plan_loss_and_grad(st_plan* p, const float* image, float* grad_out, float* losses_out, void* stream) {
    ST_REQUIRE(p && image && grad_out, "st_plan_loss_and_grad: null argument");
    if (ensure_grad_alloc(p) || ensure_streams(p, static_cast<hipStream_t>(stream))) return 1;
    return closure_entry(p, image, grad_out, losses_out, static_cast<hipStream_t>(stream));
}

int st_plan_step(st_plan* p, float* image, float* exp_avg, float* exp_avg_sq, float* ema_value,
                 long long step, double lr, double beta1, double beta2, double eps, double ema_decay,
                 float* losses_out, void* stream) {
    ST_REQUIRE(p && image && exp_avg && exp_avg_sq && ema_value, "st_plan_step: null argument");
    ST_REQUIRE(step >= 1, "st_plan_step: step must be >= 1");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (ensure_grad_alloc(p) || ensure_streams(p, s)) return 1;
    // Round 6: the sum of the loss terms and the clearing of the operand bounds for the next pass were two dependent launches
    // of ~5 us each on the caller's stream, every iteration; they ride in the update kernel (ST_STEP_TAIL=0: launches of their
    // own, as in the closure-only entry points; not under graph replay, whose captured closure ends with the sum)
    // ST_STEP_TAIL=2 (default) goes one further: the update itself is applied by conv1_1's fold kernel - the last kernel of the
    // backward pass, which has each gradient element in a register when it is final - so the iteration ends with ONE launch
    // instead of four (fold, sum, update, memset).  Not while profiling (bench.py's roofline_hbm times the update kernel).
    static Option tail_opt("ST_STEP_TAIL", 2);
    const bool fold_tail = tail_opt.get() != 0 && !p->graph_enabled;
    const bool fold_step = fold_tail && tail_opt.get() >= 2 && !p->profiling;
    AdamTail tail{};
    if (fold_tail) {
        tail.losses8 = p->losses;
        tail.losses_copy = losses_out;
        if (p->net->conv_elem == 1) { tail.zero = reinterpret_cast<unsigned int*>(p->amax_word); tail.zero_count = 64ll * kAmaxWordUints; }
    }
    const AdamScalars sc = adam_scalars(step, lr, beta1, beta2, eps, ema_decay);
    FoldUpdate upd{image, exp_avg, exp_avg_sq, ema_value, sc, tail};
    if (upd.tail.losses_copy == upd.tail.losses8) upd.tail.losses_copy = nullptr;
    p->defer_sum = fold_tail;
    p->fold_update = fold_step ? &upd : nullptr;
    p->fold_updated = false;
    const int closure_rc = closure_entry(p, image, p->grad_img, losses_out, s);
    p->defer_sum = false;
    p->fold_update = nullptr;
    if (closure_rc) return 1;
    if (p->fold_updated) {
        p->fold_updated = false;
        p->amax_clean = tail.zero != nullptr;
        return 0;
    }
    // reads image, gradient, both moments, EMA; writes image, both moments, EMA
    const int rc = hbm_profiled(p, HBM_ADAM, 9.0 * 3 * 4.0 * p->H * p->W, s, [&] {
        return launch_adam_clamp_ema(image, p->grad_img, exp_avg, exp_avg_sq, ema_value, 3ll * p->H * p->W, sc, s, tail);
    });
    p->amax_clean = rc == 0 && tail.zero != nullptr;
    return rc;
}

int st_plan_apply_update(st_plan* p, float* image, const float* grad, float* exp_avg, float* exp_avg_sq,
                         float* ema_value, long long step, double lr, double beta1, double beta2, double eps,
                         double ema_decay, void* stream) {
    ST_REQUIRE(p && image && grad && exp_avg && exp_avg_sq && ema_value, "st_plan_apply_update: null argument");
    ST_REQUIRE(step >= 1, "st_plan_apply_update: step must be >= 1");
    return launch_adam_clamp_ema(image, grad, exp_avg, exp_avg_sq, ema_value, 3ll * p->H * p->W,
                                 adam_scalars(step, lr, beta1, beta2, eps, ema_decay),
                                 static_cast<hipStream_t>(stream));
}

int st_plan_debug_read(st_plan* p, int what, float* out, int count) {
    ST_REQUIRE(p && out && count > 0, "st_plan_debug_read: bad argument");
    // what = 0: the partial sums of the TV kernels' workgroups, 4 floats each (tv_interior_kernel's first, then tv_border_kernel's)
    // what = 1: every thread's (s1, s2, s3, s4, groups visited) of tv_interior_kernel under ST_TV_VARIANT=3
    // what = 2: the 64 operand bounds of amax_word, each as the maximum over its kAmaxSlots slots (raw bits, as the consumers read it)
    // what = 16 + i: Node::g of kProgram[i], the gradient map as its consumer stages it (count = its element count)
    const bool grad_map = what >= 16 && what < 16 + kNumOps;
    ST_REQUIRE((what == 0 && count <= 4 * kStreamBlocks) || (what == 1 && count <= kStreamBlocks * 256 * 5 && tv_debug_buffer()) ||
                   (what == 2 && count == 64) ||
                   (grad_map && p->grads_allocated && (size_t)count == node_at(p, what - 16).count()),
               "st_plan_debug_read: unknown buffer or count out of range");
    ST_HIP(hipDeviceSynchronize());
    if (what == 2) {
        std::vector<unsigned int> words((size_t)64 * kAmaxWordUints);
        ST_HIP(hipMemcpy(words.data(), p->amax_word, words.size() * sizeof(unsigned int), hipMemcpyDeviceToHost));
        for (int w = 0; w < 64; ++w) {
            unsigned int m = 0;
            for (int slot = 0; slot < kAmaxSlots; ++slot) m = std::max(m, words[(size_t)w * kAmaxWordUints + (size_t)slot * kAmaxSlotStride]);
            memcpy(&out[w], &m, sizeof(float));
        }
        return 0;
    }
    if (grad_map) {
        ST_HIP(hipMemcpy(out, node_at(p, what - 16).g, (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
        return 0;
    }
    ST_HIP(hipMemcpy(out, what == 0 ? p->red_partials : tv_debug_buffer(), (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int st_plan_losses(st_plan* p, float** losses) {
    ST_REQUIRE(p && losses, "st_plan_losses: null argument");
    *losses = p->losses;
    return 0;
}

int st_plan_moment_sums(st_plan* p, int layer, float* sums, void* stream) {
    ST_REQUIRE(p && sums, "st_plan_moment_sums: null argument");
    int idx = -1;
    for (int k = 0; k < p->n_style; ++k)
        if (kProgram[p->style_op[k]].feat_index == layer) idx = k;
    ST_REQUIRE(idx >= 0, "st_plan_moment_sums: features[%d] is not a style layer", layer);
    if (ensure_style_alloc(p, p->head[p->style_op[idx]], p->style_kind[idx])) return 1;      // (strip plans: never diagonal)
    return moment_sums_of_tap(p, idx, sums, static_cast<hipStream_t>(stream));
}

int st_plan_set_graph(st_plan* p, int enable) {
    ST_REQUIRE(p, "st_plan_set_graph: null plan");
    p->graph_enabled = enable != 0;
    if (!enable) invalidate_graph(p);
    return 0;
}

int st_plan_profile_enable(st_plan* p, int enable) {
    ST_REQUIRE(p, "st_plan_profile_enable: null plan");
    p->profiling = enable != 0;
    return 0;
}

int st_plan_profile_read(st_plan* p, long long* launches, double* millis, double* flops) {
    ST_REQUIRE(p, "st_plan_profile_read: null plan");
    for (size_t i = 0; i < p->events_used; ++i) {
        ProfileEvent& e = p->events[i];
        ST_HIP(hipEventSynchronize(e.stop));
        float ms = 0.f;
        ST_HIP(hipEventElapsedTime(&ms, e.start, e.stop));
        p->prof_ms += ms;
        p->prof_flops += e.flops;
        p->prof_launches += 1;
    }
    p->events_used = 0;
    p->hbm_used = 0;
    if (launches) *launches = p->prof_launches;
    if (millis) *millis = p->prof_ms;
    if (flops) *flops = p->prof_flops;
    p->prof_launches = 0;
    p->prof_ms = 0;
    p->prof_flops = 0;
    return 0;
}

int st_plan_profile_read_hbm(st_plan* p, int category, long long* launches, double* millis, double* bytes) {
    ST_REQUIRE(p && category >= 0 && category < HBM_CATS, "st_plan_profile_read_hbm: bad argument");
    // call for every category of interest BEFORE st_plan_profile_read / the next profiled step: events are kept until
    // category -1 ... (they are recycled by st_plan_profile_read)
    long long n = 0;
    double ms_sum = 0, b = 0;
    for (size_t i = 0; i < p->hbm_used; ++i) {
        HbmEvent& e = p->hbm_events[i];
        if (e.cat != category) continue;
        ST_HIP(hipEventSynchronize(e.stop));
        float ms = 0.f;
        ST_HIP(hipEventElapsedTime(&ms, e.start, e.stop));
        ms_sum += ms;
        b += e.bytes;
        ++n;
    }
    if (launches) *launches = n;
    if (millis) *millis = ms_sum;
    if (bytes) *bytes = b;
    return 0;
}


}  // extern "C"
