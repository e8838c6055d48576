// Standalone operators of the C ABI for the kernel-level tests and tools/: one kernel family per call, on buffers the caller owns.
#include <cstdlib>
#include <vector>

#include "../../include/st_amd.h"
#include "st_common.h"

namespace st {
namespace {

// the temporary device buffers and events of one operator call: released when the call returns, on every path (the
// stream is synchronised first - kernels of the call may still read them)
struct OpScratch {
    hipStream_t stream;
    std::vector<void*> buffers;
    std::vector<hipEvent_t> events;
    explicit OpScratch(hipStream_t s) : stream(s) {}
    OpScratch(const OpScratch&) = delete;
    OpScratch& operator=(const OpScratch&) = delete;
    ~OpScratch() {
        hipStreamSynchronize(stream);
        for (void* b : buffers) hipFree(b);
        for (hipEvent_t e : events) hipEventDestroy(e);
    }
    template <class T>
    int alloc(T** out, size_t bytes) {
        void* p = nullptr;
        ST_HIP(hipMalloc(&p, bytes));
        buffers.push_back(p);
        *out = static_cast<T*>(p);
        return 0;
    }
    int event(hipEvent_t* out) {
        ST_HIP(hipEventCreate(out));
        events.push_back(*out);
        return 0;
    }
};

// precision code 5 (the Winograd form) is served by an --experiments library only: refused before anything is allocated
int reject_winograd(int precision) {
    ST_REQUIRE(precision != 5 || kExperiments,
               "the Winograd convolution (precision code 5) needs a library built with build.py --experiments");
    return 0;
}

}  // namespace
}  // namespace st

using namespace st;

extern "C" {

// ---- standalone operators for kernel-level tests -------------------------------------------------
int st_op_sqrtm_ns(const float* a, float* root, int n, void* stream) {
    ST_REQUIRE(a && root, "st_op_sqrtm_ns: null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    OpScratch tmp(s);
    float* base = nullptr;
    if (tmp.alloc(&base, ns_workspace_floats(n) * sizeof(float))) return 1;
    NSWorkspace ws{};
    ns_workspace_carve(ws, base, n);
    int rc = ns_workspace_reset(ws, s) || ns_sqrt_forward(a, root, n, ws, s);
    hipStreamSynchronize(s);
    if (!rc) rc = ns_chain_check(ws, "st_op_sqrtm_ns");
    return rc;
}

int st_op_sqrtm_ns_backward(const float* root, const float* grad_root, float* grad_a, int n, void* stream) {
    ST_REQUIRE(root && grad_root && grad_a, "st_op_sqrtm_ns_backward: null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    OpScratch tmp(s);
    float* base = nullptr;
    if (tmp.alloc(&base, ns_workspace_floats(n) * sizeof(float))) return 1;
    NSWorkspace ws{};
    ns_workspace_carve(ws, base, n);
    return ns_workspace_reset(ws, s) || ns_sqrt_backward(root, grad_root, nullptr, grad_a, n, ws, s);
}

int st_op_sqrtm_ns_backward_diag(const float* root, float grad_diag, float* grad_a, int n, void* stream) {
    ST_REQUIRE(root && grad_a, "st_op_sqrtm_ns_backward_diag: null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    OpScratch tmp(s);
    float *base = nullptr, *gd = nullptr;
    if (tmp.alloc(&base, ns_workspace_floats(n) * sizeof(float)) || tmp.alloc(&gd, 256)) return 1;
    ST_HIP(hipMemcpyAsync(gd, &grad_diag, sizeof(float), hipMemcpyHostToDevice, s));
    NSWorkspace ws{};
    ns_workspace_carve(ws, base, n);
    int rc = ns_workspace_reset(ws, s) || ns_sqrt_backward(root, nullptr, gd, grad_a, n, ws, s);
    hipStreamSynchronize(s);
    if (!rc) rc = ns_chain_check(ws, "st_op_sqrtm_ns_backward_diag");
    return rc;
}

int st_op_sqrtm_time(int n, int iters, double* fwd_us, double* bwd_us, void* stream) {
    ST_REQUIRE(fwd_us && bwd_us && iters > 0, "st_op_sqrtm_time: bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t nn = (size_t)n * n;
    OpScratch tmp(s);
    float *base = nullptr, *a = nullptr, *root = nullptr, *g = nullptr, *ga = nullptr, *gd = nullptr;
    if (tmp.alloc(&base, ns_workspace_floats(n) * 4) || tmp.alloc(&a, nn * 4) || tmp.alloc(&root, nn * 4) ||
        tmp.alloc(&g, nn * 4) || tmp.alloc(&ga, nn * 4) || tmp.alloc(&gd, 256))
        return 1;
    std::vector<float> h(nn, 0.f);
    unsigned x = 777u;
    for (size_t i = 0; i < nn; ++i) { x = x * 1664525u + 1013904223u; h[i] = ((int)(x >> 9) % 2001 - 1000) * 1e-4f; }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j) h[(size_t)i * n + j] = h[(size_t)j * n + i];     // symmetric
    for (int i = 0; i < n; ++i) h[(size_t)i * n + i] = 1.0f + 0.1f * (i % 7);          // diagonally dominant
    ST_HIP(hipMemcpy(a, h.data(), nn * 4, hipMemcpyHostToDevice));
    ST_HIP(hipMemcpy(g, h.data(), nn * 4, hipMemcpyHostToDevice));
    NSWorkspace ws{};
    ns_workspace_carve(ws, base, n);
    if (ns_workspace_reset(ws, s)) return 1;
    hipEvent_t e0, e1, e2;
    if (tmp.event(&e0) || tmp.event(&e1) || tmp.event(&e2)) return 1;
    // ST_NS_TIME_DIAG=1: time the backward the plan runs (gradient = multiple of I) instead of the general one
    static Option diag_opt("ST_NS_TIME_DIAG", 0);
    const bool diag = diag_opt.get() != 0;
    const float gdv = -2.f / n;
    ST_HIP(hipMemcpy(gd, &gdv, sizeof(float), hipMemcpyHostToDevice));
    const float* gfull = diag ? nullptr : g;
    const float* gdiag = diag ? gd : nullptr;
    if (ns_sqrt_forward(a, root, n, ws, s) || ns_sqrt_backward(root, gfull, gdiag, ga, n, ws, s)) return 1;
    ST_HIP(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i)
        if (ns_sqrt_forward(a, root, n, ws, s)) return 1;
    ST_HIP(hipEventRecord(e1, s));
    for (int i = 0; i < iters; ++i)
        if (ns_sqrt_backward(root, gfull, gdiag, ga, n, ws, s)) return 1;
    ST_HIP(hipEventRecord(e2, s));
    ST_HIP(hipEventSynchronize(e2));
    float f = 0.f, b = 0.f;
    ST_HIP(hipEventElapsedTime(&f, e0, e1));
    ST_HIP(hipEventElapsedTime(&b, e1, e2));
    *fwd_us = f * 1e3 / iters;
    *bwd_us = b * 1e3 / iters;
    return ns_chain_check(ws, "st_op_sqrtm_time");
}

int st_op_tv_loss(const float* image, int height, int width, float* loss_out, float* grad_out, void* stream) {
    ST_REQUIRE(image && loss_out && grad_out, "st_op_tv_loss: null argument");
    ST_REQUIRE(height >= 1 && width >= 1, "st_op_tv_loss: bad shape %d x %d", height, width);
    ST_REQUIRE_PIXELS("st_op_tv_loss", (long long)height * width);
    hipStream_t s = static_cast<hipStream_t>(stream);
    OpScratch tmp(s);
    float* partials = nullptr;
    if (tmp.alloc(&partials, 4 * kStreamBlocks * sizeof(float))) return 1;
    return launch_tv(image, height, width, 1.0f, grad_out, partials, loss_out, s);
}

static int conv_op(const float* in, const float* mask, const float* weight, const float* bias, float* out,
                   int cin, int cout, int height, int width, int relu, int dgrad, int precision, hipStream_t s,
                   const float* halo = nullptr, int has_up = 0, int has_down = 0, int accumulate = 0,
                   const float* out_mask = nullptr, int overlap = 0) {
    // precision 5: fp16x3 in the Winograd F(2x2, 3x3) form wherever that kernel takes the problem (st_conv_wino.hip), else the
    // direct fp16x3 kernels
    if (reject_winograd(precision)) return 1;
    const bool wino5 = precision == 5;
    if (wino5) precision = 4;
    ST_REQUIRE(conv_precision_valid(precision), "conv precision must be 0, 2, 3 or 4");
    ST_REQUIRE(height >= 1 && width >= 1, "st_op_conv3x3: bad shape %d x %d", height, width);
    ST_REQUIRE_PIXELS("st_op_conv3x3", (long long)height * width);        // (all four st_op_conv3x3* entries)
    OpScratch tmp(s);
    float* wl = nullptr;
    float* scratch = nullptr;
    unsigned int* amax = nullptr;
    if (tmp.alloc(&wl, (size_t)cin * cout * 9 * sizeof(float)) || tmp.alloc(&scratch, kConvScratchFloats * sizeof(float)) ||
        tmp.alloc(&amax, kAmaxWordUints * 4))
        return 1;
    ST_HIP(hipMemsetAsync(amax, 0, kAmaxWordUints * 4, s));
    ConvProblem c{};
    c.scratch = scratch;
    if (precision > 0) {
        c.planes = conv_precision_planes(precision);
        c.elem = conv_precision_elem(precision);
        c.amax_word = amax;
        c.amax_measure = 1;
        void* wsplit = nullptr;
        if (tmp.alloc(&wsplit, split_weight_bytes(cin, cout, c.planes)) ||
            launch_relayout_split(weight, wsplit, cin, cout, dgrad, c.planes, c.elem, s))
            return 1;
        c.wgt_split = wsplit;
    }
    if (wino5) {
        void* wino = nullptr;
        if (tmp.alloc(&wino, winograd_weight_bytes(cin, cout)) || launch_winograd_weights(weight, wino, cin, cout, dgrad, s))
            return 1;
        c.wgt_wino = wino;
        c.wino = 2;
    }
    if (!dgrad) {
        if (launch_relayout_fwd(weight, wl, cin, cout, s)) return 1;
        c.cin = cin; c.cout = cout;
    } else {
        if (launch_relayout_dgrad(weight, wl, cin, cout, s)) return 1;
        c.cin = cout; c.cout = cin;
    }
    c.in = in; c.mask = mask; c.wgt = wl; c.bias = bias; c.out = out; c.height = height; c.width = width;
    c.taps = 9; c.relu = relu; c.accumulate = accumulate; c.out_mask = out_mask;
    c.in_halo = halo; c.has_up = halo ? has_up : 0; c.has_down = halo ? has_down : 0;
    if (overlap) {          // interior rows first (no halo), then the boundary rows: the strip plans' two-launch form
        PcOverlap o{};
        ST_REQUIRE(conv_pc_overlap_choice(c, &o), "st_op_conv3x3_strip_ex: this problem cannot be cut into interior + boundary launches");
        ConvProblem part = c;
        part.overlap_part = 1; part.in_halo = nullptr; part.has_up = 0; part.has_down = 0;
        if (launch_conv(part, s)) return 1;
        part = c;
        part.overlap_part = 2; part.amax_measure = 0;
        return launch_conv(part, s);
    }
    return launch_conv(c, s);
}

int st_op_conv1x1(const float* in, const float* weight, const float* bias, float* out, int cin, int cout,
                  long long npix, int precision, void* stream) {
    ST_REQUIRE(in && weight && out, "st_op_conv1x1: null argument");
    ST_REQUIRE(precision == 0 || precision == 4, "st_op_conv1x1: precision must be 0 (fp32) or 4 (fp16x3)");
    ST_REQUIRE(cin > 0 && cout > 0 && cin % 32 == 0 && cout % 64 == 0, "st_op_conv1x1: bad shape");
    ST_REQUIRE_PIXELS("st_op_conv1x1", npix);
    hipStream_t s = static_cast<hipStream_t>(stream);
    OpScratch tmp(s);
    unsigned int* amax = nullptr;
    float* scratch = nullptr;
    if (tmp.alloc(&amax, 2 * kAmaxWordUints * 4) || tmp.alloc(&scratch, kConvScratchFloats * sizeof(float))) return 1;
    ST_HIP(hipMemsetAsync(amax, 0, 2 * kAmaxWordUints * 4, s));
    ConvProblem c{};
    c.in = in; c.wgt = weight; c.bias = bias; c.out = out; c.cin = cin; c.cout = cout;
    c.height = 1; c.width = (int)npix; c.taps = 1; c.scratch = scratch;
    if (precision == 4) {
        c.planes = 2; c.elem = 1; c.amax_word = amax; c.wgt_amax = amax + kAmaxWordUints;
        if (launch_amax(in, (long long)cin * npix, amax, 0, s) || launch_amax(weight, (long long)cin * cout, amax + kAmaxWordUints, 0, s))
            return 1;
    }
    return launch_conv(c, s);
}

int st_op_pool2x2(const float* in, float* out, int channels, int height, int width, int mode, void* stream) {
    ST_REQUIRE(in && out, "st_op_pool2x2: null argument");
    ST_REQUIRE(mode >= 0 && mode <= 2, "st_op_pool2x2: mode must be 0 (max), 1 (average) or 2 (l2)");
    ST_REQUIRE(channels > 0 && height >= 2 && width >= 2, "st_op_pool2x2: C >= 1 and H, W >= 2 required");
    ST_REQUIRE_PIXELS("st_op_pool2x2", (long long)height * width);
    return launch_pool_fwd(in, out, channels, height, width, mode, static_cast<hipStream_t>(stream));
}

int st_op_pool2x2_backward(const float* in, const float* grad_out, float* grad_in, int channels, int height, int width,
                           int mode, void* stream) {
    ST_REQUIRE(in && grad_out && grad_in, "st_op_pool2x2_backward: null argument");
    ST_REQUIRE(mode >= 0 && mode <= 2, "st_op_pool2x2_backward: mode must be 0 (max), 1 (average) or 2 (l2)");
    ST_REQUIRE(channels > 0 && height >= 2 && width >= 2, "st_op_pool2x2_backward: C >= 1 and H, W >= 2 required");
    ST_REQUIRE_PIXELS("st_op_pool2x2_backward", (long long)height * width);
    return launch_pool_bwd(in, grad_out, grad_in, channels, height, width, mode, static_cast<hipStream_t>(stream));
}

int st_op_conv3x3_time(int cin, int cout, int height, int width, int dgrad, int precision, int iters,
                       double* avg_us, void* stream) {
    ST_REQUIRE(avg_us && iters > 0, "st_op_conv3x3_time: bad argument");
    ST_REQUIRE(conv_precision_valid(precision) || precision == 5, "conv precision must be 0, 2, 3, 4 or 5 (fp16x3, Winograd form)");
    if (reject_winograd(precision)) return 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t hw = (size_t)height * width;
    OpScratch tmp(s);
    float *in = nullptr, *mask = nullptr, *w = nullptr, *wl = nullptr, *bias = nullptr, *out = nullptr,
          *scratch = nullptr;
    unsigned int* amax = nullptr;
    const int kin = dgrad ? cout : cin, kout = dgrad ? cin : cout;
    if (tmp.alloc(&in, kin * hw * 4) || tmp.alloc(&mask, kin * hw * 4) || tmp.alloc(&out, kout * hw * 4) ||
        tmp.alloc(&w, (size_t)cin * cout * 9 * 4) || tmp.alloc(&wl, (size_t)cin * cout * 9 * 4) || tmp.alloc(&bias, kout * 4) ||
        tmp.alloc(&scratch, kConvScratchFloats * 4) || tmp.alloc(&amax, 2 * kAmaxWordUints * 4))
        return 1;
    // deterministic non-trivial contents (values matter for DVFS: do not time zero-filled operands)
    std::vector<float> host(std::max<size_t>((size_t)cin * cout * 9, kin * hw));
    unsigned x = 12345u;
    for (float& v : host) { x = x * 1664525u + 1013904223u; v = ((int)(x >> 9) % 2001 - 1000) * 1e-3f; }
    ST_HIP(hipMemcpy(in, host.data(), kin * hw * 4, hipMemcpyHostToDevice));
    ST_HIP(hipMemcpy(mask, host.data(), kin * hw * 4, hipMemcpyHostToDevice));
    ST_HIP(hipMemcpy(w, host.data(), (size_t)cin * cout * 9 * 4, hipMemcpyHostToDevice));
    ST_HIP(hipMemcpy(bias, host.data(), kout * 4, hipMemcpyHostToDevice));
    ConvProblem c{};
    if (dgrad) { if (launch_relayout_dgrad(w, wl, cin, cout, s)) return 1; }
    else { if (launch_relayout_fwd(w, wl, cin, cout, s)) return 1; }
    // (ST_CONV_NOMASK=1: time the data gradient as the plan runs it - masked by its producer, no mask stream)
    static Option nomask_opt("ST_CONV_NOMASK", 0);
    c.in = in; c.mask = (dgrad && !nomask_opt.get()) ? mask : nullptr; c.wgt = wl; c.bias = dgrad ? nullptr : bias; c.out = out;
    c.cin = kin; c.cout = kout; c.height = height; c.width = width; c.taps = 9; c.relu = dgrad ? 0 : 1;
    c.scratch = scratch;
    if (precision == 5) {          // fp16x3, Winograd form wherever it takes the problem
        precision = 4;
        void* wino = nullptr;
        if (tmp.alloc(&wino, winograd_weight_bytes(cin, cout)) || launch_winograd_weights(w, wino, cin, cout, dgrad, s))
            return 1;
        c.wgt_wino = wino;
        c.wino = 2;
        c.mask = nullptr;          // (as the plan runs its data gradients: masked by their producers)
    }
    if (precision > 0) {
        c.planes = conv_precision_planes(precision);
        c.elem = conv_precision_elem(precision);
        c.amax_word = amax;
        void* wsplit = nullptr;
        if (tmp.alloc(&wsplit, split_weight_bytes(cin, cout, c.planes)) ||
            launch_relayout_split(w, wsplit, cin, cout, dgrad, c.planes, c.elem, s))
            return 1;
        c.wgt_split = wsplit;
    }
    // fp16x3: the operand bound is measured once here; inside a plan it comes for free from the producer's
    // epilogue, so the timed launches (like the plan's) only read the word and fold max |out| into another
    ST_HIP(hipMemsetAsync(amax, 0, 2 * kAmaxWordUints * 4, s));
    c.amax_measure = 1;
    c.out_amax = c.elem == 1 ? amax + kAmaxWordUints : nullptr;
    if (launch_conv(c, s)) return 1;
    c.amax_measure = 0;
    auto launch = [&]() -> int { return launch_conv(c, s); };
    for (int i = 0; i < 3; ++i)
        if (launch()) return 1;
    hipEvent_t e0, e1;
    if (tmp.event(&e0) || tmp.event(&e1)) return 1;
    ST_HIP(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i)
        if (launch()) return 1;
    ST_HIP(hipEventRecord(e1, s));
    ST_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    ST_HIP(hipEventElapsedTime(&ms, e0, e1));
    *avg_us = ms * 1e3 / iters;
    if (option_env("ST_CONV_PHASES")) {          // s_memtime phase stamps of the producer / consumer kernel (tune bit 32)
        const char* tune_env = option_env("ST_CONV_TUNE");          // ablation bits of the timed launches stay on
        const int keep = tune_env ? atoi(tune_env) : 0;
        c.tune = keep | 32;
        ST_HIP(hipMemsetAsync(scratch, 0, 1 << 20, s));
        for (int i = 0; i < 4; ++i)                     // a few launches back to back: the clock has settled
            if (launch_conv(c, s)) return 1;
        ST_HIP(hipStreamSynchronize(s));
        c.tune = 0;
        {
            std::vector<unsigned long long> st(8 * 4096);
            ST_HIP(hipMemcpy(st.data(), scratch, st.size() * 8, hipMemcpyDeviceToHost));
            double ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            int n = 0;
            for (int b = 0; b < 4096; ++b) {
                if (st[8 * b + 6] != 1) continue;
                for (int k = 0; k < 8; ++k) ph[k] += (double)st[8 * b + k];
                ++n;
            }
            if (n)
                fprintf(stderr, "[phases] %d->%d @%d dgrad %d tune %d: %d WGs, ticks avg per WG: consumer MFMA %.0f | consumer barrier "
                        "wait %.0f | epilogue %.0f | producer staging %.0f | producer barrier wait %.0f | whole %.0f; shader "
                        "clock %.0f MHz; %.1f us\n",
                        cin, cout, height, dgrad, keep, n, ph[0] / n, ph[1] / n, ph[2] / n, ph[3] / n, ph[4] / n, ph[5] / n,
                        ph[7] > 0 ? ph[5] / ph[7] * 100.0 : 0.0, *avg_us);
        }
    }
    return 0;
}

int st_op_conv3x3(const float* in, const float* weight, const float* bias, float* out, int cin, int cout,
                  int height, int width, int relu, int precision, void* stream) {
    ST_REQUIRE(in && weight && out, "st_op_conv3x3: null argument");
    return conv_op(in, nullptr, weight, bias, out, cin, cout, height, width, relu, 0, precision,
                   static_cast<hipStream_t>(stream));
}

int st_op_conv3x3_dgrad(const float* grad_out, const float* relu_out, const float* weight, float* grad_in,
                        int cin, int cout, int height, int width, int precision, void* stream) {
    ST_REQUIRE(grad_out && weight && grad_in, "st_op_conv3x3_dgrad: null argument");
    return conv_op(grad_out, relu_out, weight, nullptr, grad_in, cin, cout, height, width, 0, 1, precision,
                   static_cast<hipStream_t>(stream));
}

int st_op_conv3x3_strip(const float* in, const float* halo, int has_up, int has_down, const float* weight,
                        const float* bias, float* out, int cin, int cout, int height, int width, int relu, int dgrad,
                        int precision, void* stream) {
    ST_REQUIRE(in && halo && weight && out, "st_op_conv3x3_strip: null argument");
    return conv_op(in, nullptr, weight, dgrad ? nullptr : bias, out, cin, cout, height, width, dgrad ? 0 : relu, dgrad,
                   precision, static_cast<hipStream_t>(stream), halo, has_up != 0, has_down != 0);
}

int st_op_conv3x3_strip_ex(const float* in, const float* halo, int has_up, int has_down, const float* weight,
                           const float* bias, float* out, const float* out_mask, int cin, int cout, int height, int width,
                           int relu, int dgrad, int accumulate, int overlap, int precision, void* stream) {
    ST_REQUIRE(in && weight && out, "st_op_conv3x3_strip_ex: null argument");       // (halo == NULL: a whole image)
    return conv_op(in, nullptr, weight, dgrad ? nullptr : bias, out, cin, cout, height, width, dgrad ? 0 : relu, dgrad,
                   precision, static_cast<hipStream_t>(stream), halo, has_up != 0, has_down != 0, accumulate != 0, out_mask,
                   overlap);
}

}  // extern "C"
