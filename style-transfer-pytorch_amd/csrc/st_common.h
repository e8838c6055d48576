// Shared declarations for the gfx950 kernels of libst_amd.so.  CDNA4 only: 64-lane wavefronts,
// v_mfma_f32_32x32x2_f32 (exact fp32 FMA chain, 64 cycles/SIMD) as the contraction primitive.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <string>

namespace st {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kWave = 64;

// ---- error plumbing (no exceptions across the C ABI) -------------------------------------------
void set_error(const char* fmt, ...);
const char* get_error();

#define ST_HIP(expr)                                                                           \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            st::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,     \
                          __LINE__);                                                           \
            return 1;                                                                          \
        }                                                                                      \
    } while (0)

#define ST_LAUNCH_CHECK()                                                                      \
    do {                                                                                       \
        hipError_t _e = hipGetLastError();                                                     \
        if (_e != hipSuccess) {                                                                \
            st::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, \
                          __LINE__);                                                           \
            return 1;                                                                          \
        }                                                                                      \
    } while (0)

#define ST_REQUIRE(cond, ...)          \
    do {                               \
        if (!(cond)) {                 \
            st::set_error(__VA_ARGS__); \
            return 1;                  \
        }                              \
    } while (0)

// ---- the size limit ---------------------------------------------------------------------------------
// One image, strip, tap or feature map handed to any entry point has at most kMaxPixels = 2^24 - 1 pixels (H * W, or npix).
// The number comes from the fp16x3 3x3 kernels: they stage 16 input channels through one raw buffer resource of
// 16 * HW * 4 bytes and give a zero-padded tap the byte offset 2^30 (kOOR), which the hardware answers with 0 only while it
// lies beyond the resource, i.e. while 64 * HW <= 2^30; and every 3x3 and 1x1 convolution kernel writes through 32-channel
// output resources of 128 * HW bytes and parks the stores of out-of-tile lanes at the byte offset 0x7FFFFFFF, which is out of
// range only while 128 * HW <= 2^31 - 1, i.e. HW <= 2^24 - 1.  Every other 32-bit quantity in the library (`int` element
// counts of up to 64 * HW, 3 * HW) has room to spare at that size; profiles/size_limits.md lists them entry by entry.  st_max_pixels() reports the number; every entry refuses a larger map before it allocates.
constexpr long long kMaxPixels = (1ll << 24) - 1;
inline bool pixels_in_range(long long pixels) { return pixels >= 1 && pixels <= kMaxPixels; }
#define ST_REQUIRE_PIXELS(who, pixels)                                                                                  \
    ST_REQUIRE(st::pixels_in_range(pixels), "%s: %lld pixels: a map may hold 1 to %lld (2^24 - 1) pixels", who,        \
               (long long)(pixels), st::kMaxPixels)

// ---- build flavours -----------------------------------------------------------------------------
// The default libst_amd.so holds the hot path and nothing else.  `build.py --experiments` (-DST_EXPERIMENTS) adds the code
// that no default path executes - the persistent Newton-Schulz chain kernel (st_nschain.hip), the Winograd convolution
// (st_conv_wino.hip), the TV hazard's reproducer kernels, measurement-only kernels - and lets EVERY ST_* switch be set from the
// environment; in the default build the environment reaches only the documented switches (kEnvSwitches, tools/README.md), the
// others only answer to st_set_option (parity tests compare kernel variants inside one process).
#if defined(ST_EXPERIMENTS)
constexpr bool kExperiments = true;
#else
constexpr bool kExperiments = false;
#endif

// ---- runtime switches ---------------------------------------------------------------------------
// A/B and diagnostic switches: an ST_* environment variable, overridable at run time through the C ABI's
// st_set_option (parity tests compare kernel variants inside one process).  A call site holds a static Option;
// get() re-reads only when an override changed (generation counter), so the launch path pays one relaxed load.
int option_lookup(const char* name, int dflt);      // override > environment (where the build lets it through) > dflt
const char* option_env(const char* name);           // getenv under the same rule
unsigned option_generation();
struct Option {
    const char* name;
    int dflt;
    // (value, generation) packed into ONE atomic word: two host threads launching at once may both refresh the cache,
    // but neither can pair a new generation with a stale value
    std::atomic<unsigned long long> cached{0};
    Option(const char* n, int d) : name(n), dflt(d) {}
    int get() {
        const unsigned g = option_generation();
        const unsigned long long c = cached.load(std::memory_order_acquire);
        if ((unsigned)(c >> 32) == g) return (int)(unsigned)(c & 0xffffffffull);
        const int v = option_lookup(name, dflt);
        cached.store(((unsigned long long)g << 32) | (unsigned)v, std::memory_order_release);
        return v;
    }
};

// ---- device helpers ----------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Block-wide sum for 256-thread blocks; result valid in thread 0.  `scratch` = 4 floats of LDS.
__device__ __forceinline__ float block_sum_256(float v, float* scratch) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    float r = 0.f;
    if (threadIdx.x == 0) r = (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
    __syncthreads();
    return r;
}

// In-kernel final reduction ("last block") of the streaming value kernels (st_pointwise.hip, st_laplacian.hip): every block writes
// its partial sums, then takes a ticket; the block that draws the last one sums all partials in index order.
// The hand-off: thread 0 stores the block's N partial sums WRITE-THROUGH (agent-scope relaxed atomic stores: sc1), waits for
// them (the asm waitcnt; the compiler's own may be dropped) and only then takes the ticket - no release fence, which on gfx950
// writes back ALL of the XCD L2's dirty lines (the gradient the block has just streamed out) once per workgroup to publish
// four to sixteen bytes (profiles/last_block.md).  The helper does the stores itself, so no caller can leave a plain store in
// front of the fence-free ticket; storing, waiting and taking the ticket are one wave's (thread 0's) business.  The consumer
// side is an agent-scope acquire in every thread of the last block, then plain loads.
// release_fence (ST_LAST_BLOCK_FENCE=1, A/B and tests): the former hand-off - plain stores, an agent-scope release fence.
struct LastBlock {
    unsigned int* ticket;     // device word, zero between launches (the last block resets it); nullptr = two-launch form
    int release_fence;
};
LastBlock last_block(unsigned int* ticket);       // st_pointwise.hip: the flavour the switch selects
// every thread of the block calls it; `mine` = where the block's N partials go, v = their values (thread 0's are stored)
template <int N>
__device__ __forceinline__ bool last_block_arrives(const LastBlock& lb, bool* shared_flag, float* mine, const float (&v)[N]) {
    if (lb.ticket == nullptr) {       // the next launch on the stream reads them
        if (threadIdx.x == 0)
#pragma unroll
            for (int k = 0; k < N; ++k) mine[k] = v[k];
        return false;
    }
    if (threadIdx.x == 0) {
        if (lb.release_fence) {
#pragma unroll
            for (int k = 0; k < N; ++k) mine[k] = v[k];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        } else {
#pragma unroll
            for (int k = 0; k < N; ++k) __hip_atomic_store(mine + k, v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int prev = atomicAdd(lb.ticket, 1u);
        const bool last = (prev == gridDim.x - 1);
        if (last) *lb.ticket = 0u;
        *shared_flag = last;
    }
    __syncthreads();
    const bool last = *shared_flag;
    // every thread of the last block reads other blocks' partials: each needs its own agent-scope acquire (a CU's
    // vector L1 is never refreshed by another CU's stores; one lane's fence is not a guarantee for the other waves)
    if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    return last;
}

// StyleLossW2.forward's scalars for one head (style_transfer.py:178-181): the loss term and the seed of its backward,
// d loss / d root = gdiag * I.  A job rides along in the kernel that opens the Lyapunov backward chain (ns_prepare_kernel /
// ns_backward_entry_kernel) instead of being a launch of its own on the heads' critical path; loss_out == nullptr: no job.
struct W2LossJob {
    const float *mean, *mean_t, *cov, *cov_t, *root;
    int n;
    float weight;
    float* loss_out;
    float* gdiag_out;
};
__device__ __forceinline__ float w2_gdiag(const W2LossJob& j) { return -2.f * (j.weight / (float)j.n); }
// one 256-thread block; `scratch` = 4 floats of LDS
__device__ __forceinline__ void w2_loss_block(const W2LossJob& j, float* scratch) {
#pragma clang fp contract(off)
    float sm = 0.f, sc = 0.f;
    for (int i = threadIdx.x; i < j.n; i += 256) {
        const float d = j.mean[i] - j.mean_t[i];
        sm += d * d;
        const size_t ii = (size_t)i * j.n + i;
        sc += (j.cov_t[ii] + j.cov[ii]) - 2.f * j.root[ii];
    }
    sm = block_sum_256(sm, scratch);
    sc = block_sum_256(sc, scratch);
    if (threadIdx.x == 0) {
        const float fn = (float)j.n;
        j.loss_out[0] = (sm / fn + sc / fn) * j.weight;
        j.gdiag_out[0] = w2_gdiag(j);
    }
}

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// ---- convolution (st_conv.hip) -----------------------------------------------------------------
// Implicit-GEMM 3x3 (or 1x1) convolution on the fp32 MFMA.  D[co][pixel] = sum_k W[k][co] * X[k][pixel],
// k = (tap, ci).  `wgt` is pre-arranged as [taps][Cin][Cout] (Cout fastest).
struct ConvProblem {
    const float* in;       // [Cin][H][W]
    const float* mask;     // optional [Cin][H][W]: staged operand = (mask > 0) ? in : 0   (ReLU backward, consumer
                           // side: costs a second operand stream + 24 registers; the plan masks on the PRODUCER
                           // side instead, see out_mask, and uses this only where the producer cannot)
    const float* wgt;      // [taps][Cin][Cout]
    const float* bias;     // optional [Cout]
    float* out;            // [Cout][H][W]
    int cin, cout, height, width;
    int taps;              // 9 or 1
    int relu;              // epilogue max(x, 0)
    int accumulate;        // epilogue out += result (after bias), else out = result
    float* scratch;        // optional split-K workspace (kConvScratchFloats floats); nullptr = never split
    // Strip sharding (3x3 only): rows -1 and `height` of the operand live in a halo block
    // [2][Cin][W] (top rows, then bottom rows) filled by the neighbour exchange; a missing neighbour
    // (has_up / has_down == 0) means the global image border, i.e. zero padding.  With `mask`, halo rows
    // arrive already masked by the sender.
    const float* in_halo;
    int has_up, has_down;
    int tune;              // experiment bits (see st_conv.hip); 0 = shipped default
    // split-precision path (st_conv_split.hip): 16-bit planes of the weights, [planes][9][Cin/16][Cout][16]
    // followed by a 256-byte trailer (word 0: bits of max |w|, used by the fp16 mode's power-of-two scale).
    //   planes = 0           -> exact fp32 MFMA kernel
    //   planes = 2, elem = 0 -> bf16x3      planes = 3, elem = 0 -> bf16x6
    //   planes = 2, elem = 1 -> fp16x3: fp16 planes of operands pre-scaled by a power of two taken from an
    //                           upper bound of max |in|, read from the device bound `amax_word` (raw float
    //                           bits in kAmaxSlots slots, see amax_commit / amax_read).  The bound normally comes for free from the PRODUCER of `in` (every
    //                           kernel that finalises a conv operand folds max |out| into `out_amax`, see
    //                           amax_commit); amax_measure = 1 makes the launcher measure `in` itself first
    //                           (standalone operators).  A bound that is 2^k too large costs nothing but k
    //                           bits of fp16's underflow floor (2^-29 below the maximum), so pooled tensors
    //                           reuse their input's word.  Halo rows (strip sharding) are folded in by the
    //                           launcher.
    const void* wgt_split;
    int planes;
    int elem;
    unsigned int* amax_word;
    int amax_measure;
    int halo_amax_folded;  // strip plans: the caller has dealt with max |halo rows| - either folded it into amax_word
                           // or handed over the bounds the SENDERS measured (below)
    // strip plans, round 5: max |row| of the neighbours' halo rows as raw bits, measured by the sender while it packed the
    // rows and shipped in the same message (st_strip.hip halo_exchange: a 16-float trailer in front of the top rows / behind
    // the bottom rows).  The kernels take max(amax_word, these) - no launch between the halo's arrival and its consumer.
    const unsigned int* halo_bound_up;
    const unsigned int* halo_bound_down;
    // 1x1 problems in fp16x3 (st_conv1x1.hip): device bound on max |wgt| (plain fp32 [Cout][Cin] weights that
    // change every iteration, split while they are staged); nullptr -> exact fp32 kernel
    const unsigned int* wgt_amax;
    // optional [Cout][H][W]: out = (out_mask > 0) ? result : 0, applied last (after accumulate): the
    // threshold_backward of the NEXT data-gradient convolution, done while the gradient is produced
    const float* out_mask;
    // optional (any precision): fold max |out| of the finished output (after bias / ReLU / accumulate) into
    // this device bound (kAmaxWordUints unsigned ints), for the consumer's fp16 scale.  Zeroed once per pass.
    unsigned int* out_amax;
    // producer / consumer kernel only (st_conv_pc.hip): this launch produces output rows [row_begin, row_end) of the
    // image (0, 0 = all rows); operand rows outside the range are read from the same tensors.  Lets the launcher
    // cover an image with two tile shapes (see choose_pc_tile).
    int row_begin, row_end;
    // ... minus rows [row_skip_begin, row_skip_begin + row_skip_len) (row_skip_len == 0: nothing skipped;
    // row_skip_begin - row_begin must be a multiple of the tile height): the first and the last rows of a strip in ONE
    // launch (see overlap_part).
    int row_skip_begin, row_skip_len;
    // producer / consumer kernel, set by its launcher: Cout tiles dealt to groups of XCDs (1 = every XCD takes all Cout tiles
    // of its pixel tiles; see conv_pc_kernel's tile_of)
    int xcd_co_groups;
    // Strip plans, producer / consumer kernel only: a convolution split so that the halo exchange of its operand
    // overlaps most of it (SURVEY.md 8(e) "overlapped with interior compute").  0 = the whole strip in one go;
    // 1 = the INTERIOR rows [b, H - b), which read no halo row (in_halo must be null: the exchange may still be in
    // flight); 2 = the BOUNDARY rows [0, b) and [H - b, H) (in_halo set, launched after the exchange has landed).
    // b and both tile shapes come from conv_pc_overlap_choice(p), a pure function of the problem's shape.
    int overlap_part;
    // producer / consumer kernel only, forward: also write MaxPool2d(2) of the finished output, [Cout][H/2][W/2]
    // (reference style_transfer.py:21 'max').  Honoured only where conv_pc_fuses_pool(p) says so (tiles in which a
    // wave owns whole 2x2 windows, 16-byte store path); the caller launches the pool kernel otherwise.
    float* pool_out;
    // ... and, when this is non-null too, INSTEAD of the full-resolution output: one byte per pooled element, bits 0-1 =
    // position of the window's first maximum in row-major order (what the pooling backward scatters to), bit 2 = that
    // maximum is > 0 (the ReLU mask).  For conv outputs that nothing but the pool consumes (relu1_2, 2_2, 3_4, 4_4 in the
    // closure): the map is neither written by this launch nor re-read by the pooling backward.
    unsigned char* pool_code;
    // Winograd F(2x2, 3x3) form (st_conv_wino.hip): the layer's transformed weight planes (launch_winograd_weights; the forward
    // or the data-gradient set, matching wgt_split) and when to use them - 0 never, 1 where conv_wino_preferred() says the
    // measured time is lower, 2 wherever the kernel takes the problem (operator precision code 5, A/B runs)
    const void* wgt_wino;
    int wino;
};
// A bound lives in kAmaxSlots slots, one per 256-byte line: workgroup b commits to slot b % kAmaxSlots so that
// the ~2000 waves resident when a kernel starts (all of which see an empty bound) do not serialise on one
// address; the consumer takes the maximum over the slots.  Only the EXPONENT of the bound matters.
constexpr int kAmaxSlots = 32;
constexpr int kAmaxSlotStride = 64;                                  // unsigned ints between slots
constexpr int kAmaxWordUints = kAmaxSlots * kAmaxSlotStride;         // footprint of one bound
#if defined(__HIPCC__)
// Fold a thread's max |v| (raw bits; non-negative floats order like unsigned integers) into the bound: wave
// reduction, then at most one atomic per wave, skipped unless it raises the slot's exponent (the read may be
// stale, but slots only grow).  All 64 lanes must call it.
__device__ __forceinline__ void amax_commit(unsigned int m, unsigned int* bound) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned int o = (unsigned int)__shfl_xor((int)m, off);
        m = o > m ? o : m;
    }
    unsigned int* slot = bound + (blockIdx.x % kAmaxSlots) * kAmaxSlotStride;
    // plain (cacheable, possibly stale) read: a device-scope load here costs every wave a memory round trip at
    // the very end of its life
    if ((threadIdx.x & 63) == 0 && (m >> 23) > (*slot >> 23)) atomicMax(slot, m);
}
// the bound, wave-uniform; every lane of the wave must call it
__device__ __forceinline__ unsigned int amax_read(const unsigned int* bound) {
    unsigned int m = bound[(threadIdx.x % kAmaxSlots) * kAmaxSlotStride];
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) {
        const unsigned int o = (unsigned int)__shfl_xor((int)m, off);
        m = o > m ? o : m;
    }
    return (unsigned int)__builtin_amdgcn_readfirstlane((int)m);
}
// Workgroups are dealt to the 8 XCDs (private L2 each) round-robin by their LINEAR id.  logical_block() turns that id into one
// whose consecutive values run on the SAME XCD (XCD x takes the contiguous range [x total / 8, (x + 1) total / 8)), so that
// workgroups which read the same operand - the Cout tiles of one pixel tile, the tile pairs of one Gram split - share it
// through one L2 instead of fetching it into up to 8 of them (round 6; the 3 x 3 kernels have done this since round 1).
// Placement only: which workgroup computes what is unchanged, results are bit-identical.  remap == 0: the plain order.
__device__ __forceinline__ unsigned int logical_block(int remap) {
    const unsigned int linear = blockIdx.y * gridDim.x + blockIdx.x, total = gridDim.x * gridDim.y;
    if (!remap || (total & 7u) != 0) return linear;
    return (linear & 7u) * (total >> 3) + (linear >> 3);
}
__device__ __forceinline__ unsigned int abs_bits(float v) { return __builtin_bit_cast(unsigned int, v) & 0x7fffffffu; }
// fp16 mode: exponent e with bound * 2^e in [2^13, 2^14), from the bits of the bound on max|x| (0 for 0 /
// denormal / inf / nan).  fp16 overflows at 2^16: two spare bits, one of which the x2 average pooling and the
// L2 pooling (<= 1.56 x their input's maximum) may use when a pooled tensor reuses its input's bound.
// the operand's bound with the neighbours' halo rows' (ConvProblem::halo_bound_up / _down; wave-uniform scalar loads)
__device__ __forceinline__ unsigned int amax_with_halo(unsigned int own, const unsigned int* up, const unsigned int* down) {
    if (up) { const unsigned int u = up[0] & 0x7fffffffu; own = u > own ? u : own; }
    if (down) { const unsigned int d = down[0] & 0x7fffffffu; own = d > own ? d : own; }
    return own;
}
__host__ __device__ __forceinline__ int scale_exp(unsigned int amax_bits) {
    const int ef = (int)((amax_bits >> 23) & 0xffu);
    if (ef == 0 || ef == 255) return 0;
    const int e = 14 - (ef - 126);                    // bound < 2^(ef - 126)
    return e > 120 ? 120 : (e < -120 ? -120 : e);
}
__device__ __forceinline__ float pow2f(int e) { return __builtin_bit_cast(float, (unsigned int)(127 + e) << 23); }
#endif
int launch_conv_split(const ConvProblem& p, hipStream_t stream);
// Winograd F(2x2, 3x3) fp16x3 form of the same convolution (st_conv_wino.hip; builds with --experiments only)
#if defined(ST_EXPERIMENTS)
size_t winograd_weight_bytes(int cin, int cout);
int launch_winograd_weights(const float* w_torch, void* out, int cin, int cout, int dgrad, hipStream_t s);
bool conv_wino_applies(const ConvProblem& p);
bool conv_wino_preferred(const ConvProblem& p);   // ... and expected faster than the direct producer / consumer kernel
int launch_conv_wino(const ConvProblem& p, hipStream_t s);
#else
inline size_t winograd_weight_bytes(int, int) { return 256; }
inline int launch_winograd_weights(const float*, void*, int, int, int, hipStream_t) {
    set_error("the Winograd convolution (precision code 5) needs a library built with build.py --experiments");
    return 1;
}
inline bool conv_wino_applies(const ConvProblem&) { return false; }
inline bool conv_wino_preferred(const ConvProblem&) { return false; }
inline int launch_conv_wino(const ConvProblem&, hipStream_t) { return launch_winograd_weights(nullptr, nullptr, 0, 0, 0, nullptr); }
#endif
// fold max |x[0..n)| into a device bound (single = 0: kAmaxSlots-slot bound; 1: one word, the weight trailer)
int launch_amax(const float* x, long long n, unsigned int* word, int single, hipStream_t s);
// producer / consumer form of the unsharded fp16x3 3x3 convolution (st_conv_pc.hip)
bool conv_pc_applies(const ConvProblem& p);
bool conv_pc_preferred(const ConvProblem& p);      // ... and measured faster than the single-role kernel
int launch_conv_pc(const ConvProblem& p, hipStream_t stream);
// "fat" single-role form for large maps (st_conv_fat.hip): four waves of (32 CB) co x 128 px register tiles, staging inside the MFMA streams
bool conv_fat_applies(const ConvProblem& p);
bool conv_fat_preferred(const ConvProblem& p);     // ... and measured faster than the producer / consumer kernel
int launch_conv_fat(const ConvProblem& p, hipStream_t stream);
bool conv1x1_split_applies(const ConvProblem& p);
int launch_conv1x1_split(const ConvProblem& p, hipStream_t stream);
int launch_conv_splitk_reduce(const ConvProblem& p, int ksplit, hipStream_t stream);
// conv_precision code of the C ABI (0 fp32, 2 bf16x3, 3 bf16x6, 4 fp16x3) -> planes / element type
inline bool conv_precision_valid(int code) { return code == 0 || code == 2 || code == 3 || code == 4; }
inline int conv_precision_planes(int code) { return code == 4 ? 2 : code; }
inline int conv_precision_elem(int code) { return code == 4 ? 1 : 0; }
inline size_t split_weight_bytes(int cin, int cout, int planes) { return (size_t)cin * cout * 9 * 2 * planes + 256; }
// torch [Cout][Cin][3][3] -> 16-bit planes (+ trailer) for launch_conv_split (dgrad: roles swapped, taps rotated)
int launch_relayout_split(const float* w, void* out, int cin, int cout, int dgrad, int planes, int elem, hipStream_t s);
// Split-K: layers whose output has too few 32x32 MFMA tiles to fill 256 CUs (deep layers at small
// images) split the input-channel range over `ksplit` workgroups; raw partial sums go to `scratch`
// and a fixed-order reduce applies bias / ReLU / accumulate.  8M floats covers every case where the
// heuristic splits (ksplit * Cout * H * W <= ~4.2M by construction).
constexpr size_t kConvScratchFloats = (size_t)8 << 20;
int launch_conv(const ConvProblem& p, hipStream_t stream);
double conv_flops(const ConvProblem& p);   // algorithmic 2*taps*Cin*Cout*H*W

// torch [Cout][Cin][3][3] -> forward layout [9][Cin][Cout]
int launch_relayout_fwd(const float* w, float* out, int cin, int cout, hipStream_t stream);
// torch [Cout][Cin][3][3] -> data-gradient layout [9][Cout][Cin] with the taps rotated by 180 degrees
int launch_relayout_dgrad(const float* w, float* out, int cin, int cout, hipStream_t stream);

// Boundary rows of a [C][H][W] map into two contiguous [C][W] send buffers (row 0 -> up, row H-1 ->
// down); with `mask` the rows are multiplied by (mask > 0) (threshold_backward on the sender side).
// bounds != nullptr: also max |packed row| of either direction as raw bits into bounds_up[0] / bounds_down[0] (the message
// trailers); `scratch` = kPackScratchUints words of the plan, the last one a ticket that is zero between launches
constexpr int kPackScratchUints = 2 * 512 * 8 + 64;
int launch_pack_rows(const float* src, const float* mask, int channels, int height, int width, float* out_up,
                     float* out_down, hipStream_t s, unsigned int* bounds_up = nullptr, unsigned int* bounds_down = nullptr,
                     unsigned int* scratch = nullptr);

// ---- first layer (st_conv_first.hip) -----------------------------------------------------------
// conv1_1: Normalize + replicate pad + 3->64 conv + bias + ReLU (style_transfer.py:30-31,39,85-87)
int launch_conv_first_fwd(const float* image, const float* w /*[64][3][3][3]*/, const float* b, float* out,
                          int height, int width, hipStream_t stream, const float* halo = nullptr,
                          int has_up = 0, int has_down = 0, unsigned int* out_amax = nullptr);
// its data gradient incl. ReLU mask (relu_out == nullptr: grad_out is already masked by its producer),
// replicate-pad fold and 1/std; accumulates into grad_image
// dp_scratch: 3 * (height + 2) * (width + 2) floats (dP on the padded domain, folded by a second kernel)
// conv1_1 forward + relu1_1's partial moments in one pass (st_conv_first.hip): *splits workgroups' partials for
// launch_gram_finalize
bool conv_first_gram_applies(int height, int width, const float* image, const float* out, int max_splits);
int launch_conv_first_fwd_gram(const float* image, const float* w, const float* b, float* out, int height, int width,
                               hipStream_t stream, unsigned int* out_amax, float* partial, float* partial_sum, int max_splits,
                               int* splits, float w_l1max, float b_max);
// dp_scratch holds `parts` partial planes of 3 (height + 2) (width + 2) floats; parts = conv_first_dgrad_parts(GLOBAL height,
// width): the channel slices whose partial sums the fold kernel adds in order (1 on large images)
int conv_first_dgrad_parts(int height, int width);
// update (optional, unsharded plans): the fold kernel also applies st_plan_step's Adam + clamp + EMA update to the gradient
// element it has just finished (FoldUpdate, below) - the update is then not a launch of its own
struct FoldUpdate;
int launch_conv_first_dgrad(const float* grad_out, const float* relu_out, const float* w, float* grad_image,
                            float* dp_scratch, int height, int width, int accumulate, hipStream_t stream,
                            const float* ghalo = nullptr, int has_up = 0, int has_down = 0, int parts = 1,
                            const FoldUpdate* update = nullptr);

// ---- pooling (st_pool.hip) ---------------------------------------------------------------------
int launch_pool_fwd(const float* in, float* out, int channels, int height, int width, int mode, hipStream_t s);
bool conv_pc_fuses_pool(const ConvProblem& p);     // st_conv_pc.hip: will launch_conv(p) write p.pool_out?
int fold_halo_amax(const ConvProblem& p, hipStream_t stream);     // st_conv_split.hip
// st_conv_pc.hip: how a strip's convolution is cut into interior + boundary launches (overlap_part), and whether the cost
// model expects that to pay (split cost <= whole cost + the exchange latency it hides).  `p` = the whole problem
// (overlap_part ignored; in_halo may be null).  Returns false when the kernel does not take the problem at all.
struct PcOverlap {
    int rows_b;                 // boundary rows at the top (= the boundary tile's height)
    int rows_bottom;            // boundary rows at the bottom (a multiple of it)
    int shape_i, tw_i;          // interior tile
    int shape_b, tw_b;          // boundary tile (tile height == rows_b)
    double cost_split, cost_whole;      // microseconds (cost model)
    bool pays;
    bool pool;                  // both launches write the fused max pool (p.pool_out != null and both tiles can)
};
bool conv_pc_overlap_choice(const ConvProblem& p, PcOverlap* out);
// grad_in[C][H][W] (fully written, zeros in dropped odd rows/cols) from grad_out[C][H/2][W/2]
int launch_pool_bwd_codes(const unsigned char* code, const float* grad_out, float* grad_in, int channels, int height,
                          int width, hipStream_t s);
int launch_pool_bwd(const float* in, const float* grad_out, float* grad_in, int channels, int height,
                    int width, int mode, hipStream_t s);

// ---- Gram / moments (st_gram.hip) --------------------------------------------------------------
struct GramWorkspace {
    float* partial;      // [splits][C][C]
    float* partial_sum;  // [splits][C]
    int max_splits;
};
int gram_choose_splits(int channels, long long npix, int max_splits);
// the pixels of one split, split s owns [s per_split, min((s + 1) per_split, npix)): the even share rounded up to a multiple of
// 4, so the last splits of the grid may be short or empty
long long gram_per_split(long long npix, int splits);
// does the fp16x3 pass (a bound is there) run its 128 x 128-tile kernel on this shape?  (ST_GRAM_WIDE)
bool gram_wide_tiles(int channels, long long npix);
// partial[s] = F[:, ks:ke] F[:, ks:ke]^T, partial_sum[s] = row sums; F is [C][npix]
// bound != nullptr: fp16x3 arithmetic, scaled by the device bound on max |feat| (see ConvProblem::amax_word)
// sqrt_mask (optional, [npix]): s = sqrt(m) of a spatial mask m - the staged values become F diag(s), the partials
// F diag(m) F^T and F m (st_mask.hip has the pyramid that makes s)
int launch_gram_partial(const float* feat, int channels, long long npix, int splits, GramWorkspace ws,
                        hipStream_t s, const unsigned int* bound = nullptr, const float* sqrt_mask = nullptr);
// mean = sum/npix, srm = sum/npix (fixed-order reduction over splits); mask_sum > 0: the normaliser of masked partials, the
// sum of m, in the place of npix
int launch_gram_finalize(GramWorkspace ws, int channels, long long npix, int splits, float* mean, float* srm,
                         hipStream_t s, float* cov = nullptr, float cov_eps = 0.f,   // cov: also srm - mean mean^T + eps I
                         float mask_sum = 0.f);

// ---- small dense algebra for the W2 style loss (st_smallgemm.hip) ------------------------------
enum GemmEpilogue {
    EPI_SCALE = 0,         // D = c * P1
    EPI_IDENT_MINUS = 1,   // D = (cI * I - P1) * c
    EPI_DIFF = 2,          // D = (P1 - P2) * c
    EPI_DEV_SQRT_SCALE = 3 // D = P1 * sqrt(*dev_scalar)
};
struct GemmProblem {
    const float* a1; const float* b1;     // P1 = op(a1) @ op(b1)
    const float* a2; const float* b2; const float* b2sub;  // P2 = op(a2) @ (b2 - b2sub)  (EPI_DIFF only)
    float* d;
    int ta1, tb1, ta2;                    // 1 = operand is used transposed
    int epilogue;
    float c, ci;
    const float* dev_scalar;
    int n;                                // 0: the batch's n; else this problem's own size (mixed batches, n <= 256)
    float* sumsq_partials;                // n = 512 only (gemm_sumsq_fusable): partials[tile] = sum of D^2 over the tile, the
                                          // operand of ns_prepare / the backward chain's entry instead of a launch of its own
};
bool gemm_sumsq_fusable(int n);           // launch_gemm_batch honours GemmProblem::sumsq_partials for this size: (n / 32)^2 partials
struct GemmBatch {
    GemmProblem p[6];                     // (6: both products of a recurrence step for three chains in lockstep)
    int count;
    int n;                                // all matrices n x n, n % 32 == 0 (problems may override it, see GemmProblem::n)
};
int launch_gemm_batch(const GemmBatch& b, hipStream_t s);
// dF = Ssym F + b 1^T for a style tap of <= 1024 pixels in one launch (st_smallgemm.hip); mask: optional [C][npix], out = 0
// where mask <= 0; out_amax: optional bound for an fp16x3 consumer
bool head_dgrad_small_applies(int channels, long long npix);
int launch_head_dgrad_small(const float* ssym, const float* feat, const float* bias, const float* mask, float* out, int channels,
                            long long npix, unsigned int* out_amax, hipStream_t s);

struct NSWorkspace {                      // all n*n unless noted
    float *y0, *y1, *z0, *z1, *t;         // forward iterates
    float *a0, *a1, *q0, *q1, *e, *atq, *qa;  // backward iterates
    float* scalars;                       // [4] device scalars: ||M||_F, ||S||_F, spare
    // fp16x3 chains (st_nsgemm.hip, n >= 256): 5 matrix slots x 2 roles x 2 planes of n*n halves
    // (forward y, y', z, z', t; the backward reuses them for a, a', q, q', E)
    _Float16* planes;
    // persistent chain kernel (st_nschain.hip): two sets of barrier words used by alternate launches (a launch clears the
    // other set) + the error word; zero when the workspace is put to use (ns_workspace_reset)
    unsigned int* chain_sync;
    int chain_launches;
    float* chain_arena;                   // kNsChainArenaMats matrices when ST_NS_CHAIN_L2=2 asked for them at carve time, else null
};
constexpr int kNsChainArenaMats = 132;    // forward 4 + 2 + 11 x 2 + 10 x 4 = 68, backward 3 + 12 x 2 + 11 x 2 + 10 = 59

// ---- persistent Newton-Schulz chains (st_nschain.hip) ------------------------------------------------
struct NsChainJob {
    int n;
    int tile0, tiles;                     // set by launch_ns_chain: first workgroup and workgroup count of the job
    int forward, backward;                // which recurrences run (both: sqrtm.py:9-25 then :36-47 for a seed gdiag * I)
    const float* m;                       // forward: the matrix whose root is taken (its upper triangle is read)
    const float* m_partials;              // optional: m_nparts partial sums of squares of m (left by the product that made it)
    int m_nparts;
    int l2_loads;                         // 1: operands through the L2 (plain loads behind an acquire per barrier) instead of sc1 loads
    int symmetric;                        // 1: only the tile pairs ti <= tj of every product + mirror images (exactly symmetric
                                          // iterates, -47 % work; costs accuracy on ill-conditioned input, see st_nschain.hip);
                                          // 0: every tile, every iterate kept as X and X^T (the reference's products, faithfully)
    float *y0, *y1, *z0, *z1, *t;         // n x n workspace matrices (the backward keeps a in y's slots, q in z's, E in t's)
    float *yt0, *yt1, *zt0, *zt1, *tt;    // full jobs: their transposes
    float* arena;                         // optional, with l2_loads: kNsChainArenaMats n x n matrices - every iterate of every step
                                          // gets its own (no address is read before it is written within a launch: no acquire)
    float* root;                          // forward: result; backward only: operand
    float* grad_m;                        // backward: result, dL/dM
    float* scalars;                       // [0] = ||m||_F, [1] = ||root||_F, [8 ..] tile partial sums
    const float* gdiag_dev;               // the seed: a device scalar, or (null) the host value below, or the W2 job's own
    float gdiag;
    W2LossJob loss;                       // optional: the head's loss scalars ride along (loss_out == nullptr: none)
    unsigned int *sync, *sync_next, *error;
};
struct NsChainLaunch {
    NsChainJob job[3];
    int count;
};
#if defined(ST_EXPERIMENTS)
int ns_chain_mask();                      // ST_NS_CHAIN: bit 0 shallow heads, 1 relu4_1, 2 relu5_1, 3 standalone operators
bool ns_chain_enabled();                  // any bit
int ns_chain_sync_uints();                // barrier words per set
int ns_chain_tiles(int n, bool symmetric); // workgroups of a job
int launch_ns_chain(NsChainLaunch& launch, hipStream_t s);
#else                                     // default build: no persistent chain kernel, the callers' branches fold away
inline int ns_chain_mask() { return 0; }
inline bool ns_chain_enabled() { return false; }
inline int ns_chain_sync_uints() { return 16; }
inline int ns_chain_tiles(int, bool) { return 0; }
inline int launch_ns_chain(NsChainLaunch&, hipStream_t) {
    set_error("the persistent Newton-Schulz chain kernel needs a library built with build.py --experiments");
    return 1;
}
#endif
bool ns_chain_combined();                 // ... and neither ST_NS_FULL_BACKWARD nor ST_NS_F16_FWD asks for another recurrence
// the job of a workspace: matrices, scalars, this launch's barrier words (advances the workspace's launch parity)
NsChainJob ns_chain_job(NSWorkspace& ws, int n);
int ns_workspace_reset(NSWorkspace& ws, hipStream_t s);     // zero the barrier / error words (after ns_workspace_carve)
// forward + backward chain of one head (or up to three heads) in ONE launch; loss[i] may be null
int ns_sqrt_chain(const float* const* m, float* const* root, float* const* grad_m, const int* n, NSWorkspace* const* ws,
                  const int* m_partials, const W2LossJob* loss, int lanes, hipStream_t s);
// after a synchronise: has a chain kernel of this workspace given up waiting (a workgroup never became resident)?
int ns_chain_check(NSWorkspace& ws, const char* what);

// ---- fp16x3 Newton-Schulz products (st_nsgemm.hip) -----------------------------------------------
// scale exponent of a plane pair: stored = value * 2^exp.  Either a host constant, or (num != nullptr) derived on
// the device from the bound |num[0] / den[0]| * mult (the Lyapunov iterate q, whose magnitude is a device scalar).
struct NsScale {
    int exp;
    const float* num;
    const float* den;
    float mult;
};
struct NsPlanes {                          // operand: role-A blocks of A, or role-B blocks of B (see st_nsgemm.hip)
    const _Float16* p0;
    const _Float16* p1;
    NsScale scale;
};
struct NsPlanesOut {                       // result planes in role A and / or role B (nullptr = not needed)
    _Float16 *a0, *a1, *b0, *b1;
    NsScale scale;
};
struct NsGemmProblem {
    NsPlanes a, b;                         // D = A @ B
    float* d32;                            // optional fp32 row-major result
    NsPlanesOut out;
    int epilogue;                          // EPI_SCALE, EPI_IDENT_MINUS or EPI_DEV_SQRT_SCALE
    float c, ci;
    const float* dev_scalar;
};
struct NsGemmBatch {
    NsGemmProblem p[2];
    int count;
    int n;
};
struct NsToPlanesItem {
    const float* src;
    NsPlanesOut out;
};
struct NsToPlanes {
    NsToPlanesItem item[2];
    int count;
};
bool ns_f16_applies(int n);
int launch_ns_gemm_f16(const NsGemmBatch& b, hipStream_t s);
int launch_ns_planes_from_f32(const NsToPlanes& job, int n, hipStream_t s);
int ns_sqrt_forward_f16(const float* m, float* root, int n, NSWorkspace& ws, hipStream_t s);
int ns_sqrt_backward_diag_f16(const float* root, const float* grad_diag, float* grad_m, int n, NSWorkspace& ws,
                              hipStream_t s, const W2LossJob* loss = nullptr, int root_partials = 0);
// csrc/st_diag.hip: shares[i] = 1 if candidates[i] sits on the same hardware queue as `ref` (returns 1 if undecidable)
int probe_queue_sharing(hipStream_t ref, const hipStream_t* candidates, int count, int* shares);
size_t ns_workspace_floats(int n);
void ns_workspace_carve(NSWorkspace& ws, float* base, int n);
// m_partials > 0: ws.scalars + 8 already holds that many partial sums of squares of m (written by the product that made m);
// root_partials != nullptr: the last product leaves root's partial sums there too and reports their count (0: not fused)
int ns_sqrt_forward(const float* m, float* root, int n, NSWorkspace& ws, hipStream_t s, int m_partials = 0,
                    int* root_partials = nullptr);
// up to three fp32 chains of DIFFERENT sizes (n <= 256 each) in lockstep: every recurrence step is one launch for all
int ns_sqrt_forward_lockstep(const float* const* m, float* const* root, const int* n, NSWorkspace* const* ws, int lanes,
                             hipStream_t s);
int ns_sqrt_backward_diag_lockstep(const float* const* root, const float* const* grad_diag, float* const* grad_m, const int* n,
                                   NSWorkspace* const* ws, int lanes, hipStream_t s, const W2LossJob* loss = nullptr);
// grad_diag != nullptr: grad_root = (*grad_diag_value) * I with the value read on device from grad_diag[0].
// loss (diag form only): the head's W2 scalars are computed by the chain's opening kernel, which then also WRITES
// grad_diag[0] (= loss->gdiag_out) instead of reading it.
// root_partials > 0: ws.scalars + 8 holds that many partial sums of squares of root (ns_sqrt_forward's root_partials)
int ns_sqrt_backward(const float* root, const float* grad_root, const float* grad_diag, float* grad_m, int n,
                     NSWorkspace& ws, hipStream_t s, const W2LossJob* loss = nullptr, int root_partials = 0);

// ---- pointwise / reductions (st_pointwise.hip) -------------------------------------------------
int launch_fill(float* p, long long n, float v, hipStream_t s);
int launch_identity(float* p, int n, hipStream_t s);
// cov = srm - mean mean^T + eps I
int launch_cov_from_moments(const float* mean, const float* srm, float* cov, int n, float eps, hipStream_t s);
// out[0] = ||a||_F
int launch_frobenius(const float* a, long long count, float* out, hipStream_t s);
// norm = ||a||_F -> norm_out[0]; a_scaled = a / norm; second = I (g, gdiag null), g / norm, or (gdiag[0] / norm) I.
// `partials`: >= 256 floats of scratch.  Two launches.
int launch_sumsq_partials(const float* a, long long count, float* partials, int* nparts, hipStream_t s);
int launch_ns_prepare(const float* a, int n, float* norm_out, float* partials, float* a_scaled, const float* g,
                      const float* gdiag, float* second, hipStream_t s, bool first_t = false,
                      const W2LossJob* loss = nullptr, int partials_ready = 0);   // > 0: `partials` is filled already
// y = a / *scalar
int launch_div_by_dev_scalar(const float* a, const float* scalar, float* y, long long count, hipStream_t s);
// q = (diag_value[0] / *scalar) * I
int launch_scaled_identity_div(const float* diag_value, const float* scalar, float* q, int n, hipStream_t s);

// ContentLossMSE value + gradient: loss_out[0] = weight * mean((f-t)^2); grad = weight * 2 (f-t) / count (accumulate != 0:
// added to what grad holds)
// partials: kStreamBlocks floats (content) / 4 * kStreamBlocks floats (TV).  ticket != nullptr: a zeroed device word;
// the value is then finished by the kernel's last block (one launch instead of two)
constexpr int kStreamBlocks = 2048;
int launch_content_mse(const float* feat, const float* target, long long count, float weight, float* grad,
                       float* partials, float* loss_out, hipStream_t s, unsigned int* ticket = nullptr, int accumulate = 0);
// ScaledMSELoss (ContentLoss on features, StyleLoss on Gram matrices) in two launches on `count` floats, see st_pointwise.hip:
// the sums - totals[0] = sum d^2, totals[1] = sum |d| + eps, loss_out[0] = weight totals[0] / totals[1]; partials: 2 floats
// per block, at most 2 kStreamBlocks; ticket: a zeroed device word - then the content seed from them,
// grad = weight (2 d - L sgn d) / S1 (accumulate != 0: added to what grad holds)
constexpr float kScaledMseEps = 1e-8f;            // ScaledMSELoss eps (style_transfer.py:97): what a plan passes; a standalone head its module's
int launch_scaled_mse_sums(const float* x, const float* target, long long count, float weight, float* partials, float* totals,
                           float* loss_out, hipStream_t s, unsigned int* ticket, float eps = kScaledMseEps);
int launch_scaled_mse_grad(const float* feat, const float* target, long long count, float weight, const float* totals,
                           float* grad, hipStream_t s, int accumulate = 0);
// The three launches above under a spatial weight map (st_plan_set_content_mask): the tap is [count / npix][npix] and element i
// is weighed by wmap[i % npix] - mse: term = weight sum w d^2 / count, seed = weight (2 / count) w d; scaled_mse: S2 = sum w d^2,
// S1 = sum w |d| + eps, seed = weight w (2 d - L sgn d) / S1.  A ticket word is required; a map of ones gives the bits above.
int launch_content_mse_weighted(const float* feat, const float* target, const float* wmap, long long count, long long npix,
                                float weight, float* grad, float* partials, float* loss_out, hipStream_t s, unsigned int* ticket,
                                int accumulate = 0);
int launch_scaled_mse_sums_weighted(const float* x, const float* target, const float* wmap, long long count, long long npix,
                                    float weight, float* partials, float* totals, float* loss_out, hipStream_t s,
                                    unsigned int* ticket, float eps = kScaledMseEps);
int launch_scaled_mse_grad_weighted(const float* feat, const float* target, const float* wmap, long long count, long long npix,
                                    float weight, const float* totals, float* grad, hipStream_t s, int accumulate = 0);
// ... or, for a Gram head, (Ssym, b) of its 1x1 step: ssym = (weight / npix) (D + D^T), D = dL/dG from the totals; bvec = 0
// (mask_sum > 0, here and in launch_style_grad_finish: a masked head's normaliser in the place of npix)
int launch_gram_grad_finish(const float* gram, const float* gram_t, const float* totals, int n, float weight, long long npix,
                            float* ssym, float* bvec, hipStream_t s, unsigned int* ssym_amax = nullptr, float mask_sum = 0.f);
// st_plan_backward's seeding: g = ext (accumulate == 0) or g += ext over `count` elements; relu_out (optional): the result
// is masked by (relu_out > 0); bound (optional): max |g| folded into that device bound for an fp16x3 consumer
int launch_seed_grad(const float* ext, const float* relu_out, float* g, long long count, int accumulate, unsigned int* bound,
                     hipStream_t s);
// W2 head scalars after the NS forward.  loss_out[0] = weight * (mean((mu-mu_t)^2) + mean(diag(cov_t + cov - 2 root)))
// gdiag_out[0] = -2 * (weight / n)   (the diagonal value of dL/d root)
int launch_style_loss_value(const float* mean, const float* mean_t, const float* cov, const float* cov_t,
                            const float* root, int n, float weight, float* loss_out, float* gdiag_out,
                            hipStream_t s);
// dcov = at^T dT-product result `g` + (weight/n) I ; then
//   ssym[c][d] = (dcov[c][d] + dcov[d][c]) / npix,  bvec[c] = (2 weight (mu-mu_t)[c]/n - sum_d (dcov+dcov^T)[c][d] mu[d]) / npix
int launch_style_grad_finish(const float* g, const float* mean, const float* mean_t, int n, float weight,
                             long long npix, float* ssym, float* bvec, hipStream_t s,
                             unsigned int* ssym_amax = nullptr, float mask_sum = 0.f);
// ---- spatial style masks (st_mask.hip) ----------------------------------------------------------
constexpr int kMaskLevels = 5;                    // the image's resolution and one level per pooling of the trunk
constexpr int kMaskPyramidBlocks = 64;            // workgroups per level: their partial sums are added in a fixed order
// From mask [h[0]][w[0]] (values in [0, 1]): level k + 1 is the plain mean of the 2 x 2 cells of level k at floor sizes
// (h[k + 1] = h[k] / 2: avg_pool2d(m, 2)); sqrt_level[k] receives sqrt of level k.  stats (device, 8 doubles): [0..4] the sum
// of each level, [5] min and [6] max of the mask, [7] the number of NaNs in it; partials: kMaskLevels x kMaskPyramidBlocks x 4
// doubles.  Fixed-order sums, no atomics: two calls give the same bits.  store_root = false (the content and TV weight maps):
// the levels themselves are stored - level 0 is then a bit-exact copy of the mask; levels < kMaskLevels: only the first ones.
int launch_mask_pyramid(const float* mask, const int* h, const int* w, float* const* sqrt_level, double* partials, double* stats,
                        hipStream_t s, bool store_root = true, int levels = kMaskLevels);
// buf [c][npix] *= sqrt_mask[npix]^2 per pixel column: the masked heads' gradient step dF = (Ssym F + b 1^T) diag(m)
int launch_mask_columns(float* buf, const float* sqrt_mask, int channels, long long npix, hipStream_t s);
// ---- style regions (st_plan_set_style_regions): several masks with a style each --------------------
constexpr int kMaxRegions = 4;
// dst [c][npix] += sqrt_mask[npix]^2 * src [c][npix] per pixel column: region r >= 1's gradient step onto the seed that region 0
// wrote.  Two reads and one write of the tap; one thread owns an element, so the sum's order is the order of the launches.
int launch_mask_columns_add(float* dst, const float* src, const float* sqrt_mask, int channels, long long npix, hipStream_t s);
// out[j] = region_terms[0][j] + region_terms[1][j] + ... in region order (fp32), j < n_style; region_terms is [regions][n_style].
// One region: out[j] takes region_terms[0][j] as it is.
int launch_sum_region_terms(const float* region_terms, int regions, int n_style, float* out, hipStream_t s);
// ---- diagonal-covariance W2 heads (st_plan_set_w2_diagonal, st_op_channel_moments / st_op_w2_diag_*; st_w2diag.hip) ----
// The pixel range of every channel is cut into channel_stats_splits(npix) pieces - a function of the shape alone - and the
// scratch of a launch is 4 floats (the ticket's 16 bytes) and behind them two partials per (channel, split).
int channel_stats_splits(long long npix);
long long channel_stats_scratch_floats(int channels, long long npix);
// what the last block of the stats launch makes of a channel's sums: the moments (mean_out / srm_out, optional) and, with a
// target (mean_t, std_t), the weighted term and the gradient's coefficients coeffs = [a (C) | b (C)] (include/st_amd.h)
struct ChannelStatsFinish {
    const float* mean_t = nullptr;
    const float* std_t = nullptr;
    float eps = 0.f, weight = 1.f;
    double norm = 1.0;                  // M: the pixel count, or a mask level's sum
    float* coeffs = nullptr;
    float* loss_out = nullptr;
    float* mean_out = nullptr;
    float* srm_out = nullptr;
};
// scratch: channel_stats_scratch_floats floats whose first word is zero (the ticket; the launch leaves it zero); sqrt_mask
// (optional): [npix], the square root of the pixel weights
int launch_channel_stats(const float* feat, const float* sqrt_mask, int channels, long long npix, float* scratch,
                         const ChannelStatsFinish& fin, hipStream_t s);
// grad [C][npix] = (or, accumulate != 0: +=) (a_c feat + b_c) m_p; upstream (optional): a device scalar on a and b
int launch_channel_affine_grad(const float* feat, const float* sqrt_mask, const float* coeffs, const float* upstream, int channels,
                               long long npix, float* grad, int accumulate, hipStream_t s);
// a flagged head's target from the moments a W2 target is given: mean_t = mean, std_t = sqrt(max(srm_cc - mean_c^2, 0) + eps)
int launch_diag_target(const float* mean, const float* srm, int n, float eps, float* mean_t, float* std_t, hipStream_t s);
// ---- exact per-channel Wasserstein (sorted) W2 heads (st_plan_set_w2_marginal, st_op_channel_sort / st_op_w2_marginal_*; st_sort.hip) ----
constexpr int kMarginalBlocks = 1024;             // workgroups of the residual pass at most: its partials
constexpr long long kMarginalHeaderBytes = 8192;  // of a sort's scratch: the ticket's 16 bytes, at byte 256 the partials; then the keys
int sort_chunk();                                 // keys one workgroup sorts in LDS: 4096, or 8192 under the option ST_SORT_CHUNK
long long marginal_scratch_bytes(int channels, long long n);
// a scratch of marginal_scratch_bytes bytes, 256-byte aligned, as the launches below read it: two buffers of C n 64-bit keys
struct MarginalScratch {
    unsigned int* ticket = nullptr;     // zero between launches
    float* partials = nullptr;
    unsigned long long *keys_a = nullptr, *keys_b = nullptr;
};
MarginalScratch marginal_scratch_of(void* scratch, int channels, long long n);
// the rows of feat [C][n] in stable ascending order (ties by index, -0.0 as +0.0), as keys in m.keys_a: the order-preserving image
// of the value in the high word, the element's index in the low word
int launch_channel_sort(const float* feat, int channels, long long n, const MarginalScratch& m, hipStream_t s);
int launch_unpack_keys(const unsigned long long* keys, long long count, float* sorted_out, unsigned int* perm_out, hipStream_t s);
// out [C][n_out]: the quantile functions q [C][n_in] (sorted rows) at the n_out midpoints (include/st_amd.h); n_in == n_out: a copy
int launch_resample_quantiles(const float* q, int channels, long long n_in, long long n_out, float* out, hipStream_t s);
// the sort, then the residual pass against target [C][n]: grad [C][n] WRITTEN through the permutation, loss_out[0] the weighted term
int marginal_head_run(const float* feat, int channels, long long n, const float* target, void* scratch, float weight, float* grad,
                      float* loss_out, hipStream_t s);
// ---- nearest-neighbour feature-matching W2 heads (st_plan_set_style_nearest, st_op_nearest_*; st_nearest.hip) ----
constexpr int kNearestChunk = 32;                 // channels per K chunk of the search: a head's channel count is a multiple
constexpr int kNearestPixelTile = 128;            // pixels a workgroup of the search owns
constexpr int kNearestKTile = 128;                // style vectors per k tile: M is padded to a multiple
constexpr int kNearestMinTiles = 4;               // k tiles a split owns at least
long long nearest_m_pad(long long m);
int nearest_splits(long long n, long long m, int* tiles_per_split);     // by the shape alone
int nearest_check_shape(const char* who, int channels, long long n, long long m);
// the style set as the kernels read it, nearest_prepared_floats floats, 256-byte aligned: the bound on max |S|, bias [M_pad], S^T [M_pad][C]
long long nearest_prepared_floats(int channels, long long m);
struct NearestPrepared {
    long long m = 0, m_pad = 0;
    unsigned int* bound = nullptr;
    float *bias = nullptr, *st_t = nullptr;
    float* mu = nullptr;                // cosine metrics only: the centre [C] behind the rows (nearest_cosine_prepared_floats)
};
NearestPrepared nearest_prepared_of(float* prepared, int channels, long long m);
// per call, nearest_scratch_floats floats, 256-byte aligned: the ticket (zero between launches), a bound for a tap no trunk kernel
// wrote, the finish pass's partials, one (score, k) per pixel and split
long long nearest_scratch_floats(int channels, long long n, long long m);
struct NearestScratch {
    int splits = 1, tiles_per_split = 1;
    unsigned int *ticket = nullptr, *bound = nullptr;
    float *partials = nullptr, *part_score = nullptr;
    int* part_k = nullptr;
};
NearestScratch nearest_scratch_of(float* scratch, int channels, long long n, long long m);
// vectors [C][m] -> pr: the transpose with zero rows in the padding, bias_k = -|s_k|^2 / 2 (double, rounded once; -inf in the padding), the bound
int launch_nearest_prepare(const float* vectors, int channels, long long m, const NearestPrepared& pr, hipStream_t s);
// one (score, k) per pixel and split into sc; feat_bound: the tap's bound word, or null - measured into sc.bound first
int launch_nearest_search(const float* feat, int channels, long long n, const NearestPrepared& pr, const NearestScratch& sc,
                          const unsigned int* feat_bound, hipStream_t s);
// the search, then the finish pass: idx_out [n], score_out [n] (optional), grad [C][n] WRITTEN, loss_out[0] the weighted term
int nearest_head_run(const float* feat, int channels, long long n, const NearestPrepared& pr, const NearestScratch& sc,
                     const unsigned int* feat_bound, float weight, int* idx_out, float* score_out, float* grad, float* loss_out,
                     hipStream_t s);
// ---- cosine and centred-cosine matching of a nearest head (st_plan_set_nearest_metric, st_op_nearest_cosine_*; st_nearest.hip) ----
constexpr float kNearestCosineEps = 1e-8f;        // under both square roots: |s_k - mu|^2 + eps, |f_i - mu|^2 + eps (include/st_amd.h)
// L2's layout - the bound on max |s^| (at most 1), b [M_pad], s^T [M_pad][C] - and behind it mu [C], padded to 64 floats
long long nearest_cosine_prepared_floats(int channels, long long m);
// L2's layout (the finish pass has one block per 64 pixels: never more partials than L2's)
long long nearest_cosine_scratch_floats(int channels, long long n, long long m);
// vectors [C][m] -> pr: mu (0, or the mean over k in double in ascending k), s^_k = (s_k - mu) / sqrt(|s_k - mu|^2 + eps) and
// b_k = -<mu, s^_k> in double in channel order, each rounded once; zero rows and -inf in the padding; the bound
int launch_nearest_cosine_prepare(const float* vectors, int channels, long long m, int centered, const NearestPrepared& pr, hipStream_t s);
// the search (launch_nearest_search, unchanged), then the cosine finish pass: idx_out [n], grad [C][n] WRITTEN, loss_out[0] the weighted term
int nearest_cosine_head_run(const float* feat, int channels, long long n, const NearestPrepared& pr, const NearestScratch& sc,
                            const unsigned int* feat_bound, float weight, int* idx_out, float* grad, float* loss_out, hipStream_t s);
// ---- sliced Wasserstein W2 heads (st_plan_set_style_sliced, st_op_sliced_*; st_sliced.hip) ----
constexpr int kSlicedMaxImages = 16;              // style images a flagged entry keeps the feature vectors of
// C a multiple of 32 (the 1x1 step's chunk), P a multiple of 64 in [64, 512], rows of 1 <= n < 2^24 elements
int sliced_check_shape(const char* who, int channels, int proj, long long n);
// R [P][C] and R^T [C][P] of (seed, entry, epoch): include/st_amd.h writes the generator down
int launch_sliced_directions(unsigned long long seed, int entry, unsigned long long epoch, int proj, int channels, float* r, float* rt,
                             hipStream_t s);
// per call, sliced_scratch_bytes bytes, 256-byte aligned, for rows of at most n elements (the tap's pixels or a style image's
// vectors, whichever is more): three bound words (the operand in front of a projection, R, G), Y and G [P][n], the sort's scratch
long long sliced_scratch_bytes(int proj, long long n);
struct SlicedScratch {
    unsigned int *in_bound = nullptr, *r_bound = nullptr, *g_bound = nullptr;
    float *y = nullptr, *g = nullptr;
    void* sort = nullptr;               // marginal_scratch_bytes(P, n): its ticket is zero between launches
};
SlicedScratch sliced_scratch_of(void* scratch, int proj, long long n);
// out [Cout][npix] = W in, W given in both layouts: w [Cout][Cin] for the fp16x3 1x1 step, which runs when both bounds are given
// (in_bound on max |in|, w_bound on max |w|), wt [Cin][Cout] for the exact fp32 MFMA otherwise
int sliced_product(const float* in, int cin, int cout, long long npix, const float* w, const float* wt, const unsigned int* in_bound,
                   const unsigned int* w_bound, float* out, hipStream_t s);
// one style image's share of the target: T [P][n_out] = (accumulate ? T : 0) + weight resample_n_out(sort_rows(R feat)), feat [C][m]
int sliced_target_add(const float* feat, int channels, long long m, const float* r, const float* rt, int proj, long long n_out,
                      const SlicedScratch& sc, const unsigned int* feat_bound, const unsigned int* r_bound, float* target, int accumulate,
                      float weight, hipStream_t s);
// the head on feat [C][n]: Y = R feat, the sort and the residual pass against target [P][n] (G into the scratch, the weighted term to
// loss_out[0]), then grad [C][n] = R^T G WRITTEN.  Bounds null: the exact fp32 MFMA for both products
int sliced_head_run(const float* feat, int channels, long long n, const float* r, const float* rt, int proj, const float* target,
                    const SlicedScratch& sc, const unsigned int* feat_bound, const unsigned int* r_bound, float weight, float* grad,
                    float* loss_out, hipStream_t s);
// ---- Laplacian loss on pooled images (st_plan_set_laplacian, st_op_laplacian_*; st_laplacian.hip) ----
constexpr int kMaxLapPools = 4;
constexpr int kLapBlocks = 1024;                  // workgroups of the residual pass at most: its partials
// Q [C][H / p][W / p] = avg_pool2d(image [C][H][W], p) at floor sizes, each window summed row-major
int launch_lap_pool(const float* image, int C, int H, int W, int p, float* Q, hipStream_t s);
// target == nullptr: out = L(Q) on [C][h][w] (the target pass).  Otherwise out = r = L(Q) - target and term_out[0] =
// weight sum r^2 / (C h w) from partials (kLapBlocks floats), finished by the kernel's last block (ticket: a zeroed device
// word) or, without a ticket, by a second launch.  With a ticket: tv_out (optional) first receives slot[0], then slot[0] (optional)
// += the term - one thread, stream-ordered.
int launch_lap_residual(const float* Q, const float* target, int C, int h, int w, float weight, float* out, float* partials,
                        unsigned int* ticket, float* term_out, float* tv_out, float* slot, hipStream_t s);
// grad [C][H][W] (+)= (2 weight / (C h w p^2)) (L^T r)[y / p][x / p] inside the pooled region (accumulate != 0: added, the rest
// untouched; else written, zeros outside); upstream (optional): a device scalar that multiplies the factor
int launch_lap_grad(const float* r, int C, int H, int W, int p, float weight, const float* upstream, float* grad, int accumulate,
                    hipStream_t s);
// TV loss partial sums + gradient (optionally scaled by `weight`): see st_pointwise.hip.  wmap (st_plan_set_tv_mask): [height][width],
// every squared difference weighed by the mean of the map at its two end points; null: the unweighted kernels
int launch_tv(const float* image, int height, int width, float weight, float* grad, float* partials,
              float* loss_out, hipStream_t s, unsigned int* ticket = nullptr, const float* wmap = nullptr);
// Strip of a larger image: local rows [row0, row0 + height) of `global_height`; halo = [2][3][W] rows of the
// neighbours (nullptr / has_* == 0 at the global border).  Writes the gradient and sums[4] = the four
// sums of squared differences owned by this strip (to be all-reduced), no final value.
struct StripInfo {
    int row0, global_height, has_up, has_down;
    const float* halo;
};
int launch_tv_strip(const float* image, int height, int width, StripInfo strip, float weight, float* grad,
                    float* partials, float* sums4, hipStream_t s);
float* tv_debug_buffer();     // diagnostic (ST_TV_VARIANT=3, st_plan_debug_read what = 1)
int launch_tv_final(const float* sums4, int global_height, int width, float weight, float* loss_out, hipStream_t s);
// content MSE on a strip: gradient with the GLOBAL element count, sum of squares into sum_out[0]
int launch_content_mse_strip(const float* feat, const float* target, long long local_count,
                             long long global_count, float weight, float* grad, float* partials,
                             float* sum_out, hipStream_t s);
int launch_content_mse_final(const float* sum, long long global_count, float weight, float* loss_out, hipStream_t s);
// y = a / d (host scalar)
int launch_div_by_scalar(const float* a, float d, float* y, long long count, hipStream_t s);
// total = ((((((l0 + l1) + l2) + l3) + l4) + l5) + l6)   (SumLoss order)
int launch_sum_losses(float* losses8, hipStream_t s, float* copy = nullptr);
// a configured plan's terms (n_content + n_style + 1 floats, SumLoss order) folded into the 8-float array (and its copy)
int launch_sum_terms(const float* terms, int n_content, int n_style, float* losses8, hipStream_t s, float* copy = nullptr);
struct AdamScalars {
    float lerp_w;        // (float)(1 - beta1)
    float beta2;         // (float)beta2
    float one_m_beta2;   // (float)(1 - beta2)
    float step_size;     // (float)(lr / (1 - beta1^step))
    float bc2_sqrt;      // (float)sqrt(1 - beta2^step)
    float eps;
    float decay;         // fp32 EMA decay
    float one_m_decay;   // 1 - decay evaluated in fp32
};
// Work that used to be launches of its own around the update (round 6: two dependent launches less per iteration on the
// caller's stream): the total of the seven loss terms (sum_losses_kernel's arithmetic, by one thread) and the zeroing of the
// fp16x3 operand bounds for the NEXT forward pass.  All fields optional.
struct AdamTail {
    float* losses8;            // [7 terms | total]: total = 0 + l0 + ... + l6
    float* losses_copy;        // the caller's 8-float result buffer (may be null)
    unsigned int* zero;        // words to clear
    long long zero_count;
};
int launch_adam_clamp_ema(float* image, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema,
                          long long count, AdamScalars sc, hipStream_t s, AdamTail tail = AdamTail{});
// st_plan_step's update handed to conv1_1's fold kernel (launch_conv_first_dgrad): state tensors [3][H][W] like the gradient
struct FoldUpdate {
    float* image;
    float* exp_avg;
    float* exp_avg_sq;
    float* ema;
    AdamScalars sc;
    AdamTail tail;
};
#if defined(__HIPCC__)
// torch.optim.Adam single-tensor step (torch/optim/adam.py:414-547, as configured at style_transfer.py:458) +
// image.clamp_(0, 1) (:485) + EMA.update (:250-253) on one element; every operation rounded on its own (no contraction)
__device__ __forceinline__ void adam_clamp_ema_element(float g, float& m, float& v, float& p, float& e, const AdamScalars& sc) {
#pragma clang fp contract(off)
    m = __builtin_fmaf(sc.lerp_w, g - m, m);                 // exp_avg.lerp_(grad, 1 - beta1)
    v = v * sc.beta2;                                        // exp_avg_sq.mul_(beta2)
    v = v + (sc.one_m_beta2 * g) * g;                        //   .addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / sc.bc2_sqrt + sc.eps;     // (exp_avg_sq.sqrt() / bc2_sqrt).add_(eps)
    p = p - sc.step_size * (m / denom);                      // param.addcdiv_(exp_avg, denom, value=-step_size)
    p = fminf(fmaxf(p, 0.f), 1.f);                           // image.clamp_(0, 1)
    e = e * sc.decay;                                        // self.value *= self.decay
    e = e + sc.one_m_decay * p;                              // self.value += (1 - self.decay) * input
}
// AdamTail by the threads of a 1-D grid of 256-thread blocks
__device__ __forceinline__ void adam_tail(const AdamTail& tail) {
#pragma clang fp contract(off)
    if (tail.losses8 && blockIdx.x == 0 && threadIdx.x == 0) {
        float t = 0.f;
        for (int i = 0; i < 7; ++i) t = t + tail.losses8[i];        // Python sum(): 0 + l0 + l1 + ... (SumLoss, :208)
        tail.losses8[7] = t;
        if (tail.losses_copy) {
            for (int i = 0; i < 7; ++i) tail.losses_copy[i] = tail.losses8[i];
            tail.losses_copy[7] = t;
        }
    }
    if (tail.zero)
        for (long long i = blockIdx.x * 256ll + threadIdx.x; i < tail.zero_count; i += (long long)gridDim.x * 256) tail.zero[i] = 0u;
}
#endif

}  // namespace st
