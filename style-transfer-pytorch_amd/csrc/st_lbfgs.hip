// optimizer='lbfgs' as a native step: torch.optim.LBFGS(max_iter=1, history_size=10, lr=1, tolerance_grad=1e-7,
// tolerance_change=1e-9, line_search_fn=None).step (torch/optim/lbfgs.py, `step`; the reference configures it at
// style_transfer.py:464-465) + EMA.update (:250-253), in the VECTOR-FREE form: with the basis
//     b = [s_0 .. s_{m-1}, y_0 .. y_{m-1}, g]                      (m <= 10 curvature pairs, oldest first)
// every inner product of the two-loop recursion is an entry of B = b b^T, the recursion runs on a coefficient vector
// delta of length 2m + 1 in double, and the direction is d = sum_j delta_j b_j.  Three launches per iteration:
//   1. lbfgs_dots_kernel   one pass over the basis: y = g - g_prev into the candidate slot and the three NEW rows of B
//                          (candidate s, candidate y, g against every basis vector) + |g|_1 + |g|_inf.  Per-workgroup
//                          partial sums; the workgroup that draws the last ticket adds them in index order in double
//                          (run-to-run bit-identical, no floating-point atomics) into ONE contiguous block
//                          (LbfgsCtl::rows) - or, when the parameter is cut into row strips, into this rank's RECORD of a
//                          gather area (72 doubles per rank: the same 70 sums, |g|_inf, padding).
//      [strips only]       one all-gather of the ranks' records: the only thing that crosses the fabric (kind 6 of
//                          st_exchange: the transport copies, it forms no sum).
//   2. lbfgs_solve_kernel  one wave, plain C++ in double: [strips: first the `world` records added in rank order, |g|_inf
//                          their maximum - every rank adds the same numbers in the same order, so delta, t and the exit are
//                          bit-identical on all of them whatever algorithm the transport uses;] the three exits of LBFGS.step as device flags, acceptance of the
//                          candidate pair (y.s > 1e-10) and the rotation of the ring, the recursion on delta, t.
//   3. lbfgs_move_kernel   one pass: d = sum_j delta_j b_j, the next candidate s = t d, g_prev = g, image += s unless a
//                          flag forbids it, and the EMA update of the same pixels.
// No decision is taken on the host, so the step never waits for the device.  State is ONE caller-owned device buffer
// (st_lbfgs_state_bytes): [LbfgsCtl | per-workgroup partials | 11 s slots | 11 y slots | g_prev]; all zero = a fresh state.
// The candidate pair lives in the ring's spare slot, so a rejected pair overwrites nothing.  A strip's state
// (st_qn_strip_state_bytes) is that layout for the rank's own elements with the gather area behind it.
#include <cstddef>
#include <cstdint>

#include "st_plan.h"

namespace st {

int fabric_apply(st_fabric* f, const st_exchange& ex, hipStream_t fallback);      // st_fabric.hip
int fabric_position(const st_fabric* f, int* rank, int* world);

namespace {

constexpr int kHist = 10;                    // history_size (style_transfer.py:465)
constexpr int kSlots = kHist + 1;            // + the candidate's spare slot
constexpr int kRowW = 2 * kHist + 3;         // columns of a new row of B: s_0..s_9, y_0..y_9, candidate s, candidate y, g
constexpr int kCols = 6 * kHist + 8;         // distinct sums of a pass (the three rows without their symmetric doubles, |g|_1, |g|_inf)
constexpr int kMaxBlocks = 1024;
constexpr double kTolGrad = 1e-7, kTolChange = 1e-9, kMinCurvature = 1e-10;      // lbfgs.py defaults / `if ys > 1e-10`

// columns of a workgroup's partial sums
constexpr int cSS = 2 * kHist, cSY = cSS + 1, cSG = cSS + 2;                 // candidate s . {s_i, y_i | s, y, g}
constexpr int cY0 = cSG + 1, cYY = cY0 + 2 * kHist, cYG = cYY + 1;           // candidate y . {s_i, y_i | y, g}
constexpr int cG0 = cYG + 1, cGG = cG0 + 2 * kHist, cL1 = cGG + 1, cLinf = cL1 + 1;      // g . {s_i, y_i | g}, |g|_1, |g|_inf
static_assert(cLinf + 1 == kCols, "column map");

struct LbfgsCtl {
    int n_iter;               // state['n_iter'] of LBFGS.step
    int hist_len;             // m = len(old_dirs)
    int exit_code;            // of the last step: 0 moved, 1 |g|_inf <= tolerance_grad, 2 g.d > -tolerance_change
    int accepted;             // the last step's candidate pair entered the history
    int ring[kSlots + 1];     // ring[i], i < m: slot of pair i (oldest first); ring[m]: the candidate's slot
    unsigned int ticket;      // zero between launches
    float t;                  // step length as the move applies it
    float coef[2 * kHist + 1];        // delta as fp32: s_0..s_{m-1} at [0, m), y at [kHist, kHist + m), g at [2 kHist]
    double t_d, gtd, h_diag, ys;
    // the three new rows of B and |g|_1: sums over the elements (a strip's record holds exactly this block) ...
    double rows[3 * kRowW + 1];
    double linf;              // ... and the one maximum (on strips: what the solve kernel leaves after adding the records)
    double bss[kHist][kHist], bsy[kHist][kHist], byy[kHist][kHist];      // s_i.s_j, s_i.y_j, y_i.y_j of the history
};
constexpr size_t kCtlBytes = 4096;
static_assert(sizeof(LbfgsCtl) <= kCtlBytes && sizeof(LbfgsCtl) % 4 == 0, "control block");
static_assert(offsetof(LbfgsCtl, rows) == 192 && offsetof(LbfgsCtl, linf) == 192 + 70 * 8, "include/st_amd.h documents where the new rows lie");
constexpr size_t kPartialBytes = (size_t)kMaxBlocks * kCols * sizeof(float);
constexpr int kRecord = 72;                  // doubles per rank in the gather area: rows[70], |g|_inf, one of padding (16-byte multiple)
constexpr int kRecordSums = 3 * kRowW + 1;
constexpr int kMaxWorld = 8;
static_assert(kRecordSums + 1 <= kRecord && (kRecord * sizeof(double)) % 16 == 0, "record layout");

struct LbfgsState {
    LbfgsCtl* ctl;
    float* partials;
    float* slots;          // [2 * kSlots + 1][stride]: s slots, y slots, g_prev
    long long stride;      // elements per slot (count rounded up to 4: every slot 16-byte aligned)
};
__host__ __device__ inline long long slot_stride(long long count) { return (count + 3) & ~3ll; }
LbfgsState carve(void* state, long long count) {
    char* base = static_cast<char*>(state);
    return LbfgsState{reinterpret_cast<LbfgsCtl*>(base), reinterpret_cast<float*>(base + kCtlBytes),
                      reinterpret_cast<float*>(base + kCtlBytes + kPartialBytes), slot_stride(count)};
}

template <int V> struct Vec;
template <> struct Vec<4> { typedef f32x4 type; };
template <> struct Vec<1> { typedef float type; };
template <int V> __device__ __forceinline__ float lane(const typename Vec<V>::type& v, int k) { return v[k]; }
template <> __device__ __forceinline__ float lane<1>(const float& v, int) { return v; }
template <int V> __device__ __forceinline__ void set_lane(typename Vec<V>::type& v, int k, float x) { v[k] = x; }
template <> __device__ __forceinline__ void set_lane<1>(float& v, int, float x) { v = x; }

__device__ __forceinline__ float wave_sum64(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float wave_max64(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// ---- launch 1 -----------------------------------------------------------------------------------------------------
// One tile of V elements per thread and trip; MH = the history length (a template parameter so that the 6 MH + 8 running
// sums are registers: the kernel dispatches on the device's own counter).
template <int V, int MH>
__device__ __forceinline__ void dots_body(const float* __restrict__ g, const LbfgsState st, const int* ring, bool first,
                                          long long nv, float* __restrict__ block_out, float (*lds)[kCols]) {
    typedef typename Vec<V>::type vec;
    const vec* g_v = reinterpret_cast<const vec*>(g);
    const vec* gp_v = reinterpret_cast<const vec*>(st.slots + 2ll * kSlots * st.stride);
    const int cand = ring[MH];
    const vec* sc_v = reinterpret_cast<const vec*>(st.slots + (long long)cand * st.stride);
    vec* yc_v = reinterpret_cast<vec*>(st.slots + (long long)(kSlots + cand) * st.stride);
    const vec* s_v[MH > 0 ? MH : 1];
    const vec* y_v[MH > 0 ? MH : 1];
#pragma unroll
    for (int i = 0; i < MH; ++i) {
        s_v[i] = reinterpret_cast<const vec*>(st.slots + (long long)ring[i] * st.stride);
        y_v[i] = reinterpret_cast<const vec*>(st.slots + (long long)(kSlots + ring[i]) * st.stride);
    }
    float a_s[2 * (MH > 0 ? MH : 1)], a_y[2 * (MH > 0 ? MH : 1)], a_g[2 * (MH > 0 ? MH : 1)];
#pragma unroll
    for (int i = 0; i < 2 * MH; ++i) a_s[i] = a_y[i] = a_g[i] = 0.f;
    float ss = 0.f, sy = 0.f, sg = 0.f, yy = 0.f, yg = 0.f, gg = 0.f, l1 = 0.f, linf = 0.f;
    // every running sum is pinned to a register of its own after each update (an empty asm statement, as in
    // tv_interior_kernel): the SLP vectoriser would otherwise pair sums that share a factor into packed-FP32 operations
    // with a cross-half op_sel, which build.py's hazard guard refuses
    auto acc = [](float& sum, float a, float b) __attribute__((always_inline)) {
        sum = fmaf(a, b, sum);
        asm("" : "+v"(sum));
    };
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
        const vec gv = g_v[i];
        vec sc, yc;
        if (first) {              // nothing before this gradient: no candidate pair (uniform branch)
#pragma unroll
            for (int k = 0; k < V; ++k) { set_lane<V>(sc, k, 0.f); set_lane<V>(yc, k, 0.f); }
        } else {
            const vec gp = gp_v[i];
            sc = sc_v[i];
#pragma unroll
            for (int k = 0; k < V; ++k) set_lane<V>(yc, k, lane<V>(gv, k) - lane<V>(gp, k));      // y = flat_grad.sub(prev_flat_grad)
            yc_v[i] = yc;
        }
        vec sv[MH > 0 ? MH : 1], yv[MH > 0 ? MH : 1];
#pragma unroll
        for (int j = 0; j < MH; ++j) { sv[j] = s_v[j][i]; yv[j] = y_v[j][i]; }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float gk = lane<V>(gv, k), sk = lane<V>(sc, k), yk = lane<V>(yc, k);
#pragma unroll
            for (int j = 0; j < MH; ++j) {
                const float sj = lane<V>(sv[j], k), yj = lane<V>(yv[j], k);
                acc(a_s[j], sk, sj); acc(a_s[MH + j], sk, yj);
                acc(a_y[j], yk, sj); acc(a_y[MH + j], yk, yj);
                acc(a_g[j], gk, sj); acc(a_g[MH + j], gk, yj);
            }
            acc(ss, sk, sk); acc(sy, sk, yk); acc(sg, sk, gk);
            acc(yy, yk, yk); acc(yg, yk, gk); acc(gg, gk, gk);
            l1 += fabsf(gk);
            linf = fmaxf(linf, fabsf(gk));
        }
    }
    // workgroup sums: lanes by shuffles, the four waves in wave order
    const int wave = threadIdx.x >> 6, ln = threadIdx.x & 63;
    auto put = [&](int col, float v) __attribute__((always_inline)) {
        v = wave_sum64(v);
        if (ln == 0) lds[wave][col] = v;
    };
#pragma unroll
    for (int j = 0; j < MH; ++j) {
        put(j, a_s[j]); put(kHist + j, a_s[MH + j]);
        put(cY0 + j, a_y[j]); put(cY0 + kHist + j, a_y[MH + j]);
        put(cG0 + j, a_g[j]); put(cG0 + kHist + j, a_g[MH + j]);
    }
    if (ln == 0)              // pairs the history does not hold yet
        for (int j = MH; j < kHist; ++j)
            for (int base : {0, cY0, cG0}) lds[wave][base + j] = lds[wave][base + kHist + j] = 0.f;
    put(cSS, ss); put(cSY, sy); put(cSG, sg); put(cYY, yy); put(cYG, yg); put(cGG, gg); put(cL1, l1);
    linf = wave_max64(linf);
    if (ln == 0) lds[wave][cLinf] = linf;
    __syncthreads();
    if (threadIdx.x < kCols) {
        const int c = threadIdx.x;
        block_out[c] = c == cLinf ? fmaxf(fmaxf(lds[0][c], lds[1][c]), fmaxf(lds[2][c], lds[3][c]))
                                  : ((lds[0][c] + lds[1][c]) + lds[2][c]) + lds[3][c];
    }
}

// record: null = the whole parameter is here, the sums go to LbfgsCtl::rows / linf; else this rank's slot of the gather area
template <int V>
__global__ __launch_bounds__(256) void lbfgs_dots_kernel(const float* __restrict__ g, LbfgsState st, long long nv,
                                                         AdamTail tail, double* __restrict__ record) {
    __shared__ float lds[4][kCols];
    __shared__ double part[3][kCols];
    __shared__ bool is_last;
    adam_tail(tail);        // st_plan_lbfgs_step: the closure's loss total and the clearing of its operand bounds ride here
    const int m = st.ctl->hist_len;
    const bool first = st.ctl->n_iter == 0;
    const int* ring = st.ctl->ring;
    float* out = st.partials + (size_t)blockIdx.x * kCols;
    switch (first ? 0 : m) {
#define ST_CASE(MH) case MH: dots_body<V, MH>(g, st, ring, first, nv, out, lds); break;
        ST_CASE(0) ST_CASE(1) ST_CASE(2) ST_CASE(3) ST_CASE(4) ST_CASE(5) ST_CASE(6) ST_CASE(7) ST_CASE(8) ST_CASE(9)
        default: dots_body<V, kHist>(g, st, ring, first, nv, out, lds); break;
#undef ST_CASE
    }
    // the workgroup that draws the last ticket adds all partials in index order (release / acquire at agent scope as in
    // st_pointwise.hip's LastBlock)
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int prev = atomicAdd(&st.ctl->ticket, 1u);
        is_last = prev == gridDim.x - 1;
        if (is_last) st.ctl->ticket = 0u;
    }
    __syncthreads();
    if (!is_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const int blocks = gridDim.x;
    if (threadIdx.x < 3 * kCols) {        // three runs of consecutive workgroups per column, then the runs in order
        const int c = threadIdx.x % kCols, r = threadIdx.x / kCols;
        const int per = (blocks + 2) / 3;
        const int b0 = r * per, b1 = min(blocks, b0 + per);
        const float* p = st.partials + c;
        double acc = 0.0;
        if (c == cLinf) for (int b = b0; b < b1; ++b) acc = fmax(acc, (double)p[(size_t)b * kCols]);
        else for (int b = b0; b < b1; ++b) acc += (double)p[(size_t)b * kCols];
        part[r][c] = acc;
    }
    __syncthreads();
    if (threadIdx.x < kCols) {
        const int c = threadIdx.x;
        const double v = c == cLinf ? fmax(fmax(part[0][c], part[1][c]), part[2][c]) : (part[0][c] + part[1][c]) + part[2][c];
        part[0][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < 3 * kRowW) {        // the rows with their symmetric entries filled in
        const int r = threadIdx.x / kRowW, c = threadIdx.x % kRowW;
        int col;
        if (r == 0) col = c;                                                                     // candidate s . everything
        else if (r == 1) col = c < 2 * kHist ? cY0 + c : c == 2 * kHist ? cSY : c == 2 * kHist + 1 ? cYY : cYG;
        else col = c < 2 * kHist ? cG0 + c : c == 2 * kHist ? cSG : c == 2 * kHist + 1 ? cYG : cGG;
        (record ? record : st.ctl->rows)[threadIdx.x] = part[0][col];
    }
    if (threadIdx.x == 0) {
        if (record) {
            record[kRecordSums - 1] = part[0][cL1];
            record[kRecordSums] = part[0][cLinf];
            record[kRecordSums + 1] = 0.0;
        } else {
            st.ctl->rows[3 * kRowW] = part[0][cL1];
            st.ctl->linf = part[0][cLinf];
        }
    }
}

// ---- launch 2 -----------------------------------------------------------------------------------------------------
// LBFGS.step's scalar work (statement for statement as sharding.StripLBFGS.step restates it), every inner product read from B.
// gather: null, or `world` records (strips): added in rank order into rows / linf before anything reads them.
__global__ __launch_bounds__(64) void lbfgs_solve_kernel(LbfgsCtl* ctl, const double* __restrict__ gather, int world) {
    __shared__ LbfgsCtl c;
    __shared__ double gs[kHist], gy[kHist], al[kHist], delta[2 * kHist + 1];      // (indexed at run time: not registers)
    constexpr int words = sizeof(LbfgsCtl) / 4;
    for (int i = threadIdx.x; i < words; i += 64) reinterpret_cast<unsigned int*>(&c)[i] = reinterpret_cast<const unsigned int*>(ctl)[i];
    __syncthreads();
    if (gather) {
        for (int i = threadIdx.x; i <= kRecordSums; i += 64) {
            double v = gather[i];
            if (i < kRecordSums) {
                for (int r = 1; r < world; ++r) v += gather[r * kRecord + i];
                c.rows[i] = v;
            } else {
                for (int r = 1; r < world; ++r) v = fmax(v, gather[r * kRecord + i]);
                c.linf = v;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double* rs = c.rows;                 // candidate s . [s_i | y_i | s, y, g]
        const double* ry = c.rows + kRowW;         // candidate y . ...
        const double* rg = c.rows + 2 * kRowW;     // g . ...
        const double l1 = c.rows[3 * kRowW];
        c.accepted = 0;
        if (c.linf <= (double)(float)kTolGrad) {            // if flat_grad.abs().max() <= tolerance_grad: return orig_loss
            c.exit_code = 1;
        } else {
            c.n_iter += 1;
            int m = c.hist_len;
            for (int i = 0; i < kHist; ++i) { gs[i] = rg[i]; gy[i] = rg[kHist + i]; }
            const double gg = rg[2 * kHist + 2];
            if (c.n_iter == 1) {                            // d = flat_grad.neg(); old_dirs = old_stps = ro = []; H_diag = 1
                m = 0;
                c.h_diag = 1.0;
                for (int i = 0; i <= kSlots; ++i) c.ring[i] = i < kSlots ? i : 0;
            } else {
                const double ys = rs[2 * kHist + 1];        // ys = y.dot(s)
                c.ys = ys;
                if (ys > kMinCurvature) {
                    c.accepted = 1;
                    int shift = 0;
                    if (m == kHist) {                       // old_dirs.pop(0) ...: the oldest pair's slot becomes the spare one
                        shift = 1;
                        const int oldest = c.ring[0];
                        for (int i = 0; i < kHist; ++i) c.ring[i] = c.ring[i + 1];
                        c.ring[kHist] = oldest;
                        for (int i = 0; i + 1 < kHist; ++i)
                            for (int j = 0; j + 1 < kHist; ++j) {
                                c.bss[i][j] = c.bss[i + 1][j + 1];
                                c.bsy[i][j] = c.bsy[i + 1][j + 1];
                                c.byy[i][j] = c.byy[i + 1][j + 1];
                            }
                        for (int i = 0; i + 1 < kHist; ++i) { gs[i] = gs[i + 1]; gy[i] = gy[i + 1]; }
                        m = kHist - 1;
                    }
                    const int k = m;                        // ... .append(y), .append(s): the candidate is pair k
                    for (int j = 0; j < k; ++j) {
                        const int jo = j + shift;           // the pair's index when the rows were formed
                        c.bss[k][j] = c.bss[j][k] = rs[jo];
                        c.bsy[k][j] = rs[kHist + jo];       // s_k . y_j
                        c.bsy[j][k] = ry[jo];               // s_j . y_k
                        c.byy[k][j] = c.byy[j][k] = ry[kHist + jo];
                    }
                    c.bss[k][k] = rs[2 * kHist];
                    c.bsy[k][k] = ys;
                    c.byy[k][k] = ry[2 * kHist + 1];
                    gs[k] = rg[2 * kHist];
                    gy[k] = rg[2 * kHist + 1];
                    m = k + 1;
                    c.h_diag = ys / c.byy[k][k];            // H_diag = ys / y.dot(y)
                }
            }
            // the two-loop recursion on delta: q = -g
            for (int i = 0; i < 2 * kHist + 1; ++i) delta[i] = 0.0;
            delta[2 * kHist] = -1.0;
            for (int i = m - 1; i >= 0; --i) {              // al[i] = old_stps[i].dot(q) * ro[i]; q.add_(old_dirs[i], alpha=-al[i])
                double dot = delta[2 * kHist] * gs[i];
                for (int j = 0; j < m; ++j) dot += delta[j] * c.bss[i][j] + delta[kHist + j] * c.bsy[i][j];
                al[i] = dot / c.bsy[i][i];
                delta[kHist + i] -= al[i];
            }
            for (int i = 0; i < 2 * kHist + 1; ++i) delta[i] *= c.h_diag;       // d = r = q * H_diag
            for (int i = 0; i < m; ++i) {                   // be_i = old_dirs[i].dot(r) * ro[i]; r.add_(old_stps[i], alpha=al[i] - be_i)
                double dot = delta[2 * kHist] * gy[i];
                for (int j = 0; j < m; ++j) dot += delta[j] * c.bsy[j][i] + delta[kHist + j] * c.byy[i][j];
                delta[i] += al[i] - dot / c.bsy[i][i];
            }
            double gtd = delta[2 * kHist] * gg;             // gtd = flat_grad.dot(d)
            for (int j = 0; j < m; ++j) gtd += delta[j] * gs[j] + delta[kHist + j] * gy[j];
            // t = min(1., 1. / flat_grad.abs().sum()) * lr on the first iteration (an fp32 quotient in torch), lr afterwards
            const float t = c.n_iter == 1 ? fminf(1.f, 1.f / (float)l1) : 1.f;
            c.hist_len = m;
            c.t = t;
            c.t_d = (double)t;
            c.gtd = gtd;
            for (int i = 0; i < 2 * kHist + 1; ++i) c.coef[i] = (float)delta[i];
            c.exit_code = gtd > -kTolChange ? 2 : 0;        // if gtd > -tolerance_change: break (d, t, prev_flat_grad are kept)
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < words; i += 64) reinterpret_cast<unsigned int*>(ctl)[i] = reinterpret_cast<const unsigned int*>(&c)[i];
}

// ---- launch 3 -----------------------------------------------------------------------------------------------------
template <int V, int MH>
__device__ __forceinline__ void move_body(float* __restrict__ image, const float* __restrict__ g, float* __restrict__ ema,
                                          const LbfgsState st, const LbfgsCtl* ctl, long long nv, float decay, float one_m_decay) {
#pragma clang fp contract(off)
    typedef typename Vec<V>::type vec;
    const int* ring = ctl->ring;
    const bool moves = ctl->exit_code == 0;
    const float t = ctl->t, cg = ctl->coef[2 * kHist];
    const vec* g_v = reinterpret_cast<const vec*>(g);
    vec* x_v = reinterpret_cast<vec*>(image);
    vec* e_v = reinterpret_cast<vec*>(ema);
    vec* gp_v = reinterpret_cast<vec*>(st.slots + 2ll * kSlots * st.stride);
    vec* sc_v = reinterpret_cast<vec*>(st.slots + (long long)ring[MH] * st.stride);
    const vec* s_v[MH > 0 ? MH : 1];
    const vec* y_v[MH > 0 ? MH : 1];
    float cs[MH > 0 ? MH : 1], cy[MH > 0 ? MH : 1];
#pragma unroll
    for (int i = 0; i < MH; ++i) {
        s_v[i] = reinterpret_cast<const vec*>(st.slots + (long long)ring[i] * st.stride);
        y_v[i] = reinterpret_cast<const vec*>(st.slots + (long long)(kSlots + ring[i]) * st.stride);
        cs[i] = ctl->coef[i];
        cy[i] = ctl->coef[kHist + i];
    }
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
        const vec gv = g_v[i];
        vec x = x_v[i];
        vec sv[MH > 0 ? MH : 1], yv[MH > 0 ? MH : 1];
#pragma unroll
        for (int j = 0; j < MH; ++j) { sv[j] = s_v[j][i]; yv[j] = y_v[j][i]; }
        vec s;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            float d = cg * lane<V>(gv, k);
#pragma unroll
            for (int j = 0; j < MH; ++j) d = fmaf(cy[j], lane<V>(yv[j], k), fmaf(cs[j], lane<V>(sv[j], k), d));
            const float sk = t * d;                                           // s = d.mul(t) of the next step
            set_lane<V>(s, k, sk);
            if (moves) set_lane<V>(x, k, lane<V>(x, k) + sk);                 // p.add_(d, alpha=t); no clamp (reference :482-483)
        }
        sc_v[i] = s;
        gp_v[i] = gv;                                                         // prev_flat_grad.copy_(flat_grad)
        if (moves) x_v[i] = x;
        if (ema) {
            vec e = e_v[i];
#pragma unroll
            for (int k = 0; k < V; ++k) {
                float ek = lane<V>(e, k) * decay;                             // self.value *= self.decay
                ek = ek + one_m_decay * lane<V>(x, k);                        // self.value += (1 - self.decay) * input
                set_lane<V>(e, k, ek);
            }
            e_v[i] = e;
        }
    }
}

template <int V>
__global__ __launch_bounds__(256) void lbfgs_move_kernel(float* __restrict__ image, const float* __restrict__ g,
                                                         float* __restrict__ ema, LbfgsState st, long long nv, float decay,
                                                         float one_m_decay) {
#pragma clang fp contract(off)
    typedef typename Vec<V>::type vec;
    const LbfgsCtl* ctl = st.ctl;
    if (ctl->exit_code == 1) {          // the gradient exit: nothing of the optimiser's state moves; EMA.update still runs
        if (!ema) return;
        const vec* x_v = reinterpret_cast<const vec*>(image);
        vec* e_v = reinterpret_cast<vec*>(ema);
        for (long long i = blockIdx.x * 256ll + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
            const vec x = x_v[i];
            vec e = e_v[i];
#pragma unroll
            for (int k = 0; k < V; ++k) {
                float ek = lane<V>(e, k) * decay;
                ek = ek + one_m_decay * lane<V>(x, k);
                set_lane<V>(e, k, ek);
            }
            e_v[i] = e;
        }
        return;
    }
    switch (ctl->hist_len) {
#define ST_CASE(MH) case MH: move_body<V, MH>(image, g, ema, st, ctl, nv, decay, one_m_decay); break;
        ST_CASE(0) ST_CASE(1) ST_CASE(2) ST_CASE(3) ST_CASE(4) ST_CASE(5) ST_CASE(6) ST_CASE(7) ST_CASE(8) ST_CASE(9)
        default: move_body<V, kHist>(image, g, ema, st, ctl, nv, decay, one_m_decay); break;
#undef ST_CASE
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// 16-byte accesses when the element count and every pointer of the launch allow them, else the scalar kernels
int launch_dots(void* state, long long count, const float* grad, bool vec, hipStream_t s, AdamTail tail, double* record) {
    const LbfgsState st = carve(state, count);
    const long long nv = vec ? count >> 2 : count;
    const int grid = (int)std::min<long long>((nv + 255) / 256, kMaxBlocks);
    if (tail.losses_copy == tail.losses8) tail.losses_copy = nullptr;
    if (vec) hipLaunchKernelGGL(lbfgs_dots_kernel<4>, dim3(grid), dim3(256), 0, s, grad, st, nv, tail, record);
    else hipLaunchKernelGGL(lbfgs_dots_kernel<1>, dim3(grid), dim3(256), 0, s, grad, st, nv, tail, record);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_solve_move(void* state, long long count, float* image, const float* grad, float* ema, double ema_decay, bool vec,
                      hipStream_t s, const double* gather, int world) {
    const LbfgsState st = carve(state, count);
    const long long nv = vec ? count >> 2 : count;
    const int grid = (int)std::min<long long>((nv + 255) / 256, kMaxBlocks);
    const float decay = (float)ema_decay;                 // torch.tensor(decay): fp32 buffer (style_transfer.py:243)
    const float one_m_decay = 1.0f - decay;               // (1 - self.decay) evaluated in fp32 (:253)
    hipLaunchKernelGGL(lbfgs_solve_kernel, dim3(1), dim3(64), 0, s, st.ctl, gather, world);
    ST_LAUNCH_CHECK();
    if (vec) hipLaunchKernelGGL(lbfgs_move_kernel<4>, dim3(grid), dim3(256), 0, s, image, grad, ema, st, nv, decay, one_m_decay);
    else hipLaunchKernelGGL(lbfgs_move_kernel<1>, dim3(grid), dim3(256), 0, s, image, grad, ema, st, nv, decay, one_m_decay);
    ST_LAUNCH_CHECK();
    return 0;
}

int launch_lbfgs_update(void* state, long long count, float* image, const float* grad, float* ema, double ema_decay,
                        hipStream_t s, AdamTail tail) {
    const bool vec = (count & 3) == 0 && aligned16(state) && aligned16(image) && aligned16(grad) && (!ema || aligned16(ema));
    if (launch_dots(state, count, grad, vec, s, tail, nullptr)) return 1;
    return launch_solve_move(state, count, image, grad, ema, ema_decay, vec, s, nullptr, 1);
}

long long base_state_bytes(long long count) {
    return (long long)(kCtlBytes + kPartialBytes) + (2ll * kSlots + 1) * slot_stride(count) * (long long)sizeof(float);
}
// the gather area of a strip's state: `world` records behind the unsharded layout (a 16-byte multiple)
double* gather_area(void* state, long long count) {
    return reinterpret_cast<double*>(static_cast<char*>(state) + base_state_bytes(count));
}

}  // namespace
}  // namespace st

using namespace st;

extern "C" {

long long st_lbfgs_state_bytes(long long count) {
    if (count < 1) return 0;
    return base_state_bytes(count);
}

int st_lbfgs_reset(void* state, long long count, void* stream) {
    ST_REQUIRE(state && count >= 1, "st_lbfgs_reset: bad argument");
    ST_REQUIRE((reinterpret_cast<uintptr_t>(state) & 15) == 0, "st_lbfgs_reset: the state buffer must be 16-byte aligned");
    ST_HIP(hipMemsetAsync(state, 0, kCtlBytes, static_cast<hipStream_t>(stream)));
    return 0;
}

int st_lbfgs_update(void* state, long long count, float* image, const float* grad, float* ema_value, double ema_decay,
                    void* stream) {
    ST_REQUIRE(state && image && grad && count >= 1, "st_lbfgs_update: bad argument");
    ST_REQUIRE((reinterpret_cast<uintptr_t>(state) & 15) == 0, "st_lbfgs_update: the state buffer must be 16-byte aligned");
    return launch_lbfgs_update(state, count, image, grad, ema_value, ema_decay, static_cast<hipStream_t>(stream), AdamTail{});
}

int st_lbfgs_info(const void* state, long long count, int* n_iter, int* history, int* exit_code, int* accepted, double* t,
                  double* gtd, void* stream) {
    ST_REQUIRE(state && count >= 1, "st_lbfgs_info: bad argument");
    LbfgsCtl host;
    ST_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    ST_HIP(hipMemcpy(&host, state, sizeof(host), hipMemcpyDeviceToHost));
    if (n_iter) *n_iter = host.n_iter;
    if (history) *history = host.hist_len;
    if (exit_code) *exit_code = host.exit_code;
    if (accepted) *accepted = host.accepted;
    if (t) *t = host.t_d;
    if (gtd) *gtd = host.gtd;
    return 0;
}

int st_plan_lbfgs_step(st_plan* p, float* image, void* state, float* ema_value, double ema_decay, float* losses_out,
                       void* stream) {
    ST_REQUIRE(p && image && state && ema_value, "st_plan_lbfgs_step: null argument");
    ST_REQUIRE((reinterpret_cast<uintptr_t>(state) & 15) == 0, "st_plan_lbfgs_step: the state buffer must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (ensure_grad_alloc(p) || ensure_streams(p, s)) return 1;
    // as in st_plan_step: the total of the loss terms and the clearing of the fp16x3 operand bounds for the next pass ride in
    // the first kernel behind the closure instead of two launches of their own (not under graph replay, whose captured
    // closure ends with the sum)
    AdamTail tail{};
    const bool ride = !p->graph_enabled;
    if (ride) {
        tail.losses8 = p->losses;
        tail.losses_copy = losses_out;
        if (p->net->conv_elem == 1) { tail.zero = reinterpret_cast<unsigned int*>(p->amax_word); tail.zero_count = 64ll * kAmaxWordUints; }
    }
    p->defer_sum = ride;
    const int closure_rc = closure_entry(p, image, p->grad_img, losses_out, s);
    p->defer_sum = false;
    if (closure_rc) return 1;
    const int rc = launch_lbfgs_update(state, 3ll * p->H * p->W, image, p->grad_img, ema_value, ema_decay, s, tail);
    p->amax_clean = rc == 0 && tail.zero != nullptr;
    return rc;
}

// ---- the same step on a row strip of the parameter (the entry points are named st_qn_*: quasi-Newton) -------------------
long long st_qn_strip_state_bytes(long long count, int world) {
    if (count < 1 || world < 1 || world > kMaxWorld) return 0;
    return base_state_bytes(count) + (long long)world * kRecord * (long long)sizeof(double);
}

int st_qn_strip_dots(void* state, long long count, int rank, int world, const float* grad, st_exchange* gather, void* stream) {
    ST_REQUIRE(state && grad && gather && count >= 1, "st_qn_strip_dots: bad argument");
    ST_REQUIRE(world >= 1 && world <= kMaxWorld && rank >= 0 && rank < world, "st_qn_strip_dots: rank %d of %d", rank, world);
    ST_REQUIRE((reinterpret_cast<uintptr_t>(state) & 15) == 0, "st_qn_strip_dots: the state buffer must be 16-byte aligned");
    double* area = gather_area(state, count);
    const bool vec = (count & 3) == 0 && aligned16(grad);
    if (launch_dots(state, count, grad, vec, static_cast<hipStream_t>(stream), AdamTail{}, area + (size_t)rank * kRecord)) return 1;
    *gather = st_exchange{};
    gather->kind = 6;
    gather->count = kRecord * (long long)(sizeof(double) / sizeof(float));
    gather->buffer = reinterpret_cast<float*>(area);
    gather->stream = stream;
    return 0;
}

int st_qn_strip_apply(void* state, long long count, int world, float* image, const float* grad, float* ema_value,
                      double ema_decay, void* stream) {
    ST_REQUIRE(state && image && grad && count >= 1, "st_qn_strip_apply: bad argument");
    ST_REQUIRE(world >= 1 && world <= kMaxWorld, "st_qn_strip_apply: world %d", world);
    ST_REQUIRE((reinterpret_cast<uintptr_t>(state) & 15) == 0, "st_qn_strip_apply: the state buffer must be 16-byte aligned");
    const bool vec = (count & 3) == 0 && aligned16(image) && aligned16(grad) && (!ema_value || aligned16(ema_value));
    return launch_solve_move(state, count, image, grad, ema_value, ema_decay, vec, static_cast<hipStream_t>(stream),
                             gather_area(state, count), world);
}

int st_plan_qn_strip_step(st_plan* p, st_fabric* fabric, float* image, float* grad, void* state, float* ema_value,
                          double ema_decay, void* stream) {
    ST_REQUIRE(p && fabric && image && grad && state, "st_plan_qn_strip_step: null argument");
    ST_REQUIRE(p->strip, "st_plan_qn_strip_step: not a strip plan (st_plan_lbfgs_step is the unsharded form)");
    int rank = 0, world = 1;
    if (fabric_position(fabric, &rank, &world)) return 1;
    ST_REQUIRE(rank == p->rank && world == p->world, "st_plan_qn_strip_step: the plan is rank %d of %d, the fabric rank %d of %d",
               p->rank, p->world, rank, world);
    const long long count = 3ll * p->H * p->W;
    if (st_plan_closure_begin(p, image, grad) || st_plan_closure_run(p, fabric, stream)) return 1;
    st_exchange gather;
    if (st_qn_strip_dots(state, count, rank, world, grad, &gather, stream)) return 1;
    if (fabric_apply(fabric, gather, static_cast<hipStream_t>(stream))) return 1;
    return st_qn_strip_apply(state, count, world, image, grad, ema_value, ema_decay, stream);
}

}  // extern "C"
