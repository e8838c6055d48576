// In-library transport of the strip-sharded closure: the exchanges of the phase machine issued as RCCL operations from C++,
// on the streams the descriptors name (round 4).
//
// Why it exists.  Rounds 2 / 3 left the exchanges to the Python caller (torch.distributed on an ExternalStream over the
// library's streams).  Run over the real transport on one GPU (a middle strip whose neighbours are rank 0 itself,
// tools/fabric_host_time.py, rocprofv3 trace) that form showed two things no emulation could: (1) c10d launches the RCCL
// kernels on an INTERNAL stream of its own, whatever stream is current, and ROCm had put that stream on the trunk's hardware
// queue - every point-to-point kernel and every barrier packet waiting for a head's Gram kernel sat in front of the trunk's
// next launch, so no exchange overlapped anything (+1.5 ms per iteration on a 2896 x 272 strip); (2) ~100 us of host time per
// exchange (5 ms of enqueue per iteration against 6.5 ms of GPU work).  Here the library owns two communicators (trunk halos,
// heads' collectives: operations of one communicator execute in issue order) and issues ncclSend / ncclRecv / ncclAllReduce /
// ncclReduce / ncclBroadcast / ncclAllGather itself: the kernels run on the probed communication / head streams, and st_plan_closure_run
// walks through the whole phase sequence in one call.
//
// RCCL is resolved with dlopen at first use (librccl.so.1, the copy the process has already loaded if there is one):
// libst_amd.so itself has no link dependency on it, and the unsharded path never touches it.
#include <dlfcn.h>

#include <chrono>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "st_common.h"
#include "../../include/st_amd.h"

namespace st {
namespace {

// the slice of rccl.h this file uses (ABI of RCCL 2.x: ncclUniqueId is 128 opaque bytes passed BY VALUE)
struct NcclId { char internal[128]; };
typedef void* NcclComm;
constexpr int kNcclFloat = 7, kNcclUint32 = 3, kNcclSum = 0;

struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(NcclId*) = nullptr;
    int (*CommInitRank)(NcclComm*, int, NcclId, int) = nullptr;
    int (*CommDestroy)(NcclComm) = nullptr;
    int (*CommAbort)(NcclComm) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void*, size_t, int, int, NcclComm, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, NcclComm, hipStream_t) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, NcclComm, hipStream_t) = nullptr;
    int (*Reduce)(const void*, void*, size_t, int, int, int, NcclComm, hipStream_t) = nullptr;
    int (*Broadcast)(const void*, void*, size_t, int, int, NcclComm, hipStream_t) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, NcclComm, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};

Rccl* rccl() {
    static Rccl r;
    static std::once_flag once;
    static bool ok = false;
    std::call_once(once, [] {
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (r.lib) break;
        }
        if (!r.lib) return;
        auto sym = [&](const char* n) { return dlsym(r.lib, n); };
        r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(sym("ncclGetUniqueId"));
        r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(sym("ncclCommInitRank"));
        r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(sym("ncclCommDestroy"));
        r.CommAbort = reinterpret_cast<decltype(r.CommAbort)>(sym("ncclCommAbort"));
        r.GroupStart = reinterpret_cast<decltype(r.GroupStart)>(sym("ncclGroupStart"));
        r.GroupEnd = reinterpret_cast<decltype(r.GroupEnd)>(sym("ncclGroupEnd"));
        r.Send = reinterpret_cast<decltype(r.Send)>(sym("ncclSend"));
        r.Recv = reinterpret_cast<decltype(r.Recv)>(sym("ncclRecv"));
        r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(sym("ncclAllReduce"));
        r.Reduce = reinterpret_cast<decltype(r.Reduce)>(sym("ncclReduce"));
        r.Broadcast = reinterpret_cast<decltype(r.Broadcast)>(sym("ncclBroadcast"));
        r.AllGather = reinterpret_cast<decltype(r.AllGather)>(sym("ncclAllGather"));
        r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(sym("ncclGetErrorString"));
        ok = r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.GroupStart && r.GroupEnd && r.Send && r.Recv &&
             r.AllReduce && r.Reduce && r.Broadcast && r.AllGather;
    });
    return ok ? &r : nullptr;
}

}  // namespace
}  // namespace st

using namespace st;

struct st_fabric {
    NcclComm comm[2] = {nullptr, nullptr};      // channel 0: the trunk's halos and loss scalars; channel 1: the heads
    int rank = 0, world = 1;
    int self_halo = 0;                          // one rank whose upper AND lower neighbour is itself (tests, measurements)
    bool stuck = false;                         // a self-test timed out: operations may still be in flight, abort not destroy
};

#define ST_NCCL(expr)                                                                                          \
    do {                                                                                                       \
        const int _rc = (expr);                                                                                \
        if (_rc != 0) {                                                                                        \
            Rccl* _r = rccl();                                                                                 \
            st::set_error("%s failed: %s (%s:%d)", #expr, (_r && _r->GetErrorString) ? _r->GetErrorString(_rc) : "?", \
                          __FILE__, __LINE__);                                                                 \
            return 1;                                                                                          \
        }                                                                                                      \
    } while (0)

namespace st {

// one exchange descriptor of the phase machine over the fabric; `fallback` = the stream of descriptors that name none
int fabric_apply(st_fabric* f, const st_exchange& ex, hipStream_t fallback) {
    if (ex.kind == 0 || ex.kind == 3) return 0;
    Rccl* r = rccl();
    ST_REQUIRE(r && f, "fabric: RCCL is not available");
    hipStream_t s = ex.stream ? static_cast<hipStream_t>(ex.stream) : fallback;
    NcclComm comm = f->comm[ex.channel == 1 ? 1 : 0];
    const size_t n = (size_t)ex.count;
    if (ex.kind == 1) {
        ST_NCCL(r->GroupStart());
        // (a failing call inside the group must not leave the group open on this thread: the lambda's early returns all pass
        // through ncclGroupEnd below)
        const int rc = [&]() -> int {
        if (f->self_halo) {
            // sends and receives between one pair of ranks match in issue order: this rank's "up" rows land in the upper
            // neighbour's recv_down (its own), its "down" rows in the lower neighbour's recv_up (its own)
            ST_REQUIRE(ex.send_up && ex.send_down && ex.recv_up && ex.recv_down, "fabric: self-halo needs a middle strip");
            ST_NCCL(r->Send(ex.send_up, n, kNcclFloat, f->rank, comm, s));
            ST_NCCL(r->Recv(ex.recv_down, n, kNcclFloat, f->rank, comm, s));
            ST_NCCL(r->Send(ex.send_down, n, kNcclFloat, f->rank, comm, s));
            ST_NCCL(r->Recv(ex.recv_up, n, kNcclFloat, f->rank, comm, s));
        } else {
            if (ex.send_up && f->rank > 0) {
                ST_NCCL(r->Send(ex.send_up, n, kNcclFloat, f->rank - 1, comm, s));
                ST_NCCL(r->Recv(ex.recv_up, n, kNcclFloat, f->rank - 1, comm, s));
            }
            if (ex.send_down && f->rank < f->world - 1) {
                ST_NCCL(r->Send(ex.send_down, n, kNcclFloat, f->rank + 1, comm, s));
                ST_NCCL(r->Recv(ex.recv_down, n, kNcclFloat, f->rank + 1, comm, s));
            }
        }
        return 0;
        }();
        if (rc != 0) {
            r->GroupEnd();                       // closes the group; the first error message stays
            return 1;
        }
        ST_NCCL(r->GroupEnd());
        return 0;
    }
    if (ex.kind == 6) {
        // all-gather of opaque 32-bit words, in place: rank r's `count` words already lie at buffer + r * count.  Issued on
        // one rank too (RCCL makes it the identity there): the L-BFGS strip step on a single rank runs the same calls
        unsigned int* words = reinterpret_cast<unsigned int*>(ex.buffer);
        ST_NCCL(r->AllGather(words + (size_t)f->rank * n, words, n, kNcclUint32, comm, s));
        return 0;
    }
    if (f->world == 1) return 0;                 // a reduction or broadcast over one rank is the identity
    if (ex.kind == 2) ST_NCCL(r->AllReduce(ex.buffer, ex.buffer, n, kNcclFloat, kNcclSum, comm, s));
    else if (ex.kind == 4) ST_NCCL(r->Reduce(ex.buffer, ex.buffer, n, kNcclFloat, kNcclSum, ex.root, comm, s));
    else if (ex.kind == 5) ST_NCCL(r->Broadcast(ex.buffer, ex.buffer, n, kNcclFloat, ex.root, comm, s));
    else ST_REQUIRE(false, "fabric: unknown exchange kind %d", ex.kind);
    return 0;
}

int fabric_position(const st_fabric* f, int* rank, int* world) {
    ST_REQUIRE(f, "fabric: null fabric");
    *rank = f->rank;
    *world = f->world;
    return 0;
}

}  // namespace st

extern "C" {

int st_fabric_unique_id(unsigned char* id128) {
    ST_REQUIRE(id128, "st_fabric_unique_id: null argument");
    Rccl* r = rccl();
    ST_REQUIRE(r, "st_fabric_unique_id: librccl.so could not be loaded");
    NcclId id;
    ST_NCCL(r->GetUniqueId(&id));
    std::memcpy(id128, id.internal, 128);
    return 0;
}

int st_fabric_create(st_fabric** out, const unsigned char* id_trunk128, const unsigned char* id_heads128, int rank, int world,
                     int self_halo) {
    ST_REQUIRE(out && id_trunk128 && id_heads128, "st_fabric_create: null argument");
    ST_REQUIRE(world >= 1 && rank >= 0 && rank < world, "st_fabric_create: rank %d of %d", rank, world);
    ST_REQUIRE(!self_halo || world == 1, "st_fabric_create: the self-neighbour mode is for a single rank");
    Rccl* r = rccl();
    ST_REQUIRE(r, "st_fabric_create: librccl.so could not be loaded");
    st_fabric* f = new st_fabric();
    f->rank = rank; f->world = world; f->self_halo = self_halo;
    const unsigned char* ids[2] = {id_trunk128, id_heads128};
    for (int c = 0; c < 2; ++c) {
        NcclId id;
        std::memcpy(id.internal, ids[c], 128);
        const int rc = r->CommInitRank(&f->comm[c], world, id, rank);
        if (rc != 0) {
            st::set_error("ncclCommInitRank failed: %s", r->GetErrorString ? r->GetErrorString(rc) : "?");
            for (int k = 0; k < c; ++k) r->CommDestroy(f->comm[k]);
            delete f;
            return 1;
        }
    }
    *out = f;
    return 0;
}

// Pre-flight of a fresh fabric: every operation kind the phase machine uses, once per communicator, on tiny buffers, with a
// HOST-SIDE deadline - a transport that does not work on a system (mismatched ranks, a fabric RCCL cannot route) shows up
// here as an error the caller can act on (stylize() / bench.py fall back to torch.distributed) instead of as a hang in the
// first iteration.  Values: rank r sends 10 r + 1 upwards and 10 r + 2 downwards; the sum of (1, r) over the ranks; a
// reduction to rank 0; a broadcast from the last rank; an all-gather of 20 r + 3.
int st_fabric_selftest(st_fabric* f, void* stream, int timeout_ms) {
    ST_REQUIRE(f, "st_fabric_selftest: null fabric");
    (void)stream;
    // The test runs on a PRIVATE stream: if its RCCL kernels never complete, nothing the caller does next on its own stream
    // (the verdict's exchange over torch.distributed, a device synchronise of that stream's work) queues behind them - the
    // caller aborts the fabric first (sharding.NativeFabric), which ends them.  Everything the test allocates is released by
    // the guard below on every path on which the operations are known NOT to be in flight; after a timeout the device buffer
    // and the stream are left alone on purpose (something may still write / run there until the abort).
    struct Guard {
        float* dev = nullptr;
        hipEvent_t done = nullptr;
        hipStream_t stream = nullptr;
        bool in_flight = false;
        ~Guard() {
            if (done) hipEventDestroy(done);
            if (in_flight) return;
            if (dev) hipFree(dev);
            if (stream) hipStreamDestroy(stream);
        }
    } g;
    ST_HIP(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
    hipStream_t s = g.stream;
    const int r = f->rank, w = f->world;
    constexpr int kN = 4;                                    // floats per message
    float*& dev = g.dev;                                     // [send_up | send_down | recv_up | recv_down | sum | red | bc] x 2 channels
    constexpr int kSlots = 7;
    const int fixed = kN * kSlots * 2;                       // ... then the all-gather areas, w slots of kN per channel
    const int total = fixed + 2 * w * kN;
    ST_HIP(hipMalloc(&dev, sizeof(float) * total));
    std::vector<float> host_v(total, -1.f);
    float* host = host_v.data();
    for (int c = 0; c < 2; ++c) {
        float* h = host + c * kN * kSlots;
        for (int i = 0; i < kN; ++i) {
            h[0 * kN + i] = 10.f * r + 1.f + 100.f * c;
            h[1 * kN + i] = 10.f * r + 2.f + 100.f * c;
            h[2 * kN + i] = h[3 * kN + i] = -1.f;
            h[4 * kN + i] = (i & 1) ? (float)r : 1.f;
            h[5 * kN + i] = (float)(r + 1);
            h[6 * kN + i] = (r == w - 1) ? 7.f + c : -1.f;
            host[fixed + (c * w + r) * kN + i] = 20.f * r + 3.f + 100.f * c;
        }
    }
    ST_HIP(hipMemcpyAsync(dev, host, sizeof(float) * total, hipMemcpyHostToDevice, s));
    const bool up = f->self_halo || r > 0, down = f->self_halo || r < w - 1;
    for (int c = 0; c < 2; ++c) {
        float* d = dev + c * kN * kSlots;
        st_exchange ex{};
        ex.kind = 1; ex.count = kN; ex.channel = c; ex.stream = s;
        ex.send_up = up ? d : nullptr;             ex.recv_up = up ? d + 2 * kN : nullptr;
        ex.send_down = down ? d + kN : nullptr;    ex.recv_down = down ? d + 3 * kN : nullptr;
        // (an operation that failed to ENQUEUE leaves the earlier ones in flight: the buffers stay)
        auto failed = [&]() { f->stuck = true; g.in_flight = true; return 1; };
        if (up || down) { if (fabric_apply(f, ex, s)) return failed(); }
        st_exchange co{};
        co.count = kN; co.channel = c; co.stream = s;
        co.kind = 2; co.buffer = d + 4 * kN;
        if (fabric_apply(f, co, s)) return failed();
        co.kind = 4; co.buffer = d + 5 * kN; co.root = 0;
        if (fabric_apply(f, co, s)) return failed();
        co.kind = 5; co.buffer = d + 6 * kN; co.root = w - 1;
        if (fabric_apply(f, co, s)) return failed();
        co.kind = 6; co.buffer = dev + fixed + c * w * kN; co.root = 0;
        if (fabric_apply(f, co, s)) return failed();
    }
    hipEvent_t& done = g.done;
    g.in_flight = true;
    ST_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    ST_HIP(hipEventRecord(done, s));
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipEventQuery(done);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) { f->stuck = true; ST_HIP(q); }
        const auto ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
        if (ms > timeout_ms) {
            f->stuck = true;                     // the buffers stay allocated: something may still write to them
            st::set_error("st_fabric_selftest: rank %d of %d: the exchanges did not complete within %d ms", r, w, timeout_ms);
            return 1;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    g.in_flight = false;                         // everything completed: the guard releases buffer, event and stream
    ST_HIP(hipMemcpy(host, dev, sizeof(float) * total, hipMemcpyDeviceToHost));
    for (int c = 0; c < 2; ++c) {
        const float* h = host + c * kN * kSlots;
        const int upper = f->self_halo ? r : r - 1, lower = f->self_halo ? r : r + 1;
        for (int i = 0; i < kN; ++i) {
            // what arrives from above is the upper neighbour's DOWNWARD message and vice versa
            // (self-neighbour: fabric_apply's order puts the own upward rows into recv_down, the downward rows into recv_up)
            if (up) ST_REQUIRE(h[2 * kN + i] == 10.f * upper + 2.f + 100.f * c, "st_fabric_selftest: rank %d channel %d: halo from above is %g", r, c, h[2 * kN + i]);
            if (down) ST_REQUIRE(h[3 * kN + i] == 10.f * lower + 1.f + 100.f * c, "st_fabric_selftest: rank %d channel %d: halo from below is %g", r, c, h[3 * kN + i]);
            const float want_sum = (i & 1) ? 0.5f * w * (w - 1) : (float)w;
            ST_REQUIRE(h[4 * kN + i] == want_sum, "st_fabric_selftest: rank %d channel %d: all-reduce gave %g, expected %g", r, c, h[4 * kN + i], want_sum);
            if (r == 0) ST_REQUIRE(h[5 * kN + i] == 0.5f * w * (w + 1), "st_fabric_selftest: channel %d: reduce gave %g", c, h[5 * kN + i]);
            ST_REQUIRE(h[6 * kN + i] == 7.f + c, "st_fabric_selftest: rank %d channel %d: broadcast gave %g", r, c, h[6 * kN + i]);
            for (int q = 0; q < w; ++q) {
                const float got = host[fixed + (c * w + q) * kN + i];
                ST_REQUIRE(got == 20.f * q + 3.f + 100.f * c, "st_fabric_selftest: rank %d channel %d: all-gather slot %d is %g", r, c, q, got);
            }
        }
    }
    return 0;
}

// For a fabric whose operations may never complete (a rank left the run: Ctrl-C, an exception on one rank): ncclCommAbort
// instead of ncclCommDestroy, which would wait for them.
int st_fabric_abort(st_fabric* f) {
    if (f) f->stuck = true;
    return st_fabric_destroy(f);
}

int st_fabric_destroy(st_fabric* f) {
    if (!f) return 0;
    Rccl* r = rccl();
    for (NcclComm c : f->comm)
        if (c && r) {
            if (f->stuck && r->CommAbort) r->CommAbort(c);
            else r->CommDestroy(c);
        }
    delete f;
    return 0;
}

}  // extern "C"
