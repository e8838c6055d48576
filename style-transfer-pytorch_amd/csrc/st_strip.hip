// The strip-sharded closure: exchanges, the phase builder, comm-stream plumbing, head ownership and the
// st_plan_closure_* / st_plan_forward_begin / st_plan_set_rank entry points.
#include <cstring>

#include "st_plan.h"

namespace st {

int fabric_apply(st_fabric* f, const st_exchange& ex, hipStream_t fallback);      // st_fabric.hip

// ---- strip-sharded closure as a resumable sequence of phases -----------------
st_exchange no_exchange() {
    st_exchange e{};
    e.kind = 3;
    return e;
}
st_exchange halo_exchange(st_plan* p, float* halo, int channels, int width) {
    st_exchange e{};
    const size_t row = (size_t)channels * width;
    e.kind = 1;
    e.count = (long long)row + kHaloTrailer;
    e.send_up = p->has_up ? p->send_up : nullptr;                       // [rows | trailer]
    e.send_down = p->has_down ? p->send_down : nullptr;                 // [trailer | rows]
    e.recv_up = p->has_up ? halo - kHaloTrailer : nullptr;              // [trailer | top rows]
    e.recv_down = p->has_down ? halo + row : nullptr;                   // [bottom rows | trailer]
    return e;
}
// a node's boundary rows (masked where `mask` is given) into the two messages, with their bounds
int pack_halo_rows(st_plan* p, const float* src, const float* mask, int channels, int height, int width, hipStream_t s) {
    const size_t row = (size_t)channels * width;
    return launch_pack_rows(src, mask, channels, height, width, p->send_up, p->send_down + kHaloTrailer, s,
                            reinterpret_cast<unsigned int*>(p->send_up + row), reinterpret_cast<unsigned int*>(p->send_down),
                            p->pack_scratch);
}
// a halo block of `floats` payload floats with room for the two trailers around it
int halo_alloc(st_plan* p, float** out, size_t floats) {
    float* base = nullptr;
    if (plan_alloc(p, &base, floats + 2 * kHaloTrailer)) return 1;
    if (hipMemset(base, 0, (floats + 2 * kHaloTrailer) * sizeof(float)) != hipSuccess) { set_error("hipMemset of a halo block failed"); return 1; }
    *out = base + kHaloTrailer;
    return 0;
}
st_exchange allreduce_exchange(float* buffer, long long count) {
    st_exchange e{};
    e.kind = 2;
    e.count = count;
    e.buffer = buffer;
    return e;
}
st_exchange on_stream(st_exchange e, hipStream_t stream, int channel) {
    e.stream = stream;
    e.channel = channel;
    return e;
}
st_exchange rooted_exchange(int kind, float* buffer, long long count, int root) {
    st_exchange e{};
    e.kind = kind;          // 4: reduce (sum) to `root`, 5: broadcast from `root`
    e.count = count;
    e.buffer = buffer;
    e.root = root;
    return e;
}

struct PhaseBuilder {
    st_plan* p;
    std::vector<std::function<int(hipStream_t)>> pending;
    void add(std::function<int(hipStream_t)> f) { pending.push_back(std::move(f)); }
    void flush(st_exchange ex, const float* halo = nullptr) {
        auto steps = std::move(pending);
        pending.clear();
        st_plan::Phase ph;
        ph.run = [steps](hipStream_t s) {
            for (const auto& f : steps)
                if (f(s)) return 1;
            return 0;
        };
        ph.ex = ex;
        ph.halo = halo;
        p->phases.push_back(std::move(ph));
    }
};

// ---- strip plans: device-ordered exchanges -----------------------------------------------------------------------
// A halo exchange is issued on the plan's comm_stream behind the kernel that packed the boundary rows, and the
// convolution that consumes the halo is cut into an interior launch (no halo row needed: runs on the caller's stream
// while the rows are in flight) and a boundary launch behind the exchange (ConvProblem::overlap_part) wherever the
// cost model says the cut costs less than the exchange it hides (conv_pc_overlap_choice).  Transports that are not
// stream-ordered (the single-process lockstep emulation, gloo) perform every exchange synchronously between two
// phases; the event plumbing below is then a no-op and the results are the same.
int ensure_comm_stream(st_plan* p) {
    if (p->pack_done) return 0;
    if (ensure_streams(p)) return 1;               // (compact layout: the probed set provides the communication stream)
    if (!p->comm_stream) ST_HIP(hipStreamCreateWithFlags(&p->comm_stream, hipStreamNonBlocking));
    ST_HIP(hipEventCreateWithFlags(&p->pack_done, hipEventDisableTiming));
    ST_HIP(hipEventCreateWithFlags(&p->halo_landed, hipEventDisableTiming));
    return 0;
}

// Round 6: an exchange whose consumer is not cut has nothing to overlap with - the caller's stream records an event, the
// communication stream waits for it, carries the exchange, records an event, the caller's stream waits for that: two hops
// between hardware queues, ~22 us of idle trunk per exchange with nothing in flight (13 of a closure's 26 exchanges at
// 2896 x 2172 / 8: profiles/r06_strip_breakdown.md).  Those exchanges are issued IN LINE on the caller's stream instead
// (st_exchange::stream = null: "the stream the phase ran on"), between the pack kernel and the consumer, with no event at all.
// Operations of the trunk's communicator stay ordered: an in-line exchange follows the previous consumer's boundary launch
// (which waited for the communication stream), and the next comm_after_pack makes the communication stream wait for the
// caller's.  ST_STRIP_INLINE=0: every halo exchange on the communication stream (the round-4 / 5 form).
// ST_STRIP_HALO_BOUND=0: the round-4 halo bound, built on the communication stream (bound_with_halo)
bool shipped_halo_bound() {
    static Option opt("ST_STRIP_HALO_BOUND", 1);
    return opt.get() != 0;
}
bool inline_exchanges() {
    static Option inline_opt("ST_STRIP_INLINE", 1);
    return inline_opt.get() != 0 && shipped_halo_bound();
}
bool halo_is_inline(const st_plan* p, const float* halo) {
    auto it = p->halo_inline.find(halo);
    return it != p->halo_inline.end() && it->second;
}
// after the pack kernel: the exchange (issued by the transport on comm_stream) must start behind it
int comm_after_pack(st_plan* p, hipStream_t s, const float* halo) {
    if (halo_is_inline(p, halo)) return 0;         // (looked up when the phase RUNS: the consumer has been built by then)
    ST_HIP(hipEventRecord(p->pack_done, s));
    ST_HIP(hipStreamWaitEvent(p->comm_stream, p->pack_done, 0));
    return 0;
}
// before the first kernel that reads the halo block: wait for everything enqueued on comm_stream so far
int join_comm(st_plan* p, hipStream_t s, const float* halo) {
    if (halo_is_inline(p, halo)) return 0;
    ST_HIP(hipEventRecord(p->halo_landed, p->comm_stream));
    ST_HIP(hipStreamWaitEvent(s, p->halo_landed, 0));
    return 0;
}

// NS chains under sharding: head k's C x C work (everything between its Gram matrix and (Ssym, b)) is identical on every
// rank, so ONE rank - its owner - runs it and broadcasts the result: the two n = 512 chains land on different GPUs
// (no mutual slowdown, SURVEY.md 8(e) "layers are assigned to ranks") and the other ranks' GPUs stay free for the trunk.
// ST_STRIP_NS_OWNER=0: every rank runs every chain on the all-reduced moments (round-1 / round-2 behaviour).
int head_owner(const st_plan* p, int k) { return (4 - k) % p->world; }
bool heads_owned(const st_plan* p) {
    static Option owner_opt("ST_STRIP_NS_OWNER", 1);
    return p->world > 1 && owner_opt.get() != 0;
}

// Sharded plans: the head's OWNER rank has run style_head_chain; (Ssym | b | loss term) travel in one block.
int style_head_result_pack(st_plan* p, int idx, hipStream_t s) {          // owner, before the broadcast
    StyleHead& h = p->head[p->style_op[idx]];
    const size_t nn = (size_t)h.n * h.n;
    float* r = p->head_result[idx];
    ST_HIP(hipMemcpyAsync(r, h.ssym, nn * sizeof(float), hipMemcpyDeviceToDevice, s));
    ST_HIP(hipMemcpyAsync(r + nn, h.bvec, h.n * sizeof(float), hipMemcpyDeviceToDevice, s));
    ST_HIP(hipMemcpyAsync(r + nn + h.n, p->losses + 1 + idx, sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}
int style_head_result_unpack(st_plan* p, int idx, hipStream_t s) {        // every rank, after the broadcast
    StyleHead& h = p->head[p->style_op[idx]];
    const size_t nn = (size_t)h.n * h.n;
    const float* r = p->head_result[idx];
    ST_HIP(hipMemcpyAsync(h.ssym, r, nn * sizeof(float), hipMemcpyDeviceToDevice, s));
    ST_HIP(hipMemcpyAsync(h.bvec, r + nn, h.n * sizeof(float), hipMemcpyDeviceToDevice, s));
    ST_HIP(hipMemcpyAsync(p->losses + 1 + idx, r + nn + h.n, sizeof(float), hipMemcpyDeviceToDevice, s));
    // the fp16x3 1x1 kernel scales Ssym by a bound on max |Ssym|: measured here on every rank (the owner's epilogue
    // bound stays on the owner)
    if (p->net->conv_elem == 1 && launch_amax(h.ssym, (long long)nn, h.s_amax, 0, s)) return 1;
    return 0;
}

// fp16x3: the neighbours' halo rows are operands too, so the launch that reads them needs a bound over the operand AND
// its halo rows.  Built on the communication stream behind the exchange (it runs while the interior launch does; on the
// compute stream it was two 6.5 us launches per convolution, 0.3 ms per iteration and rank at 2896 x 2172 / 8), in a
// COPY of the operand's bound: the operand's own word may be being read - by the interior launch, by the tap's Gram
// kernel on a side stream - and must not change under its readers.
// Round 5: the SENDER measures max |row| while it packs the rows and ships the word with them (halo_exchange's trailers);
// the kernels take the maximum of the operand's own bound and the two trailer words - nothing runs between the halo's arrival
// and the boundary launch (ST_STRIP_HALO_BOUND=0: the round-4 form, a copy + an amax launch on the communication stream).
int bound_with_halo(st_plan* p, ConvProblem& c) {
    if (c.elem != 1 || !c.amax_word || !c.in_halo) return 0;
    if (shipped_halo_bound()) {
        const size_t row = (size_t)c.cin * c.width;
        c.halo_bound_up = c.has_up ? reinterpret_cast<const unsigned int*>(c.in_halo - kHaloTrailer) : nullptr;
        c.halo_bound_down = c.has_down ? reinterpret_cast<const unsigned int*>(c.in_halo + 2 * row) : nullptr;
        c.halo_amax_folded = 1;
        return 0;
    }
    ST_HIP(hipMemcpyAsync(p->halo_bound, c.amax_word, (size_t)kAmaxWordUints * sizeof(unsigned int), hipMemcpyDeviceToDevice,
                          p->comm_stream));
    c.amax_word = p->halo_bound;
    if (fold_halo_amax(c, p->comm_stream)) return 1;
    c.halo_amax_folded = 1;
    return 0;
}

// one strip convolution (forward or data gradient) whose operand halo is in flight on comm_stream
void add_strip_conv(st_plan* p, PhaseBuilder& b, const ConvProblem& whole, std::function<void(ConvProblem&)> late) {
    // `late` fills what is only known when the phase runs (nothing today besides the profile hook's state); the split
    // decision is a pure function of the shapes and is taken here, once
    PcOverlap o{};
    ConvProblem probe = whole;
    const bool split = conv_pc_overlap_choice(probe, &o) && o.pays && whole.in_halo != nullptr;
    if (whole.in_halo) p->halo_inline[whole.in_halo] = !split && inline_exchanges();
    if (split) {
        const double edge = (o.rows_b + o.rows_bottom) / (double)whole.height;      // share of the rows (and FLOPs) in the boundary launch
        b.add([=](hipStream_t s) {
            ConvProblem c = whole;
            late(c);
            c.overlap_part = 1;
            c.in_halo = nullptr; c.has_up = 0; c.has_down = 0;
            return conv_launch_profiled(p, c, s, 1.0 - edge);
        });
        b.add([=](hipStream_t s) {
            ConvProblem c = whole;
            late(c);
            c.overlap_part = 2;
            if (bound_with_halo(p, c)) return 1;
            if (join_comm(p, s, c.in_halo)) return 1;
            return conv_launch_profiled(p, c, s, edge);
        });
    } else {
        b.add([=](hipStream_t s) {
            ConvProblem c = whole;
            late(c);
            if (bound_with_halo(p, c)) return 1;
            if (join_comm(p, s, c.in_halo)) return 1;
            return conv_launch_profiled(p, c, s);
        });
    }
}

// fork_heads (closure only): right after a style tap is produced its local moment sums are computed on the head's side
// stream and reduced there (to the head's owner, or all-reduced), so neither the Gram kernel nor the collective sits on
// the trunk's stream; the owner's chain follows on the same stream and overlaps the remaining forward pass.
void build_forward_phases(st_plan* p, PhaseBuilder& b, const float* image, int last_layer, bool fork_heads = false) {
    const st_net* net = p->net;
    const int W = p->W;
    const bool f16 = net->conv_elem == 1;
    // the image's own boundary rows (conv1_1's replicate pad applies only at the global border; TV too): 35 KB, exchanged
    // on the caller's stream
    b.add([=](hipStream_t s) {
        if (ensure_comm_stream(p)) return 1;
        if (f16)      // fp16x3: Node::y_amax / g_amax of this pass
            ST_HIP(hipMemsetAsync(p->amax_word, 0, (size_t)64 * kAmaxWordUints * sizeof(float), s));
        return pack_halo_rows(p, image, nullptr, 3, p->H, W, s);
    });
    b.flush(halo_exchange(p, p->img_halo, 3, W));
    Node* prev = nullptr;
    for (int i = 0; i < kNumOps; ++i) {
        const OpDesc op = kProgram[i];
        if (op.feat_index > last_layer) break;
        Node* n = (op.kind == 0) ? &p->conv[op.index] : &p->pool[op.index];
        if (op.kind == 0 && op.index == 0) {
            b.add([=](hipStream_t s) {
                return launch_conv_first_fwd(image, net->w_first, net->bias[0], n->y, p->H, W, s, p->img_halo,
                                             p->has_up, p->has_down, f16 ? n->y_amax : nullptr);
            });
        } else if (op.kind == 0) {
            ConvProblem c{};
            forward_conv(p, i, c);
            c.in_halo = prev->yhalo; c.has_up = p->has_up; c.has_down = p->has_down;
            if (pool_follows(p, i, last_layer)) c.pool_out = p->pool[kProgram[i + 1].index].y;
            PcOverlap o{};
            const bool split = conv_pc_overlap_choice(c, &o) && o.pays;
            n->pooled_by_conv = fuse_pool(c, *n, fork_heads, split ? &o : nullptr);
            add_strip_conv(p, b, c, [](ConvProblem&) {});
        } else {
            Node* in = prev;
            b.add([=](hipStream_t s) {
                if (in->pooled_by_conv) return 0;
                return launch_pool_fwd(in->y, n->y, in->c, in->h, in->w, net->pooling, s);
            });
        }
        prev = n;
        if (fork_heads && op.kind == 0) {
            for (int k = 0; k < p->n_style; ++k) {
                if (p->style_op[k] != i) continue;
                const bool owned = heads_owned(p);
                const int owner = head_owner(p, k);
                const long long ch = p->head[i].n, nn = ch * ch;
                b.add([=](hipStream_t s) {
                    if (ensure_streams(p)) return 1;
                    hipStream_t hs = p->head_stream[k];
                    ST_HIP(hipEventRecord(p->tap_ready[k], s));
                    ST_HIP(hipStreamWaitEvent(hs, p->tap_ready[k], 0));
                    return moment_sums_of_tap(p, k, p->gram_raw[k], hs);
                });
                // (the first phase of a closure has created the streams; before that the handle is null and the
                // descriptor is rebuilt - see st_plan_closure_begin)
                st_exchange ex = owned ? rooted_exchange(4, p->gram_raw[k], nn + ch, owner)
                                       : allreduce_exchange(p->gram_raw[k], nn + ch);
                b.flush(on_stream(ex, p->head_stream[k], 1));
                b.add([=](hipStream_t) {
                    StyleHead& h = p->head[i];
                    if (owned && p->rank != owner) return 0;               // the owner's result arrives by broadcast
                    // the chain runs on the chain stream (compact layout) behind this head's reduction
                    hipStream_t hs = p->chain_stream ? p->chain_stream : p->head_stream[k];
                    ST_HIP(hipEventRecord(p->moments_ready[k], p->head_stream[k]));
                    ST_HIP(hipStreamWaitEvent(hs, p->moments_ready[k], 0));
                    if (launch_div_by_scalar(p->gram_raw[k], (float)h.npix, h.srm, nn, hs)) return 1;
                    if (launch_div_by_scalar(p->gram_raw[k] + nn, (float)h.npix, h.mean, h.n, hs)) return 1;
                    if (style_head_chain(p, head_site(p, k), hs)) return 1;
                    if (owned) {
                        if (style_head_result_pack(p, k, hs)) return 1;
                        ST_HIP(hipEventRecord(p->chain_done[k], hs));      // (the broadcast on the head's stream waits for it)
                        return 0;
                    }
                    if (style_head_gradient(p, head_site(p, k), hs)) return 1;
                    ST_HIP(hipEventRecord(p->head_done[k], hs));
                    return 0;
                });
            }
        }
        const bool next_is_conv = (i + 1 < kNumOps) && kProgram[i + 1].kind == 0 &&
                                  kProgram[i + 1].feat_index <= last_layer;
        if (next_is_conv && n->yhalo) {
            b.add([=](hipStream_t s) {
                if (pack_halo_rows(p, n->y, nullptr, n->c, n->h, n->w, s)) return 1;
                return comm_after_pack(p, s, n->yhalo);
            });
            b.flush(on_stream(halo_exchange(p, n->yhalo, n->c, n->w), p->comm_stream, 0), n->yhalo);
        }
    }
}

// the phases of a sequence are complete: the exchanges of in-line halo blocks name no stream (= the one the phase ran on)
void finish_phases(st_plan* p) {
    for (st_plan::Phase& ph : p->phases)
        if (ph.halo && ph.ex.kind == 1 && halo_is_inline(p, ph.halo)) ph.ex.stream = nullptr;
}

int build_closure_phases(st_plan* p, const float* image, float* grad_out) {
    p->phases.clear();
    p->halo_inline.clear();
    if (ensure_streams(p) || ensure_comm_stream(p)) return 1;      // the descriptors carry the stream handles
    PhaseBuilder b{p};
    build_forward_phases(p, b, image, 29, /*fork_heads=*/true);
    // TV on the raw image strip (uses the image halo): WRITES grad_out; content MSE on relu4_2
    b.add([=](hipStream_t s) {
        StripInfo si{p->row0, p->Hg, p->has_up, p->has_down, p->img_halo};
        return launch_tv_strip(image, p->H, p->W, si, p->tv_weight, grad_out, p->red_partials, p->lossbuf + 1, s);
    });
    Node* ct = &node_at(p, p->content_op[0]);
    const float* content_target = p->content_target[p->content_op[0]];
    b.add([=](hipStream_t s) {
        const long long global_count = (long long)ct->c * ct->hg * ct->w;
        return launch_content_mse_strip(ct->y, content_target, (long long)ct->count(), global_count,
                                        p->content_weight[0], ct->g, p->red_partials + 4 * kStreamBlocks, p->lossbuf, s);
    });
    b.flush(allreduce_exchange(p->lossbuf, 5));
    b.add([=](hipStream_t s) {
        const long long global_count = (long long)ct->c * ct->hg * ct->w;
        if (launch_content_mse_final(p->lossbuf, global_count, p->content_weight[0], p->losses + 0, s)) return 1;
        return launch_tv_final(p->lossbuf + 1, p->Hg, p->W, p->tv_weight, p->losses + 6, s);
    });
    // The style heads were forked tap by tap during the forward phases.  With owned heads the broadcasts are issued
    // HERE, in the order the backward needs them (4, 3, 2, 1, 0): operations of one communicator execute in issue
    // order, so a broadcast issued at tap time would hold every later head's reduction behind the owner's chain.
    const bool owned = heads_owned(p);
    auto join_head = [&](int conv_index) {
        for (int k = 0; k < p->n_style; ++k) {
            StyleHead& h = p->head[p->style_op[k]];
            if (!head_taps_conv(p, k, conv_index) || !owned || h.joined_in_build) continue;
            h.joined_in_build = true;
            const long long cnt = (long long)h.n * h.n + h.n + 1;
            if (p->rank == head_owner(p, k))
                b.add([=](hipStream_t) {
                    ST_HIP(hipStreamWaitEvent(p->head_stream[k], p->chain_done[k], 0));
                    return 0;
                });
            b.flush(on_stream(rooted_exchange(5, p->head_result[k], cnt, head_owner(p, k)), p->head_stream[k], 1));
            b.add([=](hipStream_t) {
                hipStream_t hs = p->head_stream[k];
                if (style_head_result_unpack(p, k, hs)) return 1;
                if (style_head_gradient(p, head_site(p, k), hs)) return 1;
                ST_HIP(hipEventRecord(p->head_done[k], hs));
                return 0;
            });
        }
    };
    for (int k = 0; k < p->n_style; ++k) p->head[p->style_op[k]].joined_in_build = false;
    // backward trunk: before each data gradient the masked boundary rows of its operand are exchanged
    const st_net* net = p->net;
    for (int i = kNumOps - 1; i >= 0; --i) {
        const OpDesc op = kProgram[i];
        if (op.kind == 1) {
            Node* n = &p->pool[op.index];
            Node* in = &p->conv[kProgram[i - 1].index];
            b.add([=](hipStream_t s) {
                if (in->coded) return launch_pool_bwd_codes(in->pool_code, n->g, in->g, in->c, in->h, in->w, s);
                return launch_pool_bwd(in->y, n->g, in->g, in->c, in->h, in->w, net->pooling, s);
            });
            continue;
        }
        Node* n = &p->conv[op.index];
        join_head(op.index);
        b.add([=](hipStream_t s) {
            // this conv's output gradient is about to be read: its style head (if any) must be done
            if (join_head_for_conv(p, op.index, s)) return 1;
            // (a coded node's map was not written this pass; its gradient left the pooling backward already masked)
            if (pack_halo_rows(p, n->g, n->coded ? nullptr : n->y, n->c, n->h, n->w, s)) return 1;
            return comm_after_pack(p, s, n->ghalo);
        });
        b.flush(on_stream(halo_exchange(p, n->ghalo, n->c, n->w), p->comm_stream, 0), n->ghalo);
        if (op.index == 0) {
            p->halo_inline[n->ghalo] = inline_exchanges();       // (conv1_1's data gradient is one launch)
            b.add([=](hipStream_t s) {
                if (join_comm(p, s, n->ghalo)) return 1;
                return launch_conv_first_dgrad(n->g, nullptr, net->w_first, grad_out, p->dp_scratch, p->H, p->W, 1, s, n->ghalo,
                                               p->has_up, p->has_down, p->dp_parts);
            });
            continue;
        }
        const OpDesc pop = kProgram[i - 1];
        if (pop.kind == 0) join_head(pop.index);
        if (pop.kind == 0)
            b.add([=](hipStream_t s) {
                // the launch ACCUMULATES into the input node's gradient: a style tap's head writes that buffer first
                return join_head_for_conv(p, pop.index, s);
            });
        ConvProblem c{};
        dgrad_conv(p, i, c);
        c.in_halo = n->ghalo; c.has_up = p->has_up; c.has_down = p->has_down;
        add_strip_conv(p, b, c, [](ConvProblem&) {});
    }
    b.add([=](hipStream_t s) { return launch_sum_losses(p->losses, s); });      // every head has been joined
    b.flush(no_exchange());
    finish_phases(p);
    return 0;
}

}  // namespace st

using namespace st;

extern "C" {

int st_plan_closure_begin(st_plan* p, const float* image, float* grad_out) {
    ST_REQUIRE(p && image && grad_out, "st_plan_closure_begin: null argument");
    ST_REQUIRE(p->strip, "st_plan_closure_begin: not a strip plan (use st_plan_create_strip)");
    if (require_targets(p) || ensure_grad_alloc(p)) return 1;
    for (int k = 0; k < p->n_style; ++k)
        if (ensure_style_alloc(p, p->head[p->style_op[k]], /*kind=*/0)) return 1;
    // (the tile / overlap / ownership decisions of the phase sequence depend on the library's switches)
    if (p->ph_image != image || p->ph_grad != grad_out || p->ph_last_layer != -1 || p->phases.empty() ||
        p->ph_option_gen != option_generation()) {
        if (build_closure_phases(p, image, grad_out)) return 1;
        p->ph_image = image; p->ph_grad = grad_out; p->ph_last_layer = -1;
        p->ph_option_gen = option_generation();
    }
    p->phase_pos = 0;
    return 0;
}

int st_plan_forward_begin(st_plan* p, const float* image, int last_layer) {
    ST_REQUIRE(p && image, "st_plan_forward_begin: null argument");
    ST_REQUIRE(p->strip, "st_plan_forward_begin: not a strip plan");
    ST_REQUIRE(last_layer >= 1 && last_layer <= 29, "st_plan_forward_begin: last_layer %d out of range", last_layer);
    p->phases.clear();
    p->halo_inline.clear();
    if (ensure_comm_stream(p)) return 1;       // the halo descriptors carry its handle
    PhaseBuilder b{p};
    build_forward_phases(p, b, image, last_layer);
    b.flush(no_exchange());
    finish_phases(p);
    p->ph_image = image; p->ph_grad = nullptr; p->ph_last_layer = last_layer;
    p->phase_pos = 0;
    return 0;
}

int st_plan_set_rank(st_plan* p, int rank, int world) {
    ST_REQUIRE(p && p->strip, "st_plan_set_rank: not a strip plan");
    ST_REQUIRE(world >= 1 && rank >= 0 && rank < world, "st_plan_set_rank: rank %d of %d", rank, world);
    p->rank = rank;
    p->world = world;
    p->phases.clear();          // head ownership is baked into the phase sequence
    return 0;
}

int st_plan_closure_next(st_plan* p, st_exchange* ex, void* stream) {
    ST_REQUIRE(p && ex, "st_plan_closure_next: null argument");
    if (p->phase_pos >= p->phases.size()) {
        std::memset(ex, 0, sizeof(*ex));
        return 0;
    }
    st_plan::Phase& ph = p->phases[p->phase_pos++];
    if (ph.run(static_cast<hipStream_t>(stream))) return 1;
    *ex = ph.ex;
    return 0;
}

int st_plan_closure_run(st_plan* p, st_fabric* fabric, void* stream) {
    ST_REQUIRE(p && fabric, "st_plan_closure_run: null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p->phase_pos == 0) {
        // Operations of ONE communicator must not run concurrently: the heads' collectives (channel 1) are ordered by
        // sharing a stream (the compact layout: every head's per-rank work on one stream), the trunk's (channel 0) by the
        // events between the caller's and the communication stream.  ST_STREAMS_COMPACT=0 gives every head a stream of its
        // own - fine for torch.distributed, whose process group serialises on its internal stream, not for this transport.
        void* head_stream = nullptr;
        for (const st_plan::Phase& ph : p->phases) {
            if (ph.ex.channel != 1 || ph.ex.kind == 0 || ph.ex.kind == 3) continue;
            ST_REQUIRE(!head_stream || !ph.ex.stream || ph.ex.stream == head_stream,
                       "st_plan_closure_run: the heads' exchanges name different streams (ST_STREAMS_COMPACT=0?): the in-library "
                       "transport needs the compact stream layout, use the descriptor form (ST_FABRIC_NATIVE=0) otherwise");
            if (ph.ex.stream) head_stream = ph.ex.stream;
        }
    }
    while (p->phase_pos < p->phases.size()) {
        st_plan::Phase& ph = p->phases[p->phase_pos++];
        if (ph.run(s)) return 1;
        if (st::fabric_apply(fabric, ph.ex, s)) return 1;
    }
    return 0;
}

}  // extern "C"
