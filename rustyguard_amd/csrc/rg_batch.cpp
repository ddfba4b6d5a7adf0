// rg_batch.cpp -- kernel-family routing and the device API of include/rg_aead.h: batches whose frames,
// descriptors and keys are already in device memory, enqueued on the caller's stream.
#include <algorithm>

#include "rg_host.h"

using namespace rg::host;
using rg::DeviceGuard;

namespace {

rg::Launch launch_cfg(rg_ctx *ctx, size_t n, bool open) {
    rg::Launch L;
    L.done = nullptr;
    L.lanes = rg_get_lanes_per_packet(ctx, n);
    L.cus = ctx->cus;
    L.staged_g = rg_get_kernel(ctx, n);
    L.debug_mode = open ? (ctx->debug_mode == 3 ? 3 : 0) : ctx->debug_mode;
    const int cap = std::max(1, ctx->pipe_max_wg[open ? 1 : 0]);
    if (ctx->wg_per_cu < 0) {
        L.wg_per_cu = 0;
    } else if (ctx->wg_per_cu > 0) {
        L.wg_per_cu = std::min(ctx->wg_per_cu, cap);
    } else {
        // enough resident workgroups for one lane per packet segment, capped by occupancy
        const size_t need = ((size_t)n * L.lanes + 255) / 256;
        const size_t per_cu = (need + L.cus - 1) / std::max(1, L.cus);
        L.wg_per_cu = (int)std::max<size_t>(1, std::min<size_t>(per_cu, (size_t)cap));
    }
    return L;
}

// Tile kernels: persistent grid of 4-wave workgroups, two resident per CU
// (2 waves per SIMD: the VGPR budget of the kernel).  With the planner the
// work lists and the per-class segment counts are built on the device; without
// it packets stay in array order and the segment count follows from n.
hipError_t launch_tiles_any(rg_ctx *ctx, const rg::SealArgs *sa, const rg::OpenArgs *oa, PlanBuf &pb,
                            const rg::Launch &L, hipStream_t st) {
    const uint32_t n = sa ? sa->n : oa->n;
    rg::TilePlan tp{};
    tp.target_lanes = (uint32_t)std::max(1, ctx->cus) * 256u; // one wave per SIMD
    tp.fixed_k = (uint32_t)ctx->segments;
    tp.gq = pb.pool();
    bool plan = ctx->plan == 1;
    if (ctx->plan == 2) {
        hipError_t e = pb.reserve(n);
        if (e != hipSuccess) return e;
        plan = pb.want_plan(st);
    }
    // the tile kernel deals its last rounds from a grid-wide pool: statuses pending and the control block
    // cleared first, planned or not
    {
        hipError_t e = pb.preset(sa ? sa->status : oa->status, n, st);
        if (e != hipSuccess) return e;
    }
    if (plan) {
        hipError_t e = pb.reserve(n);
        if (e != hipSuccess) return e;
        tp.counts = pb.counts();
        tp.lists = static_cast<uint32_t *>(pb.lists.p);
        tp.cap = pb.cap;
        tp.classes_out = pb.d_classes;
        e = rg::launch_plan(sa ? sa->desc : oa->desc, n, oa != nullptr, tp, st);
        if (e != hipSuccess) return e;
    } else if (!tp.fixed_k) {
        tp.fixed_k = n >= tp.target_lanes ? 1u : 2ull * n >= tp.target_lanes ? 2u : 4u;
    }
    return rg::launch_tiles(sa, oa, L.staged_g, tp, L, st);
}

// Pipelined kernel: planned (size classes, per-class segments, tile queue) or
// in array order with lanes_per_packet segments.
hipError_t launch_pipe_any(rg_ctx *ctx, const rg::SealArgs *sa, const rg::OpenArgs *oa, PlanBuf &pb,
                           const rg::Launch &L, hipStream_t st) {
    const uint32_t n = sa ? sa->n : oa->n;
    bool plan = ctx->plan == 1;
    if (ctx->plan == 2) {
        hipError_t e = pb.reserve(n);
        if (e != hipSuccess) return e;
        plan = pb.want_plan(st);
    }
    // array order: lane unit u is packet u >> lg, by index alone -- no hand-off, no preset
    if (!plan) return rg::launch_pipe(sa, oa, L, nullptr, st);
    rg::Launch Lp = L;
    // two workgroups per CU are asked for, but the kernels' register budget (268 / 264 VGPR+AGPR, above
    // 256) admits one wave per SIMD, and the occupancy query (pipe_max_wg) caps the request at that:
    // the planned kernel runs one wave per SIMD.  Two co-resident waves, forced with
    // __launch_bounds__(256, 2), measured slower on config 2 (profiles/r4_cfg2_twowave.txt).
    const int want_wg = ctx->wg_per_cu > 0 ? ctx->wg_per_cu : 2;
    Lp.wg_per_cu = std::min(want_wg, std::max(1, ctx->pipe_max_wg[oa ? 1 : 0]));
    hipError_t e = pb.reserve(n);
    if (e != hipSuccess) return e;
    // the planner's last workgroup hands the schedule to the transport kernel: statuses pending and the
    // control block (counts, finished-workgroup count, schedule) cleared first -- a lost hand-off leaves an
    // empty schedule and every status pending
    e = pb.preset(sa ? sa->status : oa->status, n, st);
    if (e != hipSuccess) return e;
    rg::TilePlan tp{};
    tp.counts = pb.counts();
    tp.lists = static_cast<uint32_t *>(pb.lists.p);
    tp.cap = pb.cap;
    tp.sched = pb.sched();
    tp.simds = (uint32_t)std::max(1, ctx->cus) * 4u; // balance per SIMD: co-resident waves share its issue slots
    tp.classes_out = pb.d_classes;
    e = rg::launch_plan(sa ? sa->desc : oa->desc, n, oa != nullptr, tp, st);
    if (e != hipSuccess) return e;
    rg::PipePlan pp{pb.counts(), static_cast<const uint32_t *>(pb.lists.p), pb.cap, pb.sched(), pb.d_classes,
                    tp.simds};
    return rg::launch_pipe(sa, oa, Lp, &pp, st);
}

// Flattened chunk-stream kernel: units of equal work (planner on / auto) or of
// equal packet counts (planner off); the balancing runs inside the kernel.
hipError_t launch_flat_any(rg_ctx *ctx, const rg::SealArgs *sa, const rg::OpenArgs *oa, hipStream_t st,
                           hipEvent_t done) {
    hipError_t e = ctx->d_junk.reserve(rg::flat_junk_bytes(ctx->cus));
    if (e != hipSuccess) return e;
    return rg::launch_flat(sa, oa, ctx->plan != 0, static_cast<uint4 *>(ctx->d_junk.p), ctx->cus, st, done);
}

// Automatic choice between the two small-batch kernels: when the last planned batch of this planner
// held more than one size class (mixed sizes, e.g. IMIX), the flattened chunk stream runs -- it
// balances mixed sizes inside the kernel, without a planner pass; every 32nd call goes back to the
// planned pipelined kernel, whose planner refreshes the class count (a uniform batch returns there),
// except inside a stream capture: a captured graph replays one route, and it should be the fast one.
int pick_family(rg_ctx *ctx, int g, PlanBuf &pb, hipStream_t st) {
    if (ctx->staged_g >= 0 || g != 0 || ctx->plan != 2 || !pb.h_classes) return g;
    const uint32_t cls = *pb.h_classes;
    if (cls < 2 || cls == ~0u) return g;
    const bool cap = capturing(st);
    if ((pb.calls % 32) != 0 || cap) {
        ++pb.calls;
        return 3;
    }
    return g;
}

// rg_seal_batch_dev / rg_open_batch_dev behind their own argument rule (bad): a batch of n packets on the
// context's planner, with the stream mark of claim_stream behind it
int dev_batch(rg_ctx *ctx, size_t n, bool bad, const char *bad_text, rg::SealArgs *sa, rg::OpenArgs *oa, void *stream) {
    DeviceGuard dg_;
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (bad || n > 0xFFFFFFFFull) return set_err(RG_EINVAL, bad_text);
    hipStream_t st = (hipStream_t)stream;
    rc = claim_stream(ctx, st);
    if (rc) return rc;
    (sa ? sa->n : oa->n) = (uint32_t)n;
    hipEvent_t ev = stream_event(ctx, st);
    RG_HIP(launch_any(ctx, sa, oa, ctx->plan_dev, st, ev), sa ? "seal launch" : "open launch");
    if (ev) mark_stream(ctx, st);
    return RG_OK;
}

} // namespace

hipError_t rg::host::launch_any(rg_ctx *ctx, const rg::SealArgs *sa, const rg::OpenArgs *oa, PlanBuf &pb,
                                hipStream_t st, hipEvent_t done) {
    rg::Launch L = launch_cfg(ctx, sa ? sa->n : oa->n, oa != nullptr);
    L.done = done;
    L.staged_g = pick_family(ctx, L.staged_g, pb, st);
    ctx->last_kernel = L.staged_g;
    // stamps (diagnostic builds): debug mode 3, or any diagnostic mode of the pipelined kernel (an open
    // knows mode 3 alone: launch_cfg)
    uint64_t *dbg = L.debug_mode == 3 || (L.staged_g == 0 && L.debug_mode != 0) ? ctx->dbg : nullptr;
    rg::SealArgs s;
    rg::OpenArgs o;
    if (sa) {
        s = *sa;
        s.dbg = dbg;
        sa = &s;
    } else {
        o = *oa;
        o.dbg = dbg;
        oa = &o;
    }
    if (L.staged_g == 3) return launch_flat_any(ctx, sa, oa, st, done);
    if (L.staged_g == 0) return launch_pipe_any(ctx, sa, oa, pb, L, st);
    return launch_tiles_any(ctx, sa, oa, pb, L, st);
}

extern "C" {

int rg_seal_batch_dev(rg_ctx *ctx, const uint8_t *keys, const uint32_t *receivers, uint32_t nkeys,
                      const rg_pkt_desc *desc, const uint64_t *counters, size_t n, uint8_t *buf, size_t buf_len,
                      uint8_t *status, void *stream) {
    rg::SealArgs a{};
    a.keys = reinterpret_cast<const uint32_t *>(keys);
    a.receivers = receivers;
    a.desc = desc;
    a.counters = counters;
    a.buf = buf;
    a.buf_len = buf_len;
    a.status = status;
    a.nkeys = nkeys;
    return dev_batch(ctx, n, !keys || !desc || !counters || !buf || !status || nkeys == 0,
                     "seal: bad args (status is required)", &a, nullptr, stream);
}

int rg_open_batch_dev(rg_ctx *ctx, const uint8_t *keys, uint32_t nkeys, const rg_pkt_desc *desc, size_t n,
                      uint8_t *buf, size_t buf_len, uint8_t *status, uint64_t *counters_out, void *stream) {
    rg::OpenArgs a{};
    a.keys = reinterpret_cast<const uint32_t *>(keys);
    a.desc = desc;
    a.buf = buf;
    a.buf_len = buf_len;
    a.status = status;
    a.counters_out = counters_out;
    a.nkeys = nkeys;
    return dev_batch(ctx, n, !keys || !desc || !buf || !status || nkeys == 0, "open: bad args", nullptr, &a, stream);
}

int rg_synth_fill_dev(rg_ctx *ctx, const rg_pkt_desc *desc, const uint32_t *inner_len, size_t n, uint8_t *buf,
                      size_t buf_len, uint64_t seed, void *stream) {
    DeviceGuard dg_;
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!desc || !inner_len || !buf || n > 0x7FFFFFFFull) return set_err(RG_EINVAL, "synth: bad args");
    RG_HIP(rg::launch_synth_fill(desc, inner_len, (uint32_t)n, buf, buf_len, seed, (hipStream_t)stream),
           "synth launch");
    return RG_OK;
}

int rg_rx_table_build(const uint32_t *receivers, const uint32_t *key_idx, size_t n, rg_rx_entry *table,
                      uint32_t cap) {
    if (!table || (n && (!receivers || !key_idx))) return set_err(RG_EINVAL, "rx table: null pointer");
    if (!pow2(cap) || (uint64_t)cap < 2ull * n)
        return set_err(RG_EINVAL, "rx table: cap must be a power of two >= 2 n");
    for (uint32_t s = 0; s < cap; ++s) table[s] = rg_rx_entry{0, RG_KEY_SKIP};
    for (size_t i = 0; i < n; ++i) {
        if (key_idx[i] == RG_KEY_SKIP) return set_err(RG_EINVAL, "rx table: key index RG_KEY_SKIP is reserved");
        uint32_t s = rg::rx_slot(receivers[i], cap);
        while (table[s].key_idx != RG_KEY_SKIP) {
            if (table[s].receiver == receivers[i]) return set_err(RG_EINVAL, "rx table: duplicate receiver");
            s = (s + 1) & (cap - 1);
        }
        table[s] = rg_rx_entry{receivers[i], key_idx[i]};
    }
    return RG_OK;
}

int64_t rg_rx_table_find(const rg_rx_entry *table, uint32_t cap, uint32_t receiver) {
    if (!table || !pow2(cap)) return -1;
    const uint32_t k = rg::rx_find(table, cap, receiver);
    return k == RG_KEY_SKIP ? -1 : (int64_t)k;
}

// Config::get_peer_idx as a table over peer rows (rg_handshake.hip reads it): the receiver table's slot rule
// on the public key's first word.  Keys are compared over all 32 bytes, without an early exit.
static uint32_t peer_key_diff(const uint8_t *a, const uint8_t *b) {
    uint32_t diff = 0;
    for (int i = 0; i < 32; ++i) diff |= (uint32_t)(a[i] ^ b[i]);
    return diff;
}

static uint32_t peer_key_word(const uint8_t *pk) {
    return (uint32_t)pk[0] | ((uint32_t)pk[1] << 8) | ((uint32_t)pk[2] << 16) | ((uint32_t)pk[3] << 24);
}

int rg_peer_table_build(const rg_hs_peer *peers, uint32_t npeers, uint32_t *table, uint32_t cap) {
    if (!table || (npeers && !peers)) return set_err(RG_EINVAL, "peer table: null pointer");
    if (!pow2(cap) || (uint64_t)cap < 2ull * npeers)
        return set_err(RG_EINVAL, "peer table: cap must be a power of two >= 2 npeers");
    for (uint32_t s = 0; s < cap; ++s) table[s] = RG_PEER_NONE;
    for (uint32_t i = 0; i < npeers; ++i) {
        uint32_t s = rg::rx_slot(peer_key_word(peers[i].public_key), cap);
        while (table[s] != RG_PEER_NONE) {
            if (peer_key_diff(peers[table[s]].public_key, peers[i].public_key) == 0)
                return set_err(RG_EINVAL, "peer table: duplicate public key");
            s = (s + 1) & (cap - 1);
        }
        table[s] = i;
    }
    return RG_OK;
}

int64_t rg_peer_table_find(const rg_hs_peer *peers, const uint32_t *table, uint32_t cap, const uint8_t pk[32]) {
    if (!peers || !table || !pk || !pow2(cap)) return -1;
    uint32_t s = rg::rx_slot(peer_key_word(pk), cap);
    for (uint32_t probe = 0; probe < cap && table[s] != RG_PEER_NONE; ++probe) {
        if (peer_key_diff(peers[table[s]].public_key, pk) == 0) return table[s];
        s = (s + 1) & (cap - 1);
    }
    return -1;
}

int rg_open_batch_dev_rx(rg_ctx *ctx, const uint8_t *keys, uint32_t nkeys, const rg_rx_entry *rx_table,
                         uint32_t rx_cap, const rg_pkt_desc *desc, size_t n, uint8_t *buf, size_t buf_len,
                         uint8_t *status, uint64_t *counters_out, uint32_t *key_idx_out, void *stream) {
    DeviceGuard dg_;
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!rx_table || !pow2(rx_cap) || !desc || n > 0xFFFFFFFFull)
        return set_err(RG_EINVAL, "open_rx: bad args");
    rc = claim_stream(ctx, (hipStream_t)stream); // before the resolve pass writes the context's descriptors
    if (rc) return rc;
    // resolved descriptors live in the context: calls on one context are stream-ordered
    RG_HIP(ctx->d_rx_desc.reserve(n * sizeof(rg_pkt_desc)), "rx descriptors");
    auto *rd = static_cast<rg_pkt_desc *>(ctx->d_rx_desc.p);
    RG_HIP(rg::launch_rx_resolve(desc, (uint32_t)n, buf, buf_len, rx_table, rx_cap, rd, key_idx_out,
                                 (hipStream_t)stream),
           "rx resolve launch");
    return rg_open_batch_dev(ctx, keys, nkeys, rd, n, buf, buf_len, status, counters_out, stream);
}

int rg_mac_verify_batch_dev(rg_ctx *ctx, const uint8_t *keys, uint32_t key_len, uint32_t nkeys, int which,
                            const rg_pkt_desc *desc, size_t n, const uint8_t *buf, size_t buf_len, uint8_t *status,
                            uint32_t *key_idx_out, void *stream) {
    DeviceGuard dg_;
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!keys || nkeys == 0 || (key_len != 16 && key_len != 32) || (which != 1 && which != 2) || !desc || !buf ||
        !status || n > 0xFFFFFFFFull)
        return set_err(RG_EINVAL, "mac verify: bad args");
    rg::MacArgs a{};
    a.keys = reinterpret_cast<const uint32_t *>(keys);
    a.key_len = key_len;
    a.nkeys = nkeys;
    a.which = (uint32_t)which;
    a.n = (uint32_t)n;
    a.desc = desc;
    a.buf = buf;
    a.buf_len = buf_len;
    a.status = status;
    a.key_out = key_idx_out;
    // the states are key material: a regrow wipes the old block behind its readers, on this stream
    std::lock_guard<std::mutex> g(ctx->mu);
    hipStream_t st = (hipStream_t)stream;
    RG_HIP(ctx->d_mac_keys.reserve((size_t)nkeys * 32, st), "mac key states");
    a.key_state = static_cast<uint32_t *>(ctx->d_mac_keys.p);
    RG_HIP(rg::launch_mac_verify(a, st), "mac verify launch");
    RG_HIP(ctx->d_mac_keys.use(st), "mac key states event");
    return RG_OK;
}

} // extern "C"
