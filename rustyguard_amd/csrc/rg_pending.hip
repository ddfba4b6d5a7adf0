// rg_pending.hip -- the initiator's pending handshakes kept on the device: which peers get an initiation, which
// pending row it lands in, when a lost one is retried and when an abandoned one is reaped is decided on the stream
// that sends and receives.  The reference does this at the tail of new_handshake
// (rustyguard-core/src/handshake.rs:266-297, 319-322) and in the InitAttempt and ExpireHandshake arms of
// tick_timers (rustyguard-core/src/time.rs:49-83, 99-113) over Peer.current_handshake.
//
//   rg_pending_install_batch_dev  behind the initiator chain: its pending rows become the peers' current_handshake
//   rg_pending_turn_dev           retry and expiry over the whole table, merged with a list of requests
//                                 -> (peers to initiate to, gate, expired flags, counts)
//   rg_pending_index_dev          pend_table over the live rows, alone
//
// The table has one row a peer and one source of liveness, pending[p].peer == p, so the finish call's wipe ends a
// row's life with no call of this file.  Both calls equal an in-order loop (include/rg_aead.h has them) with
// nothing decided by the order the lanes arrive in.  The install's kernels, all on its stream:
//   clear    claim[p] = 0; pend_table all empty
//   claim    one lane per row: installed_out = RG_PEER_NONE; a gated row gets its answer; every other row with a
//            peer below npeers takes atomicMax(claim[p], i + 1): the last row of a peer in array order
//   commit   eight lanes per peer, one per 16-byte piece of the claimed row; the lane of the piece that holds
//            `peer` reads whether the row was live before it overwrites it, and writes the timers, hs_ids and
//            installed_out
//   wipe     eight lanes per row of the batch, behind the commit that read it; the lane of the `peer` piece reads
//            the peer first and stores the status last
//   index    one lane per live row claims its pend_table entry (rg_rxclaim.h)
// The turn's:
//   clear    want[p] = 0, the list and the gate all padding, the counts zero; pend_table all empty
//   row      one lane per peer: a live row past REKEY_ATTEMPT_TIME since its last attempt is wiped (want bit
//            kExpired), one past REKEY_TIMEOUT within REKEY_ATTEMPT_TIME of its first is stamped (want bit kInit)
//   request  one lane per entry of the request list: a peer without a live row gets kInit (atomicOr: the same
//            word whatever the order)
//   compact  rg_grouped.h's count / carry / rank over the peers, PendWants in both walks: (init, expired) of each
//            peer, both counts in one 64-bit sum; init_peers_out[rank] = the peer, init_gate_out[rank] = RG_PKT_OK
//   index    as above
// The two row rules cannot both hold without clock wrap: started_ns <= sent_ns, so sent_ns + 90 s < now implies
// started_ns + 90 s < now, which the retry rule excludes.  With a wrapping clock the expiry is taken.
//
// The entry points' host side is here too (rg_session.hip's precedent).  Every argument rule is answered before the
// device is selected.  All scratch is the caller's; nothing is allocated, waited for or kept in the context, and
// every fill is a kernel, so the calls capture into a graph without memset nodes.
#include "rg_host.h"
#include "rg_grouped.h"
#include "rg_rxclaim.h"

namespace rg {
namespace {

constexpr uint64_t kRetryNs = RG_REKEY_TIMEOUT_NS;
constexpr uint64_t kAttemptNs = RG_REKEY_ATTEMPT_TIME_NS;

constexpr uint32_t kRowQuads = sizeof(rg_hs_pending) / 16; // a pending row in 16-byte pieces
constexpr uint32_t kPeerQuad = 6;                          // the piece that holds peer (.x) and sender (.y)
static_assert(kRowQuads == 8 && offsetof(rg_hs_pending, peer) == 16 * kPeerQuad &&
                  offsetof(rg_hs_pending, sender) == 16 * kPeerQuad + 4,
              "rg_hs_pending layout");

constexpr uint32_t kInit = 1u, kExpired = 2u;                // want[p]
constexpr uint64_t kOneInit = 1ull, kOneExp = 1ull << 32;    // one sum: initiations in the low word, expiries in the high

// rg_pending_tables as the kernels take it
struct Tables {
    uint4 *pending;                 // [npeers][kRowQuads]
    uint64_t *timers;               // [npeers][2]: started_ns, sent_ns
    uint32_t *hs_ids;               // [npeers]
    unsigned long long *pend_table; // [pend_cap] sender | peer << 32
    uint32_t npeers, pend_cap;
};

__device__ __forceinline__ bool live(const Tables &t, uint32_t p) { return t.pending[(uint64_t)kRowQuads * p + kPeerQuad].x == p; }
// piece q of a wiped row: zeros with peer = RG_PEER_NONE
__device__ __forceinline__ uint4 wiped_quad(uint32_t q) {
    return make_uint4(q == kPeerQuad ? RG_PEER_NONE : 0u, 0, 0, 0);
}

// ------------------------------------------------------ the pending table
__global__ __launch_bounds__(256) void pend_fill_kernel(Tables t) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s < t.pend_cap) t.pend_table[s] = kRxEmpty;
}
__global__ __launch_bounds__(256) void pend_index_kernel(Tables t) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= t.npeers || !live(t, p)) return;
    rx_claim(t.pend_table, t.pend_cap, t.pending[(uint64_t)kRowQuads * p + kPeerQuad].y, p);
}

// ------------------------------------------------------------- the install
struct InstallArgs {
    Tables t;
    uint4 *batch;        // [n][kRowQuads]
    const uint8_t *gate; // [n] or nullptr
    const uint64_t *now_ns;
    uint8_t *status;         // [n]
    uint32_t *installed_out; // [n]
    uint32_t *claim;         // [npeers]
    uint32_t n;
};

// one lane per peer or table entry, whichever are more
__global__ __launch_bounds__(256) void install_clear_kernel(InstallArgs a) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k < a.t.npeers) a.claim[k] = 0;
    if (k < a.t.pend_cap) a.t.pend_table[k] = kRxEmpty;
}

__global__ __launch_bounds__(256) void install_claim_kernel(InstallArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    a.installed_out[i] = RG_PEER_NONE;
    if (a.gate && a.gate[i] != RG_PKT_OK) {
        a.status[i] = RG_PKT_REJECTED; // nothing else of the row is read or written
        return;
    }
    const uint32_t p = a.batch[(uint64_t)kRowQuads * i + kPeerQuad].x;
    if (p < a.t.npeers) atomicMax(&a.claim[p], i + 1); // the last one in array order: i + 1 <= 2^32 - 1
}

__global__ __launch_bounds__(256) void install_commit_kernel(InstallArgs a) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t p64 = k / kRowQuads;
    if (p64 >= a.t.npeers) return;
    const uint32_t p = (uint32_t)p64, q = (uint32_t)(k % kRowQuads);
    const uint32_t c = a.claim[p];
    if (c == 0 || c > a.n) return; // no row of this batch names the peer
    const uint32_t i = c - 1;
    const uint4 piece = a.batch[(uint64_t)kRowQuads * i + q];
    uint4 *dst = a.t.pending + (uint64_t)kRowQuads * p + q;
    if (q != kPeerQuad) {
        *dst = piece;
        return;
    }
    const bool was_live = dst->x == p; // only this lane writes the piece
    const uint64_t now = *a.now_ns;
    uint64_t *tm = a.t.timers + 2ull * p;
    if (!was_live) tm[0] = now; // a retry keeps `started`
    tm[1] = now;
    a.t.hs_ids[p] = piece.y;
    *dst = piece;
    a.installed_out[i] = p;
}

__global__ __launch_bounds__(256) void install_wipe_kernel(InstallArgs a) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t i = k / kRowQuads;
    if (i >= a.n) return;
    if (a.gate && a.gate[i] != RG_PKT_OK) return; // answered by the claim kernel
    const uint32_t q = (uint32_t)(k % kRowQuads);
    uint4 *piece = a.batch + (uint64_t)kRowQuads * i + q;
    if (q != kPeerQuad) {
        *piece = wiped_quad(q);
        return;
    }
    const uint32_t p = piece->x;
    *piece = wiped_quad(q);
    a.status[i] = p < a.t.npeers ? RG_PKT_OK : RG_PKT_INVALID; // after the row
}

// ---------------------------------------------------------------- the turn
struct TurnArgs {
    Tables t;
    const uint64_t *now_ns;
    const uint32_t *start_peers; // [m] or nullptr
    const uint8_t *start_status; // [m] or nullptr
    uint32_t start_match, m;
    uint32_t *want;           // [npeers]
    uint32_t *init_peers_out; // [npeers]
    uint8_t *init_gate_out;   // [npeers]
    uint8_t *expired_out;     // [npeers] or nullptr
    uint32_t *counts_out;     // [2]
};

// one lane per peer or table entry, whichever are more: nothing wanted, the list and the gate all padding, the
// counts zero, the table empty
__global__ __launch_bounds__(256) void turn_clear_kernel(TurnArgs a) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k == 0) a.counts_out[0] = a.counts_out[1] = 0;
    if (k < a.t.npeers) {
        a.want[k] = 0;
        a.init_peers_out[k] = RG_PEER_NONE;
        a.init_gate_out[k] = RG_PKT_REJECTED;
    }
    if (k < a.t.pend_cap) a.t.pend_table[k] = kRxEmpty;
}

__global__ __launch_bounds__(256) void turn_row_kernel(TurnArgs a) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.t.npeers) return;
    bool gone = false;
    if (live(a.t, p)) {
        const uint64_t now = *a.now_ns;
        uint64_t *tm = a.t.timers + 2ull * p;
        const uint64_t started = tm[0], sent = tm[1];
        if (sent + kAttemptNs < now) { // ExpireHandshake: wrapping, strict
            uint4 *row = a.t.pending + (uint64_t)kRowQuads * p;
#pragma unroll
            for (uint32_t q = 0; q < kRowQuads; ++q) row[q] = wiped_quad(q);
            tm[0] = 0;
            tm[1] = 0;
            a.want[p] = kExpired;
            gone = true;
        } else if (sent + kRetryNs < now && now < started + kAttemptNs) { // InitAttempt and should_reinit
            tm[1] = now; // new_handshake stamps `sent` before it can fail
            a.want[p] = kInit;
        }
    }
    if (a.expired_out) a.expired_out[p] = gone ? 1 : 0;
}

__global__ __launch_bounds__(256) void turn_request_kernel(TurnArgs a) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.m) return;
    if (a.start_status && a.start_status[j] != a.start_match) return;
    const uint32_t q = a.start_peers[j];
    if (q < a.t.npeers && !live(a.t, q)) atomicOr(&a.want[q], kInit); // a live row's own retry governs
}

// The pass of rg_grouped.h's compact over the peers: what peer p adds to the two counts, and where its rank on
// the list of initiations sends it.
struct PendWants {
    TurnArgs a;
    __device__ __forceinline__ uint64_t item(uint64_t pos) const {
        const uint32_t w = a.want[pos];
        return ((w & kInit) ? kOneInit : 0) | ((w & kExpired) ? kOneExp : 0);
    }
    __device__ __forceinline__ void emit(uint64_t pos, uint64_t w, uint64_t ex) const {
        const uint32_t k = (uint32_t)ex;
        if ((w & kOneInit) && k < a.t.npeers) {
            a.init_peers_out[k] = (uint32_t)pos;
            a.init_gate_out[k] = RG_PKT_OK;
        }
    }
    __device__ __forceinline__ void total(uint64_t all) const {
        a.counts_out[0] = (uint32_t)all;
        a.counts_out[1] = (uint32_t)(all >> 32);
    }
};

struct PendingLayout {
    uint64_t words; // [npeers] u32: the install's claim, the turn's want
    AggLayout agg;  // u64 sums of the peers' tiles
    uint64_t total;
};
PendingLayout pending_layout(uint64_t n, uint64_t m, uint64_t npeers) {
    PendingLayout L{};
    if (n > 0xFFFFFFFFull || m > 0xFFFFFFFFull || npeers > 0xFFFFFFFFull) return L; // total = 0
    WorkspaceCursor ws;
    L.words = ws.take(npeers * 4);
    L.agg.take_agg(ws, npeers, 8);
    L.total = ws.total();
    return L;
}

} // namespace
} // namespace rg

using namespace rg::host;

namespace {
// the struct's rules (include/rg_aead.h), answered without a look at the device; RG_OK with the kernels' view in *out
int check_tables(const char *what, const rg_pending_tables *t, rg::Tables *out) {
    if (!t) return bad(what, "bad args");
    if (!t->pend_table || (t->npeers && (!t->pending || !t->timers || !t->hs_ids)))
        return bad(what, "a null array in the tables");
    if (!pow2(t->pend_cap) || (uint64_t)t->pend_cap < 2ull * t->npeers)
        return bad(what, "pend_cap must be a power of two >= 2 npeers");
    if (misaligned(t->pending, 16) || misaligned(t->timers, 8) || misaligned(t->pend_table, 8) ||
        misaligned(t->hs_ids, 4))
        return bad(what, "pending must be 16-byte, timers and pend_table 8-byte and hs_ids 4-byte aligned");
    out->pending = reinterpret_cast<uint4 *>(t->pending);
    out->timers = reinterpret_cast<uint64_t *>(t->timers);
    out->hs_ids = t->hs_ids;
    out->pend_table = reinterpret_cast<unsigned long long *>(t->pend_table);
    out->npeers = t->npeers;
    out->pend_cap = t->pend_cap;
    return RG_OK;
}

// one lane per peer or table entry, whichever are more
dim3 clear_grid(const rg::Tables &t) { return lanes(std::max<uint64_t>({t.npeers, t.pend_cap, 1})); }

void launch_index(const rg::Tables &t, hipStream_t st) {
    if (t.npeers) hipLaunchKernelGGL(rg::pend_index_kernel, lanes(t.npeers), kWg, 0, st, t);
}
} // namespace

extern "C" size_t rg_pending_workspace_size(size_t n, size_t m, uint32_t npeers) {
    return (size_t)rg::pending_layout(n, m, npeers).total;
}

extern "C" int rg_pending_index_dev(rg_ctx *ctx, const rg_pending_tables *tables, void *stream) {
    const char *what = "pending index";
    if (!ctx) return set_err(RG_EINVAL, "null context");
    rg::Tables t{};
    int rc = check_tables(what, tables, &t);
    if (rc) return rc;
    rg::DeviceGuard dg_;
    rc = check_ctx(ctx);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rg::pend_fill_kernel, lanes(t.pend_cap), kWg, 0, st, t);
    launch_index(t, st);
    RG_HIP(hipGetLastError(), what);
    return RG_OK;
}

extern "C" int rg_pending_install_batch_dev(rg_ctx *ctx, const rg_pending_tables *tables, rg_hs_pending *batch,
                                            const uint8_t *gate, size_t n, const uint64_t *now_ns, uint8_t *status,
                                            uint32_t *installed_out, void *workspace, size_t workspace_len,
                                            void *stream) {
    const char *what = "pending install";
    if (!ctx) return set_err(RG_EINVAL, "null context");
    if (n == 0) return RG_OK;
    if (!batch || !now_ns || !status || !installed_out || !workspace || n > 0xFFFFFFFFull) return bad(what, "bad args");
    rg::InstallArgs a{};
    int rc = check_tables(what, tables, &a.t);
    if (rc) return rc;
    if (misaligned(batch, 16) || misaligned(now_ns, 8) || misaligned(installed_out, 4))
        return bad(what, "batch must be 16-byte, now_ns 8-byte and installed_out 4-byte aligned");
    {
        const uintptr_t b0 = (uintptr_t)batch, b1 = b0 + n * sizeof(rg_hs_pending);
        const uintptr_t p0 = (uintptr_t)tables->pending, p1 = p0 + (uintptr_t)a.t.npeers * sizeof(rg_hs_pending);
        if (b0 < p1 && p0 < b1) return bad(what, "batch overlaps tables.pending");
    }
    const rg::PendingLayout L = rg::pending_layout(n, 0, a.t.npeers);
    rc = check_workspace(what, tables->timers, workspace, workspace_len, L.total);
    if (rc) return rc;
    rg::DeviceGuard dg_;
    rc = check_ctx(ctx);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    a.batch = reinterpret_cast<uint4 *>(batch);
    a.gate = gate;
    a.now_ns = now_ns;
    a.status = status;
    a.installed_out = installed_out;
    a.claim = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(workspace) + L.words);
    a.n = (uint32_t)n;
    hipLaunchKernelGGL(rg::install_clear_kernel, clear_grid(a.t), kWg, 0, st, a);
    hipLaunchKernelGGL(rg::install_claim_kernel, lanes(n), kWg, 0, st, a);
    if (a.t.npeers) hipLaunchKernelGGL(rg::install_commit_kernel, lanes((uint64_t)a.t.npeers * rg::kRowQuads), kWg, 0, st, a);
    hipLaunchKernelGGL(rg::install_wipe_kernel, lanes((uint64_t)n * rg::kRowQuads), kWg, 0, st, a);
    launch_index(a.t, st);
    RG_HIP(hipGetLastError(), what);
    return RG_OK;
}

extern "C" int rg_pending_turn_dev(rg_ctx *ctx, const rg_pending_tables *tables, const uint64_t *now_ns,
                                   const uint32_t *start_peers, const uint8_t *start_status, uint8_t start_match,
                                   size_t m, uint32_t *init_peers_out, uint8_t *init_gate_out, uint8_t *expired_out,
                                   uint32_t *counts_out, void *workspace, size_t workspace_len, void *stream) {
    const char *what = "pending turn";
    if (!ctx) return set_err(RG_EINVAL, "null context");
    if (!now_ns || !counts_out || !workspace || (m && !start_peers) || m > 0xFFFFFFFFull) return bad(what, "bad args");
    rg::TurnArgs a{};
    int rc = check_tables(what, tables, &a.t);
    if (rc) return rc;
    if (a.t.npeers && (!init_peers_out || !init_gate_out)) return bad(what, "a null output array");
    if (misaligned(now_ns, 8) || misaligned(start_peers, 4) || misaligned(init_peers_out, 4) ||
        misaligned(counts_out, 4))
        return bad(what, "now_ns must be 8-byte and the word arrays 4-byte aligned");
    const rg::PendingLayout L = rg::pending_layout(0, m, a.t.npeers);
    rc = check_workspace(what, tables->timers, workspace, workspace_len, L.total);
    if (rc) return rc;
    rg::DeviceGuard dg_;
    rc = check_ctx(ctx);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    a.now_ns = now_ns;
    a.start_peers = start_peers;
    a.start_status = start_status;
    a.start_match = start_match;
    a.m = (uint32_t)m;
    a.want = reinterpret_cast<uint32_t *>(ws + L.words);
    a.init_peers_out = init_peers_out;
    a.init_gate_out = init_gate_out;
    a.expired_out = expired_out;
    a.counts_out = counts_out;
    hipLaunchKernelGGL(rg::turn_clear_kernel, clear_grid(a.t), kWg, 0, st, a);
    if (a.t.npeers) {
        hipLaunchKernelGGL(rg::turn_row_kernel, lanes(a.t.npeers), kWg, 0, st, a);
        if (a.m) hipLaunchKernelGGL(rg::turn_request_kernel, lanes(a.m), kWg, 0, st, a);
        const rg::PendWants wants{a};
        rg::compact(wants, wants, a.t.npeers, rg::Agg<uint64_t>(ws, L.agg), st);
        launch_index(a.t, st);
    }
    RG_HIP(hipGetLastError(), what);
    return RG_OK;
}
