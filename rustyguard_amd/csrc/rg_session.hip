// rg_session.hip -- the session table of the resident transport calls kept on the device: finished handshakes
// become live rows of the caller's tables on the stream that produced them, and sessions past their lifetime
// leave them the same way.  The reference does this at the tail of handle_handshake_init
// (rustyguard-core/src/handshake.rs:110-133), at the tail of handle_handshake_resp (:201-227) and in the
// ExpireTransport timer (rustyguard-core/src/time.rs:84-98).
//
//   rg_session_install_batch_dev         (gate, local id, remote id, peer, key row) per handshake -> rows
//   rg_session_install_resp_batch_dev    the same behind rg_handshake_resp_batch_dev's outputs
//   rg_session_install_finish_batch_dev  the same behind rg_handshake_finish_batch_dev's outputs
//   rg_session_expire_batch_dev          REJECT_AFTER_TIME and an explicit list of rows
//   rg_session_index_dev                 the receiver table over the live rows, alone
//
// The install equals an in-order loop (include/rg_aead.h has it) and is computed with nothing decided by the
// order the lanes arrive in.  Kernels of that call, all on its stream:
//   prep      one lane per handshake: the gather of the wrapper, the gate, the peer bound, the duplicate check
//             against the live rows (a read of the receiver table as it stands); every row that passes enters
//             the batch's (id -> lowest index) table, an atomicMin of (id << 32 | index) per slot
//   compact   rg_grouped.h's count / carry / rank over the batch.  InstallJudge (the count walk): the lowest index
//             of an id is eligible, the others are duplicates.  InstallRank (the rank walk): every eligible row's
//             rank among the eligible rows
//   compact   the same over the table, FreeRows in both walks: free_list[k] = the k-th free row, ascending
//   commit    one lane per handshake: row = free_list[rank] or RG_PKT_FULL; the row's nine fields; the key row
//             zeroed; atomicMax(claim[peer], i + 1)
//   peer_commit  one lane per peer: peer_slot = the row of its highest installed index
//   index     memset 0xFF, then one lane per live row claims the first empty entry from its home slot by a
//             64-bit atomicCAS.  Which of two colliding rows gets the earlier entry depends on arrival; what
//             rx_find answers does not.
// Once the free rows run out every later eligible row is RG_PKT_FULL, so an id's first eligible holder is known
// without knowing who got a row, and one round suffices.
//
// The entry points' host side is here too (rg_peerstate.hip's precedent), on rg_host.h like the host units, none
// of which names a launcher of this file.  All scratch is the caller's; nothing is allocated, waited for or kept
// in the context.
#include "rg_host.h"
#include "rg_grouped.h"
#include "rg_rxclaim.h"

namespace rg {
namespace {

constexpr uint64_t kEmpty64 = ~0ull; // a free entry of the id table
constexpr uint32_t kWindowWords = sizeof(rg_antireplay) / 8;
constexpr uint64_t kRejectAfterNs = RG_REJECT_AFTER_TIME_NS;

// rg_session_tables as the kernels take it
struct Tables {
    uint4 *send_keys, *recv_keys; // [nkeys][2]
    uint32_t *receivers, *local_ids, *slot_peer;
    uint64_t *windows;    // [nkeys][kWindowWords]
    uint64_t *send_state; // [nkeys][3]
    unsigned long long *rx_table; // [rx_cap] receiver | key_idx << 32
    uint32_t *peer_slot;
    uint32_t nkeys, rx_cap, npeers;
};

struct SessionLayout {
    uint64_t lid, rid, peer; // [n] u32 each: the gathered ids and peer of a row that entered the id table
    uint64_t rank;           // [n] u32: prep's mark, judge's 0 / 1, then the rank among the eligible rows
    uint64_t ids;            // [ids_cap] u64: id << 32 | lowest index
    AggLayout agg_n;         // u32 counts of the batch's tiles
    AggLayout agg_k;         // of the table's tiles
    uint64_t free_list;      // [nkeys] u32
    uint64_t claim;          // [npeers] u32
    uint64_t mark;           // [nkeys] u8: rows an expire call names
    uint64_t total;
    uint64_t ids_cap; // a power of two >= 2 n, at most 2^32
};
SessionLayout session_layout(uint64_t n, uint32_t nkeys, uint32_t npeers) {
    SessionLayout L{};
    if (n > 0xFFFFFFFFull) return L; // total = 0
    WorkspaceCursor ws;
    L.ids_cap = 64;
    while (L.ids_cap < 2 * n && L.ids_cap < (1ull << 32)) L.ids_cap <<= 1;
    L.lid = ws.take(n * 4);
    L.rid = ws.take(n * 4);
    L.peer = ws.take(n * 4);
    L.rank = ws.take(n * 4);
    L.ids = ws.take(L.ids_cap * 8);
    L.agg_n.take_agg(ws, n, 4);
    L.agg_k.take_agg(ws, nkeys, 4);
    L.free_list = ws.take((uint64_t)nkeys * 4);
    L.claim = ws.take((uint64_t)npeers * 4);
    L.mark = ws.take(nkeys);
    L.total = ws.total();
    return L;
}

// where a handshake's fields come from: the arrays themselves, or one of the handshake calls' outputs
enum : uint32_t { kDirect = 0, kResp = 1, kFinish = 2 };
struct InstallArgs {
    Tables t;
    uint32_t mode;
    const uint8_t *gate;       // [n] or nullptr
    const uint32_t *local_ids; // [n]; kResp: session_ids; kFinish: pend_session_ids [npending]
    const uint32_t *remote_ids; // [n]; kFinish: remote_out
    const uint32_t *peers;     // [n]; kFinish: pend_peers [npending]
    const uint4 *results;      // kResp: [n] rg_hs_init_result rows of 8 uint4 (peer: quad 6 .w, sender: quad 7 .x)
    const uint32_t *pend_idx;  // kFinish: [n]
    uint32_t npending;
    uint4 *keys; // [n][4]: send key || receive key
    const uint64_t *now_ns;
    uint8_t *status;
    uint32_t *rows_out;
    uint32_t *lid, *rid, *peer, *rank;
    unsigned long long *ids;
    uint64_t ids_mask;
    uint32_t ids_shift;
    uint32_t *free_list, *claim;
    uint32_t n;
};

constexpr uint32_t kCandidate = 1u; // rank[i] after prep: the row entered the id table (0: it has its answer)

__device__ __forceinline__ void zero_key_row(uint4 *row) {
#pragma unroll
    for (int q = 0; q < 4; ++q) row[q] = make_uint4(0, 0, 0, 0);
}

__device__ __forceinline__ uint64_t ids_home(const InstallArgs &a, uint32_t id) {
    return (uint64_t)((id * 0x9E3779B1u) >> a.ids_shift) & a.ids_mask;
}
// An entry is id << 32 | the lowest index that brought the id.  Once taken, an entry's id never changes.  The
// table has at least as many entries as the batch has rows (two per row below 2^31 rows): a probe ends.
__device__ __forceinline__ void ids_insert(const InstallArgs &a, uint32_t id, uint32_t i) {
    const unsigned long long mine = ((unsigned long long)id << 32) | i; // never kEmpty64: i <= 2^32 - 2
    uint64_t s = ids_home(a, id);
    for (uint64_t probe = 0; probe <= a.ids_mask; ++probe, s = (s + 1) & a.ids_mask) {
        const unsigned long long e = atomicCAS(&a.ids[s], kEmpty64, mine);
        if (e == kEmpty64) return;
        if ((uint32_t)(e >> 32) == id) {
            atomicMin(&a.ids[s], mine); // the minimum is the same whatever order the lanes arrive in
            return;
        }
    }
}
__device__ __forceinline__ uint32_t ids_first(const InstallArgs &a, uint32_t id) {
    uint64_t s = ids_home(a, id);
    for (uint64_t probe = 0; probe <= a.ids_mask; ++probe, s = (s + 1) & a.ids_mask) {
        const unsigned long long e = a.ids[s];
        if (e == kEmpty64) break;
        if ((uint32_t)(e >> 32) == id) return (uint32_t)e;
    }
    return RG_KEY_SKIP;
}

__global__ __launch_bounds__(256) void install_prep_kernel(InstallArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    a.rows_out[i] = RG_KEY_SKIP;
    a.rank[i] = 0;
    if (a.gate && a.gate[i] != RG_PKT_OK) {
        a.status[i] = RG_PKT_REJECTED; // nothing else of the row is read or written
        return;
    }
    uint32_t lid = 0, rid = 0, peer = RG_PEER_NONE;
    bool valid = true;
    if (a.mode == kResp) {
        lid = a.local_ids[i];
        peer = a.results[8ull * i + 6].w;
        rid = a.results[8ull * i + 7].x;
    } else if (a.mode == kFinish) {
        const uint32_t pi = a.pend_idx[i];
        valid = pi < a.npending;
        if (valid) {
            lid = a.local_ids[pi];
            peer = a.peers[pi];
        }
        rid = a.remote_ids[i];
    } else {
        lid = a.local_ids[i];
        rid = a.remote_ids[i];
        peer = a.peers[i];
    }
    uint8_t st = RG_PKT_PENDING;
    if (!valid || peer >= a.t.npeers) st = RG_PKT_INVALID;
    else if (rx_find(reinterpret_cast<const rg_rx_entry *>(a.t.rx_table), a.t.rx_cap, lid) != RG_KEY_SKIP)
        st = RG_PKT_REJECTED; // the id of a live row
    if (st != RG_PKT_PENDING) {
        zero_key_row(a.keys + 4ull * i); // a key row is consumed once, whatever follows
        a.status[i] = st;
        return;
    }
    a.lid[i] = lid;
    a.rid[i] = rid;
    a.peer[i] = peer;
    a.rank[i] = kCandidate;
    ids_insert(a, lid, i);
}

// The two passes of rg_grouped.h's compact over the batch.  The count walk judges: the first holder of an id is
// eligible (1), a later one a duplicate, answered here (0); rank[i] keeps the verdict.
struct InstallJudge {
    InstallArgs a;
    __device__ __forceinline__ uint32_t item(uint64_t pos) const {
        const uint32_t i = (uint32_t)pos;
        uint32_t e = 0;
        if (a.rank[i] == kCandidate) {
            if (ids_first(a, a.lid[i]) == i) e = 1;
            else {
                zero_key_row(a.keys + 4ull * i);
                a.status[i] = RG_PKT_REJECTED; // a duplicate of an earlier row of the batch
            }
        }
        a.rank[i] = e;
        return e;
    }
};
// The rank walk reads that verdict: rank[i] = the row's rank among the eligible rows, or RG_KEY_SKIP.
struct InstallRank {
    uint32_t *rank;
    __device__ __forceinline__ uint32_t item(uint64_t pos) const { return rank[pos]; }
    __device__ __forceinline__ void emit(uint64_t pos, uint32_t e, uint32_t ex) const {
        rank[pos] = e ? ex : RG_KEY_SKIP;
    }
    __device__ __forceinline__ void total(uint32_t) const {}
};
// The pass over the table: free_list[k] = the k-th free row, ascending (the entries behind the last stay
// RG_KEY_SKIP).
struct FreeRows {
    const uint32_t *slot_peer;
    uint32_t *free_list;
    uint32_t nkeys;
    __device__ __forceinline__ uint32_t item(uint64_t pos) const { return slot_peer[pos] == RG_PEER_NONE; }
    __device__ __forceinline__ void emit(uint64_t pos, uint32_t f, uint32_t ex) const {
        if (f && ex < nkeys) free_list[ex] = (uint32_t)pos;
    }
    __device__ __forceinline__ void total(uint32_t) const {}
};

// What a row that changes hands holds: the given keys and birth time, no packet sent, none seen.
__device__ __forceinline__ void reset_row(const Tables &t, uint32_t r, uint4 k0, uint4 k1, uint4 k2, uint4 k3,
                                          uint64_t born) {
    t.send_keys[2ull * r] = k0;
    t.send_keys[2ull * r + 1] = k1;
    t.recv_keys[2ull * r] = k2;
    t.recv_keys[2ull * r + 1] = k3;
    uint64_t *w = t.windows + (uint64_t)kWindowWords * r;
    for (uint32_t q = 0; q < kWindowWords; ++q) w[q] = 0;
    uint64_t *s = t.send_state + 3ull * r;
    s[0] = 0;
    s[1] = born;
    s[2] = born;
}

__global__ __launch_bounds__(256) void install_commit_kernel(InstallArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t rk = a.rank[i];
    if (rk == RG_KEY_SKIP) return; // answered by prep or judge
    uint4 *key = a.keys + 4ull * i;
    const uint32_t r = rk < a.t.nkeys ? a.free_list[rk] : RG_KEY_SKIP;
    const uint32_t peer = a.peer[i];
    if (r >= a.t.nkeys || peer >= a.t.npeers) { // the free rows ran out
        zero_key_row(key);
        a.status[i] = RG_PKT_FULL;
        return;
    }
    const uint4 k0 = key[0], k1 = key[1], k2 = key[2], k3 = key[3];
    zero_key_row(key);
    reset_row(a.t, r, k0, k1, k2, k3, a.now_ns ? *a.now_ns : 0);
    a.t.receivers[r] = a.rid[i];
    a.t.local_ids[r] = a.lid[i];
    a.t.slot_peer[r] = peer;
    atomicMax(&a.claim[peer], i + 1); // peer.current_transport: the last one in array order
    a.rows_out[i] = r;
    a.status[i] = RG_PKT_OK; // after the row
}

__global__ __launch_bounds__(256) void peer_commit_kernel(InstallArgs a) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.t.npeers) return;
    const uint32_t c = a.claim[p];
    if (c == 0 || c > a.n) return; // no handshake of this peer got a row
    const uint32_t r = a.rows_out[c - 1];
    if (r < a.t.nkeys) a.t.peer_slot[p] = r;
}

// ------------------------------------------------------ the receiver table
__global__ __launch_bounds__(256) void index_kernel(Tables t) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= t.nkeys || t.slot_peer[r] == RG_PEER_NONE) return;
    rx_claim(t.rx_table, t.rx_cap, t.local_ids[r], r);
}

// ------------------------------------------------------------------ expiry
struct ExpireArgs {
    Tables t;
    const uint64_t *now_ns; // or nullptr
    const uint32_t *rows;   // [m] or nullptr
    uint32_t m;
    uint8_t *mark;        // [nkeys], 0 before the call; nullptr without rows
    uint8_t *expired_out; // [nkeys] or nullptr
};
__global__ __launch_bounds__(256) void expire_mark_kernel(ExpireArgs a) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.m) return;
    const uint32_t r = a.rows[j];
    if (r < a.t.nkeys) a.mark[r] = 1; // the same value from every lane that names the row
}
__global__ __launch_bounds__(256) void expire_kernel(ExpireArgs a) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.t.nkeys) return;
    const uint32_t p = a.t.slot_peer[r];
    bool gone = false;
    if (p != RG_PEER_NONE) {
        if (a.now_ns) gone = a.t.send_state[3ull * r + 1] + kRejectAfterNs < *a.now_ns; // should_expire: wrapping, strict
        if (a.mark && a.mark[r]) gone = true;
    }
    if (gone) {
        const uint4 z = make_uint4(0, 0, 0, 0);
        reset_row(a.t, r, z, z, z, z, 0);
        a.t.receivers[r] = 0;
        a.t.local_ids[r] = 0;
        // only this lane can find r there: a newer session of the peer stays its current one (time.rs:93-95)
        if (p < a.t.npeers && a.t.peer_slot[p] == r) a.t.peer_slot[p] = RG_KEY_SKIP;
        a.t.slot_peer[r] = RG_PEER_NONE;
    }
    if (a.expired_out) a.expired_out[r] = gone ? 1 : 0;
}

} // namespace
} // namespace rg

using namespace rg::host;

namespace {
// the struct's rules (include/rg_aead.h); RG_OK with the kernels' view in *out
int check_tables(const char *what, const rg_session_tables *t, rg::Tables *out) {
    if (!t) return bad(what, "bad args");
    if (!t->rx_table || (t->npeers && !t->peer_slot) ||
        (t->nkeys && (!t->send_keys || !t->recv_keys || !t->receivers || !t->local_ids || !t->slot_peer ||
                      !t->windows || !t->send_state)))
        return bad(what, "a null array in the tables");
    if (t->rx_cap == 0 || (t->rx_cap & (t->rx_cap - 1)) != 0 || (uint64_t)t->rx_cap < 2ull * t->nkeys)
        return bad(what, "rx_cap must be a power of two >= 2 nkeys");
    if (misaligned(t->send_keys, 16) || misaligned(t->recv_keys, 16) || misaligned(t->windows, 8) ||
        misaligned(t->send_state, 8) || misaligned(t->rx_table, 8) || misaligned(t->receivers, 4) ||
        misaligned(t->local_ids, 4) || misaligned(t->slot_peer, 4) || misaligned(t->peer_slot, 4))
        return bad(what, "the key tables must be 16-byte, windows, send_state and rx_table 8-byte and the word "
                         "arrays 4-byte aligned");
    out->send_keys = reinterpret_cast<uint4 *>(t->send_keys);
    out->recv_keys = reinterpret_cast<uint4 *>(t->recv_keys);
    out->receivers = t->receivers;
    out->local_ids = t->local_ids;
    out->slot_peer = t->slot_peer;
    out->windows = reinterpret_cast<uint64_t *>(t->windows);
    out->send_state = reinterpret_cast<uint64_t *>(t->send_state);
    out->rx_table = reinterpret_cast<unsigned long long *>(t->rx_table);
    out->peer_slot = t->peer_slot;
    out->nkeys = t->nkeys;
    out->rx_cap = t->rx_cap;
    out->npeers = t->npeers;
    return RG_OK;
}

int launch_index(const char *what, const rg::Tables &t, hipStream_t st) {
    RG_HIP(hipMemsetAsync(t.rx_table, 0xFF, (size_t)t.rx_cap * sizeof(rg_rx_entry), st), what);
    if (t.nkeys) {
        hipLaunchKernelGGL(rg::index_kernel, lanes(t.nkeys), kWg, 0, st, t);
        RG_HIP(hipGetLastError(), what);
    }
    return RG_OK;
}

// the three install entry points behind their gathers: a carries mode and the gathered arrays
int install(const char *what, rg_ctx *ctx, const rg_session_tables *tables, rg::InstallArgs a, uint8_t *transport_keys,
            size_t n, const uint64_t *now_ns, uint8_t *status, uint32_t *rows_out, void *workspace,
            size_t workspace_len, void *stream, bool args_ok) {
    rg::DeviceGuard dg_;
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!args_ok || !transport_keys || !status || !rows_out || !workspace || n > 0xFFFFFFFFull) return bad(what, "bad args");
    rc = check_tables(what, tables, &a.t);
    if (rc) return rc;
    if (misaligned(transport_keys, 16) || misaligned(rows_out, 4) || misaligned(now_ns, 8) ||
        misaligned(a.local_ids, 4) || misaligned(a.remote_ids, 4) || misaligned(a.peers, 4) ||
        misaligned(a.results, 16) || misaligned(a.pend_idx, 4))
        return bad(what, "transport_keys and results must be 16-byte, now_ns 8-byte and the word arrays 4-byte aligned");
    const rg::SessionLayout L = rg::session_layout(n, a.t.nkeys, a.t.npeers);
    rc = check_workspace(what, tables->windows, workspace, workspace_len, L.total);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    auto words = [&](uint64_t off) { return reinterpret_cast<uint32_t *>(ws + off); };
    a.keys = reinterpret_cast<uint4 *>(transport_keys);
    a.now_ns = now_ns;
    a.status = status;
    a.rows_out = rows_out;
    a.lid = words(L.lid);
    a.rid = words(L.rid);
    a.peer = words(L.peer);
    a.rank = words(L.rank);
    a.ids = reinterpret_cast<unsigned long long *>(ws + L.ids);
    a.ids_mask = L.ids_cap - 1;
    a.ids_shift = 32 - (uint32_t)__builtin_ctzll(L.ids_cap);
    a.free_list = words(L.free_list);
    a.claim = words(L.claim);
    a.n = (uint32_t)n;
    RG_HIP(hipMemsetAsync(status, RG_PKT_PENDING, n, st), what); // a call that never ran reads as unfinished
    RG_HIP(hipMemsetAsync(a.ids, 0xFF, (size_t)L.ids_cap * 8, st), what);
    if (a.t.nkeys) RG_HIP(hipMemsetAsync(a.free_list, 0xFF, (size_t)a.t.nkeys * 4, st), what);
    if (a.t.npeers) RG_HIP(hipMemsetAsync(a.claim, 0, (size_t)a.t.npeers * 4, st), what);
    hipLaunchKernelGGL(rg::install_prep_kernel, lanes(n), kWg, 0, st, a);
    rg::compact(rg::InstallJudge{a}, rg::InstallRank{a.rank}, a.n, rg::Agg<uint32_t>(ws, L.agg_n), st);
    if (a.t.nkeys) {
        const rg::FreeRows rows{a.t.slot_peer, a.free_list, a.t.nkeys};
        rg::compact(rows, rows, a.t.nkeys, rg::Agg<uint32_t>(ws, L.agg_k), st);
    }
    hipLaunchKernelGGL(rg::install_commit_kernel, lanes(n), kWg, 0, st, a);
    if (a.t.npeers) hipLaunchKernelGGL(rg::peer_commit_kernel, lanes(a.t.npeers), kWg, 0, st, a);
    RG_HIP(hipGetLastError(), what);
    return launch_index(what, a.t, st);
}
} // namespace

extern "C" size_t rg_session_workspace_size(size_t n, uint32_t nkeys, uint32_t npeers) {
    return (size_t)rg::session_layout(n, nkeys, npeers).total;
}

extern "C" int rg_session_install_batch_dev(rg_ctx *ctx, const rg_session_tables *tables, const uint8_t *gate,
                                            const uint32_t *local_ids, const uint32_t *remote_ids,
                                            const uint32_t *peers, uint8_t *transport_keys, size_t n,
                                            const uint64_t *now_ns, uint8_t *status, uint32_t *rows_out,
                                            void *workspace, size_t workspace_len, void *stream) {
    rg::InstallArgs a{};
    a.mode = rg::kDirect;
    a.gate = gate;
    a.local_ids = local_ids;
    a.remote_ids = remote_ids;
    a.peers = peers;
    return install("session install", ctx, tables, a, transport_keys, n, now_ns, status, rows_out, workspace,
                   workspace_len, stream, local_ids && remote_ids && peers);
}

extern "C" int rg_session_install_resp_batch_dev(rg_ctx *ctx, const rg_session_tables *tables, const uint8_t *gate,
                                                 const uint32_t *session_ids, const rg_hs_init_result *results,
                                                 uint8_t *transport_keys, size_t n, const uint64_t *now_ns,
                                                 uint8_t *status, uint32_t *rows_out, void *workspace,
                                                 size_t workspace_len, void *stream) {
    rg::InstallArgs a{};
    a.mode = rg::kResp;
    a.gate = gate;
    a.local_ids = session_ids;
    a.results = reinterpret_cast<const uint4 *>(results);
    return install("session install resp", ctx, tables, a, transport_keys, n, now_ns, status, rows_out, workspace,
                   workspace_len, stream, session_ids && results);
}

extern "C" int rg_session_install_finish_batch_dev(rg_ctx *ctx, const rg_session_tables *tables, const uint8_t *gate,
                                                   const uint32_t *pend_idx_out, const uint32_t *remote_out,
                                                   const uint32_t *pend_session_ids, const uint32_t *pend_peers,
                                                   uint32_t npending, uint8_t *transport_keys, size_t n,
                                                   const uint64_t *now_ns, uint8_t *status, uint32_t *rows_out,
                                                   void *workspace, size_t workspace_len, void *stream) {
    rg::InstallArgs a{};
    a.mode = rg::kFinish;
    a.gate = gate;
    a.pend_idx = pend_idx_out;
    a.remote_ids = remote_out;
    a.local_ids = pend_session_ids;
    a.peers = pend_peers;
    a.npending = npending;
    return install("session install finish", ctx, tables, a, transport_keys, n, now_ns, status, rows_out, workspace,
                   workspace_len, stream, pend_idx_out && remote_out && (!npending || (pend_session_ids && pend_peers)));
}

extern "C" int rg_session_expire_batch_dev(rg_ctx *ctx, const rg_session_tables *tables, const uint64_t *now_ns,
                                           const uint32_t *rows, size_t m, uint8_t *expired_out, void *workspace,
                                           size_t workspace_len, void *stream) {
    const char *what = "session expire";
    rg::DeviceGuard dg_;
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if (!workspace || (m && !rows) || m > 0xFFFFFFFFull) return bad(what, "bad args");
    rg::ExpireArgs a{};
    rc = check_tables(what, tables, &a.t);
    if (rc) return rc;
    if (misaligned(now_ns, 8) || misaligned(rows, 4)) return bad(what, "now_ns must be 8-byte and rows 4-byte aligned");
    const rg::SessionLayout L = rg::session_layout(0, a.t.nkeys, a.t.npeers);
    rc = check_workspace(what, tables->windows, workspace, workspace_len, L.total);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    a.now_ns = now_ns;
    a.expired_out = expired_out;
    if (m && a.t.nkeys) {
        a.rows = rows;
        a.m = (uint32_t)m;
        a.mark = static_cast<uint8_t *>(workspace) + L.mark;
        RG_HIP(hipMemsetAsync(a.mark, 0, a.t.nkeys, st), what);
        hipLaunchKernelGGL(rg::expire_mark_kernel, lanes(m), kWg, 0, st, a);
    }
    if (a.t.nkeys) hipLaunchKernelGGL(rg::expire_kernel, lanes(a.t.nkeys), kWg, 0, st, a);
    RG_HIP(hipGetLastError(), what);
    return launch_index(what, a.t, st);
}

extern "C" int rg_session_index_dev(rg_ctx *ctx, const rg_session_tables *tables, void *stream) {
    const char *what = "session index";
    rg::DeviceGuard dg_;
    int rc = check_ctx(ctx);
    if (rc) return rc;
    rg::Tables t{};
    rc = check_tables(what, tables, &t);
    if (rc) return rc;
    return launch_index(what, t, (hipStream_t)stream);
}
