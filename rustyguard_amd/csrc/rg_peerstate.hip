// rg_peerstate.hip -- the three per-peer fields the reference keeps in Peer (rustyguard-core/src/lib.rs:170-180)
// as a device table of rg_hs_peer_state rows, and the four batch calls that read and write it, so that neither
// the responder chain nor the initiator's cookie loop goes back to the host between handshake calls:
//
//   rg_peer_ts_batch_dev              latest_ts: the in-order timestamp-replay check of handle_handshake_init
//                                     (handshake.rs:88-91) behind rg_handshake_init_batch_dev
//   rg_peer_cookie_consume_batch_dev  cookie: handle_cookie / decrypt_cookie (handshake.rs:233-257) for a batch of
//                                     CookieMessages
//   rg_peer_cookies_batch_dev         cookie -> the cookies / has_cookie arrays the initiate and response calls take
//   rg_peer_mac1_batch_dev            last_sent_mac1: the mac1 field of what was just sent (handshake.rs:108 and
//                                     new_handshake), the AAD of the next cookie reply
//
// The timestamp check is sequential per peer: `if ts < latest { reject } else { latest = ts }`.  Whether or not a
// row is accepted, latest after it is max(latest, ts), so row i is accepted iff
//   ts_i >= max(latest at the start, ts_j of the eligible rows j < i of the same peer)
// a segmented exclusive prefix maximum in the stable grouped order, and the peer's last row leaves
// max(latest, the group's maximum) behind.  Kernels of that call, all on its stream:
//   ts_prep      rows[i] = the peer of an eligible row (status OK, peer < npeers), RG_KEY_SKIP otherwise; every
//                other row gets its final answer here (an OK row without a peer row: RG_PKT_INVALID, wiped)
//   radix_hist / radix_scan / radix_scatter   rg_grouped.h: the stable grouping by peer
//   seg_reduce / carry / seg_verdict   rg_grouped.h's segscan with TsArgs as its pass: per workgroup of 2048 grouped
//                rows the aggregate of the segmented prefix maximum, the tiles' carries, then every eligible row's
//                prefix maximum and verdict (judge) and the running maximum at each peer's last row (tail)
//   ts_advance   one lane per peer with traffic: latest_ts
// The value is the 96-bit timestamp as an integer, big-endian as TAI64N orders it, in an unsigned __int128; zero
// is the identity (a zeroed row is Peer::new, and no timestamp is below it).  A row without a peer rides along
// in peer 0's group as that identity and is not judged.  No atomic decides anything by arrival order.
//
// The cookie and the mac1 are "last writer wins" in the reference's loop: the highest message index per peer,
// by atomicMax into a claim word per peer and a commit launch over the peers, the mirror of the finish call's
// atomicMin (rg_handshake.hip).
//
// The entry points' host side is here too (rg_cookie.hip's precedent), on rg_host.h like the host units, none
// of which names a launcher of this file.  All scratch is the caller's; nothing is allocated, waited for or
// kept in the context.
#include "rg_host.h"
#include "rg_grouped.h"
#include "rg_noise.h"

namespace rg {
namespace {

// rg_hs_peer_state as 4 uint4: (latest_ts[0..12], has_cookie), cookie, last_sent_mac1, pad
constexpr uint32_t kStateQuads = 4;

// ------------------------------------------------------------- timestamps
using Ts = unsigned __int128; // be64(ts[0..8]) << 32 | be32(ts[8..12])
struct TsMax {
    __device__ __forceinline__ Ts operator()(Ts a, Ts b) const { return a > b ? a : b; }
};

// the 12 bytes as they lie in memory (three little-endian words) -> their big-endian value, and back
__device__ __forceinline__ Ts ts_value(uint32_t w0, uint32_t w1, uint32_t w2) {
    const uint64_t hi = ((uint64_t)__builtin_bswap32(w0) << 32) | __builtin_bswap32(w1);
    return ((Ts)hi << 32) | __builtin_bswap32(w2);
}

struct TsLayout {
    uint64_t rows; // [n] u32: the peer of an eligible row, RG_KEY_SKIP otherwise
    GroupLayout g; // the grouped order and the aggregates (Ts) of the segmented prefix maximum
    uint64_t lf;   // [n] Ts: the running maximum at each peer's last row
    uint64_t total;
};
TsLayout ts_layout(uint64_t n, uint32_t npeers) {
    TsLayout L{};
    if (n > 0xFFFFFFFFull) return L; // total = 0
    WorkspaceCursor ws;
    L.rows = ws.take(n * 4);
    L.g.take(ws, n, npeers, sizeof(Ts));
    L.lf = ws.take(n * sizeof(Ts));
    L.total = ws.total();
    return L;
}

// as the init call leaves the row of a message that failed: zeros, peer = RG_PEER_NONE
__device__ __forceinline__ void wipe_result(uint4 *row) {
#pragma unroll
    for (int q = 0; q < 8; ++q) row[q] = q == 6 ? make_uint4(0, 0, 0, RG_PEER_NONE) : make_uint4(0, 0, 0, 0);
}

// The call's arguments; the scan kernels take them as the pass of rg_grouped.h's segscan.
struct TsArgs {
    using Pair = SegPair<Ts, TsMax>;
    struct Item : SegItem {
        Ts ts; // 0 for a row that rides along
    };
    uint4 *state;        // [npeers] rg_hs_peer_state
    uint4 *results;      // [n] rg_hs_init_result rows of 8 uint4; word 3 of quad 6 is the peer
    uint8_t *status;     // [n]
    uint32_t *peers_out; // [n]
    uint32_t *rows;      // [n] workspace
    Ts *lf;              // [n] workspace
    uint32_t npeers;
    uint32_t n;
    GroupScan<Ts> g; // g.rows = rows

    __device__ __forceinline__ void load(Item &it) const {
        if (it.row) {
            const uint4 q = results[8ull * it.i + 6];
            it.ts = ts_value(q.x, q.y, q.z);
        }
    }
    __device__ __forceinline__ Ts value(const Item &it) const { return it.ts; }
    __device__ __forceinline__ void seen(const Item &) const {}
    // before = the peer's largest eligible timestamp ahead of this row
    __device__ __forceinline__ void judge(const Item &it, Ts before, Ts) const {
        if (!it.row) return;
        const uint4 s0 = state[(uint64_t)kStateQuads * it.key]; // read only here; ts_advance writes it
        const Ts latest = ts_value(s0.x, s0.y, s0.z);
        if (it.ts < (before > latest ? before : latest)) { // equal passes: the reference compares with <
            wipe_result(results + 8ull * it.i);
            peers_out[it.i] = RG_PEER_NONE;
            status[it.i] = RG_PKT_REJECTED; // after the row
        } else peers_out[it.i] = it.key;
    }
    // the peer's last row of the batch hands the running maximum to ts_advance
    __device__ __forceinline__ void tail(uint64_t pos, const Item &, Ts upto) const { lf[pos] = upto; }
};

__global__ __launch_bounds__(256) void ts_prep_kernel(TsArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    uint32_t row = RG_KEY_SKIP;
    if (a.status[i] == RG_PKT_OK) {
        const uint32_t peer = a.results[8ull * i + 6].w;
        if (peer < a.npeers) row = peer; // eligible: the scan's judge answers
        else {
            wipe_result(a.results + 8ull * i);
            a.peers_out[i] = RG_PEER_NONE;
            a.status[i] = RG_PKT_INVALID; // after the row
        }
    } else a.peers_out[i] = RG_PEER_NONE; // keeps its status
    a.rows[i] = row;
}

// One lane per peer with traffic (the lane of its last grouped row): latest_ts = max(latest_ts, the group's
// maximum).  A group without an eligible row has the maximum 0 and writes nothing.
__global__ __launch_bounds__(256) void ts_advance_kernel(TsArgs a) {
    const uint64_t pos = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (pos >= a.g.n) return;
    const uint32_t key = a.g.key_at(pos);
    if (!a.g.is_tail(pos, key) || key >= a.g.nrows) return;
    uint32_t *row = reinterpret_cast<uint32_t *>(a.state + (uint64_t)kStateQuads * key);
    const Ts latest = ts_value(row[0], row[1], row[2]), top = a.lf[pos];
    if (top <= latest) return;
    const uint64_t hi = (uint64_t)(top >> 32);
    row[0] = __builtin_bswap32((uint32_t)(hi >> 32));
    row[1] = __builtin_bswap32((uint32_t)hi);
    row[2] = __builtin_bswap32((uint32_t)top);
}

// ------------------------------------------------------------------ cookies
struct ConsumeArgs {
    uint4 *state;
    uint32_t npeers;
    const uint32_t *keys;     // [npeers][8] LE words: cookie_key(peer public key)
    const rg_rx_entry *table; // [cap]: receiver id -> peer row
    uint32_t cap;
    const rg_pkt_desc *desc;
    const uint8_t *gate; // [n] or nullptr
    const uint8_t *buf;
    uint64_t buf_len;
    uint32_t *cookies_out; // [n][4]
    uint32_t *claim;       // [npeers], 0 before the call: 1 + the highest message index that opened
    uint8_t *status;
    uint32_t n;
};

// decrypt_cookie for one message per lane: the open of rg_cookie.hip's seal, out of place
__global__ __launch_bounds__(256) void cookie_consume_kernel(ConsumeArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const rg_pkt_desc d = a.desc[i];
    uint32_t cookie[4] = {0, 0, 0, 0}, peer = RG_PEER_NONE;
    uint32_t st = frame_verdict(d, a.gate ? a.gate[i] : (uint32_t)RG_PKT_OK, a.buf_len, kCookieLen);
    if (st == kGoing) {
        const uint4 *mp = reinterpret_cast<const uint4 *>(a.buf + d.offset);
        const uint4 m0 = mp[0]; // type, receiver, nonce[0..8]
        if (m0.x != 3u) st = RG_PKT_INVALID; // Error::InvalidMessage
        else if ((peer = rx_find(a.table, a.cap, m0.y)) == RG_KEY_SKIP) st = RG_PKT_REJECTED;
        else if (peer >= a.npeers) st = RG_PKT_INVALID;
        else {
            const uint4 m1 = mp[1], ct = mp[2], tg = mp[3];
            const uint4 mac1 = a.state[(uint64_t)kStateQuads * peer + 2]; // the AAD: last_sent_mac1
            const uint32_t nonce[6] = {m0.z, m0.w, m1.x, m1.y, m1.z, m1.w}, theirs[4] = {tg.x, tg.y, tg.z, tg.w};
            uint32_t tag[4];
            const uint4 pt = cookie_aead(load_key(a.keys, peer), nonce, mac1, ct, false, tag);
            const bool ok = tag_diff(tag, theirs) == 0; // no early exit
            cookie[0] = ok ? pt.x : 0u;
            cookie[1] = ok ? pt.y : 0u;
            cookie[2] = ok ? pt.z : 0u;
            cookie[3] = ok ? pt.w : 0u;
            st = ok ? RG_PKT_OK : RG_PKT_DECRYPT_ERR;
        }
    }
    uint32_t *out = a.cookies_out + 4ull * i;
#pragma unroll
    for (int w = 0; w < 4; ++w) out[w] = cookie[w];
    a.status[i] = (uint8_t)st; // after the row
    if (st == RG_PKT_OK) atomicMax(&a.claim[peer], i + 1); // the maximum is the same whatever order the lanes arrive in
}

// "the last valid cookie stays" (the reference's in-order loop): one lane per peer takes the cookie of the
// highest message index that opened for it
__global__ __launch_bounds__(256) void cookie_commit_kernel(ConsumeArgs a) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.npeers) return;
    const uint32_t c = a.claim[p];
    if (c == 0 || c > a.n) return; // no valid message: the row stays byte for byte
    const uint32_t *ck = a.cookies_out + 4ull * (c - 1);
    uint4 *row = a.state + (uint64_t)kStateQuads * p;
    row[1] = make_uint4(ck[0], ck[1], ck[2], ck[3]);
    reinterpret_cast<uint32_t *>(row)[3] = 1u; // has_cookie, after the cookie
}

struct GatherArgs {
    const uint4 *state;
    uint32_t npeers;
    const uint32_t *peer_idx; // [n]
    uint32_t *cookies_out;    // [n][4]
    uint8_t *has_out;         // [n]
    uint32_t n;
};
__global__ __launch_bounds__(256) void cookie_gather_kernel(GatherArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t p = a.peer_idx[i];
    uint4 ck = make_uint4(0, 0, 0, 0);
    bool has = false;
    if (p < a.npeers) {
        const uint4 *row = a.state + (uint64_t)kStateQuads * p;
        has = row[0].w != 0;
        if (has) ck = row[1];
    }
    uint32_t *out = a.cookies_out + 4ull * i;
    out[0] = ck.x; out[1] = ck.y; out[2] = ck.z; out[3] = ck.w;
    a.has_out[i] = has ? 1 : 0;
}

// --------------------------------------------------------------------- mac1
struct Mac1Args {
    uint4 *state;
    uint32_t npeers;
    const uint32_t *peer_idx; // [n]
    const uint8_t *status;    // [n]
    const uint8_t *messages;  // [n] rows of `stride` bytes
    uint64_t stride;
    uint32_t mac1_offset;
    uint32_t *claim; // [npeers], 0 before the call: 1 + the highest sent row
    uint32_t n;
};
__global__ __launch_bounds__(256) void mac1_claim_kernel(Mac1Args a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n || a.status[i] != RG_PKT_OK) return;
    const uint32_t p = a.peer_idx[i];
    if (p < a.npeers) atomicMax(&a.claim[p], i + 1);
}
__global__ __launch_bounds__(256) void mac1_commit_kernel(Mac1Args a) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.npeers) return;
    const uint32_t c = a.claim[p];
    if (c == 0 || c > a.n) return;
    const uint8_t *m = a.messages + (uint64_t)(c - 1) * a.stride + a.mac1_offset; // any row alignment: bytes
    uint32_t w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
        w[q] = (uint32_t)m[4 * q] | ((uint32_t)m[4 * q + 1] << 8) | ((uint32_t)m[4 * q + 2] << 16) |
               ((uint32_t)m[4 * q + 3] << 24);
    a.state[(uint64_t)kStateQuads * p + 2] = make_uint4(w[0], w[1], w[2], w[3]);
}

} // namespace
} // namespace rg

using namespace rg::host;

extern "C" size_t rg_peer_ts_workspace_size(size_t n, uint32_t npeers) { return (size_t)rg::ts_layout(n, npeers).total; }

extern "C" int rg_peer_ts_batch_dev(rg_ctx *ctx, rg_hs_peer_state *state, uint32_t npeers, rg_hs_init_result *results,
                                    uint8_t *status, uint32_t *peers_out, size_t n, void *workspace,
                                    size_t workspace_len, void *stream) {
    rg::DeviceGuard dg_;
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!results || !status || !peers_out || !workspace || (npeers && !state) || n > 0xFFFFFFFFull)
        return set_err(RG_EINVAL, "peer ts: bad args");
    if (misaligned(state, 16) || misaligned(results, 16) || misaligned(peers_out, 4))
        return set_err(RG_EINVAL, "peer ts: state and results must be 16-byte aligned, peers_out 4-byte aligned");
    const rg::TsLayout L = rg::ts_layout(n, npeers);
    rc = check_workspace("peer ts", state, workspace, workspace_len, L.total);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    rg::TsArgs a{};
    a.state = reinterpret_cast<uint4 *>(state);
    a.results = reinterpret_cast<uint4 *>(results);
    a.status = status;
    a.peers_out = peers_out;
    a.rows = reinterpret_cast<uint32_t *>(ws + L.rows);
    a.lf = reinterpret_cast<rg::Ts *>(ws + L.lf);
    a.npeers = npeers;
    a.n = (uint32_t)n;
    hipLaunchKernelGGL(rg::ts_prep_kernel, lanes(n), kWg, 0, st, a);
    RG_HIP(hipGetLastError(), "peer ts: prep launch");
    if (npeers == 0) return RG_OK; // no row is eligible: prep answered them all
    a.g = rg::group_rows<rg::Ts>(a.rows, npeers, a.n, ws, L.g, st);
    rg::segscan(a, st);
    hipLaunchKernelGGL(rg::ts_advance_kernel, lanes(n), kWg, 0, st, a);
    RG_HIP(hipGetLastError(), "peer ts: scan launch");
    return RG_OK;
}

extern "C" int rg_peer_cookie_consume_batch_dev(rg_ctx *ctx, rg_hs_peer_state *state, uint32_t npeers,
                                                const uint8_t *cookie_keys, const rg_rx_entry *sess_table,
                                                uint32_t sess_cap, const rg_pkt_desc *desc, const uint8_t *gate,
                                                size_t n, const uint8_t *buf, size_t buf_len, uint8_t *cookies_out,
                                                uint32_t *claim, uint8_t *status, void *stream) {
    rg::DeviceGuard dg_;
    const int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!sess_table || !desc || !buf || !cookies_out || !status || (npeers && (!state || !cookie_keys || !claim)) ||
        n > 0xFFFFFFFFull)
        return set_err(RG_EINVAL, "peer cookie consume: bad args");
    if (!pow2(sess_cap))
        return set_err(RG_EINVAL, "peer cookie consume: sess_cap must be a power of two");
    if (misaligned(state, 16) || misaligned(cookie_keys, 16) || misaligned(desc, 16) || misaligned(sess_table, 4) ||
        misaligned(cookies_out, 4) || misaligned(claim, 4))
        return set_err(RG_EINVAL, "peer cookie consume: state, cookie_keys and desc must be 16-byte aligned, "
                                  "sess_table, cookies_out and claim 4-byte aligned");
    rg::ConsumeArgs a{};
    a.state = reinterpret_cast<uint4 *>(state);
    a.npeers = npeers;
    a.keys = reinterpret_cast<const uint32_t *>(cookie_keys);
    a.table = sess_table;
    a.cap = sess_cap;
    a.desc = desc;
    a.gate = gate;
    a.buf = buf;
    a.buf_len = buf_len;
    a.cookies_out = reinterpret_cast<uint32_t *>(cookies_out);
    a.claim = claim;
    a.status = status;
    a.n = (uint32_t)n;
    hipStream_t s = (hipStream_t)stream;
    if (npeers) RG_HIP(hipMemsetAsync(claim, 0, (size_t)npeers * sizeof(uint32_t), s), "peer cookie consume claim");
    hipLaunchKernelGGL(rg::cookie_consume_kernel, lanes(n), kWg, 0, s, a);
    RG_HIP(hipGetLastError(), "peer cookie consume launch");
    if (npeers) {
        hipLaunchKernelGGL(rg::cookie_commit_kernel, lanes(npeers), kWg, 0, s, a);
        RG_HIP(hipGetLastError(), "peer cookie consume commit launch");
    }
    return RG_OK;
}

extern "C" int rg_peer_cookies_batch_dev(rg_ctx *ctx, const rg_hs_peer_state *state, uint32_t npeers,
                                         const uint32_t *peer_idx, size_t n, uint8_t *cookies_out,
                                         uint8_t *has_cookie_out, void *stream) {
    rg::DeviceGuard dg_;
    const int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!peer_idx || !cookies_out || !has_cookie_out || (npeers && !state) || n > 0xFFFFFFFFull)
        return set_err(RG_EINVAL, "peer cookies: bad args");
    if (misaligned(state, 16) || misaligned(peer_idx, 4) || misaligned(cookies_out, 4))
        return set_err(RG_EINVAL, "peer cookies: state must be 16-byte aligned, peer_idx and cookies_out 4-byte aligned");
    rg::GatherArgs a{};
    a.state = reinterpret_cast<const uint4 *>(state);
    a.npeers = npeers;
    a.peer_idx = peer_idx;
    a.cookies_out = reinterpret_cast<uint32_t *>(cookies_out);
    a.has_out = has_cookie_out;
    a.n = (uint32_t)n;
    hipLaunchKernelGGL(rg::cookie_gather_kernel, lanes(n), kWg, 0, (hipStream_t)stream, a);
    RG_HIP(hipGetLastError(), "peer cookies launch");
    return RG_OK;
}

extern "C" int rg_peer_mac1_batch_dev(rg_ctx *ctx, rg_hs_peer_state *state, uint32_t npeers, const uint32_t *peer_idx,
                                      const uint8_t *status, const uint8_t *messages, uint32_t stride,
                                      uint32_t mac1_offset, size_t n, uint32_t *claim, void *stream) {
    rg::DeviceGuard dg_;
    const int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!peer_idx || !status || !messages || (npeers && (!state || !claim)) || n > 0xFFFFFFFFull)
        return set_err(RG_EINVAL, "peer mac1: bad args");
    if ((mac1_offset & 3u) != 0 || mac1_offset > stride || stride - mac1_offset < 16)
        return set_err(RG_EINVAL, "peer mac1: mac1_offset must be a multiple of 4 with mac1_offset + 16 <= stride");
    if (misaligned(state, 16) || misaligned(peer_idx, 4) || misaligned(claim, 4))
        return set_err(RG_EINVAL, "peer mac1: state must be 16-byte aligned, peer_idx and claim 4-byte aligned");
    if (npeers == 0) return RG_OK; // no row names a peer
    rg::Mac1Args a{};
    a.state = reinterpret_cast<uint4 *>(state);
    a.npeers = npeers;
    a.peer_idx = peer_idx;
    a.status = status;
    a.messages = messages;
    a.stride = stride;
    a.mac1_offset = mac1_offset;
    a.claim = claim;
    a.n = (uint32_t)n;
    hipStream_t s = (hipStream_t)stream;
    RG_HIP(hipMemsetAsync(claim, 0, (size_t)npeers * sizeof(uint32_t), s), "peer mac1 claim");
    hipLaunchKernelGGL(rg::mac1_claim_kernel, lanes(n), kWg, 0, s, a);
    RG_HIP(hipGetLastError(), "peer mac1 launch");
    hipLaunchKernelGGL(rg::mac1_commit_kernel, lanes(npeers), kWg, 0, s, a);
    RG_HIP(hipGetLastError(), "peer mac1 commit launch");
    return RG_OK;
}
