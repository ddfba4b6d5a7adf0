// rg_send.hip -- send counters reserved on the device, batched: the sequential part of
// EncryptionKey::encrypt (rustyguard-crypto/src/prim.rs:376-399: `counter` handed out and incremented) and
// PeerState::force_encrypt (rustyguard-core/src/lib.rs:260-297: should_reject / should_expire, `sent`) for a
// whole batch, and a send that never leaves the stream (rg_send_batch_dev_resident: reserve, seal, verdicts).
//
// The array-order loop (include/rg_aead.h, rg_send_reserve_batch_dev) has a closed form over a batch
// ("Device-resident send").  For row w with counter = C0 at the start and E = its eligible
// packets in array order (valid row, len % 16 == 0, row not expired -- none of which the loop changes):
//   packet of rank r in E takes C0 + r   iff  C0 < REJECT and r < REJECT - C0      (ranks are compared, never
//                                             C0 + r with REJECT: that sum can wrap 64 bits)
//   rekey = C0 + r + 1 >= REKEY
//   counter' = C0 + min(|E|, REJECT - C0) (unchanged for C0 >= REJECT), sent' = now iff a packet took one
// r is a stable segmented exclusive count of eligibility flags over the packets grouped by row.
//
// Kernels, all on the call's stream:
//   radix_hist / radix_scan / radix_scatter   stable grouping of the packet indices by row; none for one row:
//            the array is its own grouping
//   send_reduce    per workgroup of 2048 grouped packets the aggregate of the segmented count: each wave
//            walks its quarter 64 packets a round (ballots of eligibility and of row heads, popcounts), the
//            four waves meet in LDS
//   carry          one workgroup scans the aggregates
//   send_verdict   every packet's rank, then status, counter, rekey flag and working descriptor; |E| at each
//            row's last packet
//   send_update    one lane per row with traffic: counter', sent'
//   send_overlay   (resident send) the verdicts of packets without a counter over the seal's statuses
// A packet without a row (RG_KEY_SKIP, out of range) rides along in row 0's group, not eligible.
// Plain vector stores only; no atomics on global memory.
// Shared with the anti-replay commit (rg_replay.hip), in rg_grouped.h: the radix passes, the grouped view of
// the batch, the segmented pair, the carry kernel and the workspace arrays of these.  The walk over a tile
// (ballots and popcounts, since the value is a count of flags) is this file's.
//
// The entry points' host side is here too (rg_replay.hip's precedent), on rg_host.h like the host units.
// All scratch is the caller's workspace; nothing is allocated, waited for or kept.
#include "rg_device.h"
#include "rg_host.h"
#include "rg_grouped.h"

namespace rg {
namespace {

constexpr uint64_t kRejectAfterTimeNs = RG_REJECT_AFTER_TIME_NS; // lib.rs:204-209

// Workspace of the device send calls (WorkspaceCursor, rg_internal.h).  total == 0: the batch is too large.
// Every term is non-decreasing in n and in nkeys.
struct SendLayout {
    uint64_t wdesc;   // [n] rg_pkt_desc: working descriptors (RG_KEY_SKIP = took no counter); = 0
    GroupLayout g;    // the grouped order and the aggregates (u32) of the segmented count
    uint64_t tot;     // [n] u32: |E| at each row's last grouped packet
    uint64_t verdict; // [n] u8: the reserve's statuses (resident send)
    uint64_t ctr;     // [n] u64: reserved counters when the caller passes no counters_out (resident send)
    uint64_t total;
};
SendLayout send_layout(uint64_t n, uint32_t nkeys) {
    SendLayout L{};
    if (n > 0xFFFFFFFFull) return L;
    WorkspaceCursor ws;
    L.wdesc = ws.take(n * sizeof(rg_pkt_desc));
    L.g.take(ws, n, nkeys, sizeof(uint32_t));
    L.tot = ws.take(n * 4);
    L.verdict = ws.take(n);
    L.ctr = ws.take(n * 8);
    L.total = ws.total();
    return L;
}

struct SendArgs {
    rg_send_state *state;
    const rg_pkt_desc *desc; // [n]
    const uint64_t *now_ns;  // one u64, or nullptr: no time rule
    uint8_t *status;         // [n]
    uint64_t *counters_out;  // [n]
    uint8_t *rekey_out;      // [n] or nullptr
    rg_pkt_desc *wdesc;      // [n]
    uint32_t *tot;
    GroupScan<uint32_t> g;   // g.rows = the packets' slot words
};

__device__ __forceinline__ bool expired(const SendArgs &a, uint32_t w, bool timed, uint64_t now) {
    return timed && a.state[w].started_ns + kRejectAfterTimeNs < now; // u64 wrapping add, as the host
}

// segmented count: v = eligible packets since the row's first packet
struct AddOp {
    __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; }
};
using Pair = SegPair<uint32_t, AddOp>;

// One grouped packet as the scan sees it.  (f, v) is the packet's exclusive prefix inside its wave's quarter
// of the tile: f = a row began at or before it there, v = eligible packets of its row ahead of it there.
struct Item {
    uint32_t i, w; // packet index, its slot word; i == 0xFFFFFFFF beyond the batch
    uint32_t key;
    uint32_t f, v;
    bool elig;
};

// The workgroup's tile: wave v owns the contiguous quarter v and walks it 64 positions a round.  Fills
// items[] and returns the exclusive prefix of this wave inside the tile; `total` is the tile's aggregate.
__device__ __forceinline__ Pair tile_scan(const SendArgs &a, Item (&items)[kTileItems], Pair &total) {
    __shared__ uint32_t s_f[4], s_v[4];
    const uint32_t t = threadIdx.x, v = t >> 6, lane = t & 63;
    const uint64_t base = (uint64_t)blockIdx.x * kGroupTile + v * (kGroupTile / 4);
    const bool timed = a.now_ns != nullptr;
    const uint64_t now = timed ? *a.now_ns : 0ull;
    const uint64_t below = (1ull << lane) - 1, upto = (2ull << lane) - 1;
    // the key ahead of this wave's first position (a row's head is a change of key)
    uint32_t last_key = a.g.key_before(base);
    Pair run{0u, 0u};
#pragma unroll
    for (uint32_t r = 0; r < kTileItems; ++r) {
        const uint64_t pos = base + r * 64 + lane;
        Item it{0xFFFFFFFFu, RG_KEY_SKIP, 0u, 0u, 0u, false};
        bool head = false;
        if (pos < a.g.n) {
            it.i = a.g.index_at(pos);
            it.w = a.g.rows[it.i];
            const bool row = a.g.has_row(it.w);
            it.key = row ? it.w : 0u;
            it.elig = row && (a.desc[it.i].len & 15u) == 0 && !expired(a, it.w, timed, now);
        }
        const uint32_t up = __shfl_up(it.key, 1);
        const uint32_t prev = lane ? up : last_key;
        if (pos < a.g.n) head = pos == 0 || it.key != prev;
        const uint64_t H = __ballot(head), E = __ballot(it.elig);
        const uint64_t hm = H & upto;
        if (hm) { // the packet's row began in this round
            const uint32_t s = 63u - (uint32_t)__clzll((long long)hm);
            it.f = 1u;
            it.v = (uint32_t)__popcll(E & below & ~((1ull << s) - 1));
        } else {
            it.f = run.f;
            it.v = run.v + (uint32_t)__popcll(E & below);
        }
        items[r] = it;
        if (H) {
            const uint32_t s = 63u - (uint32_t)__clzll((long long)H);
            run = Pair{1u, (uint32_t)__popcll(E & ~((1ull << s) - 1))};
        } else {
            run.v += (uint32_t)__popcll(E);
        }
        last_key = __shfl(it.key, 63);
    }
    if (lane == 0) {
        s_f[v] = run.f;
        s_v[v] = run.v;
    }
    __syncthreads();
    Pair ex{0u, 0u}, all{0u, 0u};
    for (uint32_t q = 0; q < 4; ++q) {
        if (q == v) ex = all;
        all = join(all, Pair{s_f[q], s_v[q]});
    }
    total = all;
    return ex;
}

__global__ __launch_bounds__(256) void send_reduce_kernel(SendArgs a) {
    Item items[kTileItems];
    Pair total;
    (void)tile_scan(a, items, total);
    store_tile(a.g.agg, total);
}

__global__ __launch_bounds__(256) void send_verdict_kernel(SendArgs a) {
    Item items[kTileItems];
    Pair total;
    const Pair wave_ex = tile_scan(a, items, total);
    const Pair ex = join(tile_start<Pair>(a.g.agg), wave_ex);
    const uint32_t v = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t base = (uint64_t)blockIdx.x * kGroupTile + v * (kGroupTile / 4);
#pragma unroll
    for (uint32_t r = 0; r < kTileItems; ++r) {
        const Item &it = items[r];
        const uint64_t pos = base + r * 64 + lane;
        if (pos >= a.g.n) continue;
        const uint64_t rank = it.f ? (uint64_t)it.v : (uint64_t)ex.v + it.v; // eligible packets of the row ahead
        rg_pkt_desc d = a.desc[it.i];
        d.key_idx = RG_KEY_SKIP;
        uint64_t ctr = 0;
        uint8_t st = RG_PKT_REJECTED, rekey = 0;
        if (a.g.has_row(it.w)) {
            if ((d.len & 15u) != 0) st = RG_PKT_INVALID; // takes no counter
            else if (it.elig) {                          // else the row has expired
                const uint64_t C0 = a.state[it.w].counter;
                const uint64_t room = C0 < RG_REJECT_AFTER_MESSAGES ? RG_REJECT_AFTER_MESSAGES - C0 : 0ull;
                if (rank < room) {
                    ctr = C0 + rank; // < REJECT: neither this sum nor ctr + 1 wraps
                    rekey = ctr + 1 >= RG_REKEY_AFTER_MESSAGES;
                    st = RG_PKT_PENDING; // a counter is reserved; only a seal lane may write RG_PKT_OK
                    d.key_idx = it.w;
                }
            }
        }
        a.status[it.i] = st;
        a.counters_out[it.i] = ctr;
        if (a.rekey_out) a.rekey_out[it.i] = rekey;
        a.wdesc[it.i] = d;
        // the row's last packet of the batch hands |E| to send_update
        if (a.g.is_tail(pos, it.key)) a.tot[pos] = (uint32_t)rank + (it.elig ? 1u : 0u);
    }
}

// One lane per row with traffic (the lane of its last grouped packet).
__global__ __launch_bounds__(256) void send_update_kernel(SendArgs a) {
    const uint64_t pos = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (pos >= a.g.n) return;
    const uint32_t key = a.g.key_at(pos);
    if (!a.g.is_tail(pos, key)) return;
    if (key >= a.g.nrows) return;
    rg_send_state &row = a.state[key];
    const uint64_t C0 = row.counter, E = a.tot[pos];
    const uint64_t room = C0 < RG_REJECT_AFTER_MESSAGES ? RG_REJECT_AFTER_MESSAGES - C0 : 0ull;
    const uint64_t took = E < room ? E : room;
    if (took == 0) return; // the row stays byte for byte
    row.counter = C0 + took;
    if (a.now_ns) row.sent_ns = *a.now_ns; // force_encrypt, lib.rs:285
}

// no rows at all (nkeys == 0): every packet is rejected
__global__ __launch_bounds__(256) void send_none_kernel(SendArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.g.n) return;
    rg_pkt_desc d = a.desc[i];
    d.key_idx = RG_KEY_SKIP;
    a.status[i] = RG_PKT_REJECTED;
    a.counters_out[i] = 0;
    if (a.rekey_out) a.rekey_out[i] = 0;
    a.wdesc[i] = d;
}

// the verdicts of the packets that took no counter replace what the seal wrote for their RG_KEY_SKIP rows
__global__ __launch_bounds__(256) void send_overlay_kernel(const uint8_t *verdict, uint8_t *status, uint32_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint8_t v = verdict[i];
    if (v != RG_PKT_PENDING) status[i] = v;
}

hipError_t launch_reserve(rg_send_state *state, uint32_t nkeys, const uint32_t *slots, const rg_pkt_desc *desc,
                          uint32_t n, const uint64_t *now_ns, uint8_t *status, uint64_t *counters_out,
                          uint8_t *rekey_out, uint8_t *ws, const SendLayout &L, hipStream_t st) {
    SendArgs a{};
    a.state = state;
    a.desc = desc;
    a.now_ns = now_ns;
    a.status = status;
    a.counters_out = counters_out;
    a.rekey_out = rekey_out;
    a.wdesc = reinterpret_cast<rg_pkt_desc *>(ws + L.wdesc);
    a.tot = reinterpret_cast<uint32_t *>(ws + L.tot);
    const dim3 per_packet = host::lanes(n), tiles(L.g.nblk), wg = host::kWg;
    if (nkeys == 0) {
        a.g.n = n;
        hipLaunchKernelGGL(send_none_kernel, per_packet, wg, 0, st, a);
        return hipGetLastError();
    }
    a.g = group_rows<uint32_t>(slots, nkeys, n, ws, L.g, st);
    hipLaunchKernelGGL(send_reduce_kernel, tiles, wg, 0, st, a);
    hipLaunchKernelGGL(carry_kernel<Pair>, dim3(1), wg, 0, st, a.g.agg);
    hipLaunchKernelGGL(send_verdict_kernel, tiles, wg, 0, st, a);
    hipLaunchKernelGGL(send_update_kernel, per_packet, wg, 0, st, a);
    return hipGetLastError();
}

} // namespace
} // namespace rg

extern "C" size_t rg_send_workspace_size(size_t n, uint32_t nkeys) { return (size_t)rg::send_layout(n, nkeys).total; }

extern "C" int rg_send_reserve_batch_dev(rg_ctx *ctx, rg_send_state *state, uint32_t nkeys, const uint32_t *slots,
                                         const rg_pkt_desc *desc, size_t n, const uint64_t *now_ns, uint8_t *status,
                                         uint64_t *counters_out, uint8_t *rekey_out, void *workspace,
                                         size_t workspace_len, void *stream) {
    using namespace rg::host;
    rg::DeviceGuard dg_;
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!state || !slots || !desc || !status || !counters_out || !workspace || n > 0xFFFFFFFFull)
        return set_err(RG_EINVAL, "send reserve: bad args");
    const rg::SendLayout L = rg::send_layout(n, nkeys);
    rc = check_workspace("send reserve", state, workspace, workspace_len, L.total);
    if (rc) return rc;
    RG_HIP(rg::launch_reserve(state, nkeys, slots, desc, (uint32_t)n, now_ns, status, counters_out, rekey_out,
                              static_cast<uint8_t *>(workspace), L, (hipStream_t)stream),
           "send reserve launch");
    return RG_OK;
}

extern "C" int rg_send_batch_dev_resident(rg_ctx *ctx, const uint8_t *keys, const uint32_t *receivers, uint32_t nkeys,
                                          rg_send_state *state, const uint32_t *slots, const rg_pkt_desc *desc,
                                          size_t n, const uint64_t *now_ns, uint8_t *buf, size_t buf_len,
                                          uint8_t *status, uint64_t *counters_out, uint8_t *rekey_out, void *workspace,
                                          size_t workspace_len, void *stream) {
    using namespace rg::host;
    rg::DeviceGuard dg_;
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!keys || !receivers || nkeys == 0 || !state || !slots || !desc || !buf || !status || !workspace ||
        n > 0xFFFFFFFFull)
        return set_err(RG_EINVAL, "send resident: bad args");
    const rg::SendLayout L = rg::send_layout(n, nkeys);
    rc = check_workspace("send resident", state, workspace, workspace_len, L.total);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = claim_stream(ctx, st); // before any counter is taken
    if (rc) return rc;
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    uint8_t *verdict = ws + L.verdict;
    uint64_t *ctr = counters_out ? counters_out : reinterpret_cast<uint64_t *>(ws + L.ctr);
    RG_HIP(rg::launch_reserve(state, nkeys, slots, desc, (uint32_t)n, now_ns, verdict, ctr, rekey_out, ws, L, st),
           "send resident: reserve launch");
    // a packet that took no counter is RG_KEY_SKIP to the seal: no AEAD work, frame untouched
    rc = rg_seal_batch_dev(ctx, keys, receivers, nkeys, reinterpret_cast<const rg_pkt_desc *>(ws + L.wdesc), ctr, n, buf,
                           buf_len, status, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(rg::send_overlay_kernel, lanes(n), kWg, 0, st, (const uint8_t *)verdict, status, (uint32_t)n);
    RG_HIP(hipGetLastError(), "send resident: overlay launch");
    return RG_OK;
}
