// rg_replay.hip -- the RFC 6479 anti-replay window on the device, batched: the in-order tail of
// DecryptionKey::decrypt (rustyguard-crypto/src/prim.rs:414-437; AntiReplay::{would_accept, mark_seen},
// rustyguard-utils/src/anti_replay.rs:25-64) for a whole batch, and a receive that never leaves the stream
// (rg_recv_batch_dev_resident: resolve + gate, open, commit, re-seal of what the commit rejected).
//
// The sequential rule has a closed form over a batch ("Device-resident anti-replay").  For
// window w with last = L0 at the start and S = its packets, in array order, whose status is OK or
// DECRYPT_ERR:
//   M_p    = max(L0, counters of the OK packets of S before p)         a segmented prefix maximum
//   p is REJECTED iff  ctr_p <= M_p and M_p - ctr_p >= 1984            too old
//                  or  ctr_p <= M_p, ctr_p's block <= L0's block and its bit is set in the window as it
//                      stood at the start                              seen before the batch
//                  or  an earlier OK packet of S has the same counter  seen in the batch
//   last'  = M over all of S; slot j & 31 of the bitmap, for the block j in (last' / 64 - 32, last' / 64],
//            keeps its starting word when j <= L0 / 64 and starts from zero otherwise, OR the bits of the
//            accepted packets of block j.
//
// Kernels of the commit pass, all on the call's stream:
//   radix_hist / radix_scan / radix_scatter   stable grouping of the packet indices by window: an LSD radix
//            sort over the window index, 8 bits per pass, as many passes as the window count needs (none
//            for one window: the array is its own grouping)
//   replay_clear    the (window, counter) table starts empty
//   seg_reduce / carry / seg_verdict   rg_grouped.h's segscan with ReplayArgs as its pass.  The reduce walk:
//            per workgroup of 2048 grouped packets the aggregate of the segmented prefix maximum; every OK
//            packet enters the (window, counter) table, the smallest packet index winning (seen).  The
//            verdict walk: every packet's M_p, the three tests, status and undo (judge); the running maximum
//            at each window's last packet (tail)
//   replay_advance  one lane per window with traffic: the slots the window moved past are cleared, last'
//   replay_mark     the accepted packets' bits (64-bit atomic OR)
// A packet without a window (RG_KEY_SKIP, out of range) or without a verdict to judge (any status but OK /
// DECRYPT_ERR, RG_PKT_PENDING included) rides along in window 0's group as a neutral element and comes
// back untouched.
//
// The entry points' host side is here too (rg_cookie.hip's precedent), on rg_host.h like the host units,
// none of which names a launcher of this file.  All scratch is the caller's workspace; nothing is
// allocated, waited for or kept.
#include "rg_device.h"
#include "rg_host.h"
#include "rg_grouped.h"

namespace rg {
namespace {

// Workspace of the device anti-replay calls (WorkspaceCursor, rg_internal.h).  total == 0: the batch is too
// large.
struct ReplayLayout {
    uint64_t rdesc; // [n] rg_pkt_desc: working descriptors of the open (RG_KEY_SKIP = unknown or gated); = 0
    // commit pass
    uint64_t hash; // [hash_cap] u32: earliest RG_PKT_OK packet of each (window, counter)
    GroupLayout g; // the grouped order and the aggregates (u64) of the segmented prefix maximum
    uint64_t lf;   // [n] u64: the running maximum at each window's last packet
    // resident receive (rdesc at offset 0: include/rg_aead.h documents it to callers)
    uint64_t ctr;     // [n] u64: header counters
    uint64_t widx;    // [n] u32: resolved key rows = window rows
    uint64_t undo;    // [n] u8
    uint64_t ustatus; // [n] u8: statuses of the re-seal
    uint64_t udesc;   // [n] rg_pkt_desc: re-seal descriptors
    uint64_t total;
    uint64_t hash_cap; // a power of two >= 2 n
};
ReplayLayout replay_layout(uint64_t n, uint32_t nwin) {
    ReplayLayout L{};
    if (n > 0xFFFFFFFFull) return L; // total = 0
    WorkspaceCursor ws;
    L.hash_cap = 64;
    while (L.hash_cap < 2 * n) L.hash_cap <<= 1;
    L.rdesc = ws.take(n * sizeof(rg_pkt_desc));
    L.hash = ws.take(L.hash_cap * 4);
    L.g.take(ws, n, nwin, sizeof(uint64_t));
    L.lf = ws.take(n * 8);
    L.ctr = ws.take(n * 8);
    L.widx = ws.take(n * 4);
    L.undo = ws.take(n);
    L.ustatus = ws.take(n);
    L.udesc = ws.take(n * sizeof(rg_pkt_desc));
    L.total = ws.total();
    return L;
}

constexpr uint32_t kEmpty = 0xFFFFFFFFu; // (window, counter) table: free slot (n <= 2^32 - 1)

__device__ __forceinline__ uint64_t hash_slot(uint32_t w, uint64_t c, uint64_t mask) {
    uint64_t x = c ^ ((uint64_t)w * 0x9E3779B97F4A7C15ull);
    x ^= x >> 32;
    x *= 0xD6E8FEB86659FD93ull;
    x ^= x >> 32;
    x *= 0xD6E8FEB86659FD93ull;
    x ^= x >> 32;
    return x & mask;
}

__global__ __launch_bounds__(256) void replay_clear_kernel(uint4 *hash4, uint64_t quads) {
    for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (uint64_t)gridDim.x * 256)
        hash4[q] = make_uint4(kEmpty, kEmpty, kEmpty, kEmpty);
}

// segmented prefix maximum: v = the largest OK counter since the window's first packet (0 when none: every
// window's last is >= 0)
struct MaxOp {
    __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const { return a > b ? a : b; }
};

// The commit's arguments; the scan kernels take them as the pass of rg_grouped.h's segscan.
struct ReplayArgs {
    using Pair = SegPair<uint64_t, MaxOp>;
    struct Item : SegItem {
        uint32_t st; // status, or 0xFF without a window
        uint64_t ctr;
    };
    rg_antireplay *windows;
    const uint64_t *counters; // [n]
    uint8_t *status;          // [n]
    uint8_t *undo;            // [n] or nullptr
    uint32_t *hash;
    uint64_t hash_mask;
    uint64_t *lf;
    GroupScan<uint64_t> g; // g.rows = the packets' window rows

    // (window, counter) -> earliest OK packet.  A slot holds the index of a packet with the slot's key; packets
    // of one key lower it to their smallest index.  Once taken, a slot's key never changes, so a probe compares
    // against whichever index it reads.  The table has at least two slots per packet: a probe ends.
    __device__ __forceinline__ void hash_insert(uint32_t i, uint32_t w, uint64_t c) const {
        for (uint64_t s = hash_slot(w, c, hash_mask);; s = (s + 1) & hash_mask) {
            const uint32_t e = atomicCAS(&hash[s], kEmpty, i);
            if (e == kEmpty) return;
            if (g.rows[e] == w && counters[e] == c) {
                atomicMin(&hash[s], i);
                return;
            }
        }
    }
    __device__ __forceinline__ uint32_t hash_find(uint32_t w, uint64_t c) const {
        for (uint64_t s = hash_slot(w, c, hash_mask);; s = (s + 1) & hash_mask) {
            const uint32_t e = hash[s];
            if (e == kEmpty) return kEmpty;
            if (g.rows[e] == w && counters[e] == c) return e;
        }
    }

    __device__ __forceinline__ void load(Item &it) const {
        it.st = it.row ? status[it.i] : 0xFFu;
        it.ctr = it.row && it.st <= RG_PKT_DECRYPT_ERR ? counters[it.i] : 0ull;
    }
    __device__ __forceinline__ uint64_t value(const Item &it) const { return it.st == RG_PKT_OK ? it.ctr : 0ull; }
    // every OK packet enters the table, the smallest packet index winning
    __device__ __forceinline__ void seen(const Item &it) const {
        if (it.st == RG_PKT_OK) hash_insert(it.i, it.key, it.ctr);
    }
    // before = the largest OK counter of the window ahead of this packet
    __device__ __forceinline__ void judge(const Item &it, uint64_t before, uint64_t) const {
        uint8_t u = 0;
        if (it.st <= RG_PKT_DECRYPT_ERR) { // has a window and a verdict to judge
            const rg_antireplay &win = windows[it.key];
            const uint64_t L0 = win.last, M = before > L0 ? before : L0, c = it.ctr;
            bool rej = false;
            if (c <= M) {
                if (M - c >= RG_REPLAY_WINDOW) rej = true;
                else if ((c >> 6) <= (L0 >> 6) && ((win.bitmap[(c >> 6) & 31] >> (c & 63)) & 1ull)) rej = true;
                else {
                    const uint32_t first = hash_find(it.key, c);
                    rej = first != kEmpty && first < it.i;
                }
            }
            if (rej) {
                u = it.st == RG_PKT_OK;
                status[it.i] = RG_PKT_REJECTED; // also for a bad tag: would_accept comes first
            }
        }
        if (undo) undo[it.i] = u;
    }
    // the window's last packet of the batch hands the running maximum to replay_advance
    __device__ __forceinline__ void tail(uint64_t pos, const Item &, uint64_t upto) const { lf[pos] = upto; }
};

// One lane per window with traffic (the lane of its last grouped packet): the slots of the blocks the
// window moved past start from zero, then last.  Both branches of mark_seen: a jump of more than 32
// blocks leaves no block j <= L0 / 64 in reach, so every slot is cleared.
__global__ __launch_bounds__(256) void replay_advance_kernel(ReplayArgs a) {
    const uint64_t pos = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (pos >= a.g.n) return;
    const uint32_t key = a.g.key_at(pos);
    if (!a.g.is_tail(pos, key)) return;
    if (key >= a.g.nrows) return; // no window at all
    rg_antireplay &win = a.windows[key];
    const uint64_t L0 = win.last, Lf = a.lf[pos];
    if (Lf <= L0) return; // nothing accepted above last: no slot changes hands
    const uint64_t bf = Lf >> 6, b0 = L0 >> 6;
    for (uint32_t s = 0; s < 32; ++s) {
        const uint64_t back = (bf - s) & 31u; // slot s holds block bf - back
        if (back <= bf && bf - back > b0) win.bitmap[s] = 0;
    }
    win.last = Lf;
}

__global__ __launch_bounds__(256) void replay_mark_kernel(ReplayArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.g.n) return;
    const uint32_t w = a.g.rows[i];
    if (!a.g.has_row(w) || a.status[i] != RG_PKT_OK) return;
    rg_antireplay &win = a.windows[w];
    const uint64_t c = a.counters[i];
    if ((win.last >> 6) - (c >> 6) < 32) // else the window has moved past its block since
        atomicOr(reinterpret_cast<unsigned long long *>(&win.bitmap[(c >> 6) & 31]), 1ull << (c & 63));
}

// packets without windows at all (nwin == 0): nothing to judge
__global__ __launch_bounds__(256) void replay_none_kernel(uint8_t *undo, uint32_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) undo[i] = 0;
}

hipError_t launch_commit(rg_antireplay *windows, uint32_t nwin, const uint32_t *win_idx, const uint64_t *counters,
                         uint32_t n, uint8_t *status, uint8_t *undo, uint8_t *ws, const ReplayLayout &L,
                         hipStream_t st) {
    const dim3 per_packet = host::lanes(n), wg = host::kWg;
    if (nwin == 0) {
        if (undo) hipLaunchKernelGGL(replay_none_kernel, per_packet, wg, 0, st, undo, n);
        return hipGetLastError();
    }
    ReplayArgs a{};
    a.windows = windows;
    a.counters = counters;
    a.status = status;
    a.undo = undo;
    a.hash = reinterpret_cast<uint32_t *>(ws + L.hash);
    a.hash_mask = L.hash_cap - 1;
    a.lf = reinterpret_cast<uint64_t *>(ws + L.lf);
    a.g = group_rows<uint64_t>(win_idx, nwin, n, ws, L.g, st);
    const uint64_t quads = L.hash_cap / 4;
    hipLaunchKernelGGL(replay_clear_kernel, dim3((uint32_t)((quads + 255) / 256 < 2048 ? (quads + 255) / 256 : 2048)), wg, 0, st,
                       reinterpret_cast<uint4 *>(a.hash), quads);
    segscan(a, st);
    hipLaunchKernelGGL(replay_advance_kernel, per_packet, wg, 0, st, a);
    hipLaunchKernelGGL(replay_mark_kernel, per_packet, wg, 0, st, a);
    return hipGetLastError();
}

// ------------------------------------------------------- resident receive
struct ResidentArgs {
    const rg_pkt_desc *desc;
    const uint8_t *buf;
    uint64_t buf_len;
    const rg_rx_entry *table;
    uint32_t cap;
    const rg_antireplay *windows;
    uint32_t nkeys;
    uint32_t n;
    rg_pkt_desc *rdesc;
    uint64_t *ctr;
    uint32_t *widx;
    uint32_t *key_out;      // or nullptr
    const uint8_t *undo;    // undo pass
    rg_pkt_desc *udesc;     // undo pass
    uint64_t *counters_out; // undo pass, or nullptr
};

// rx_resolve_kernel (rg_kernels.hip; the frame check and the lookup are rg_internal.h's, shared with it)
// with the would_accept pre-check of prim.rs:414-420: a frame whose
// session is known and whose header counter the window, as it stands before the batch, would not accept
// goes to the open kernels as RG_KEY_SKIP -- RG_PKT_REJECTED, no AEAD work, frame untouched.  Exact: last
// only grows, and a seen bit leaves the window only when its counter has become too old.
__global__ __launch_bounds__(256) void resident_gate_kernel(ResidentArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    rg_pkt_desc d = a.desc[i];
    uint32_t k = 0, found = RG_KEY_SKIP;
    uint64_t ctr = 0;
    uint4 hdr;
    if (rx_frame_header(d, a.buf, a.buf_len, hdr)) {
        ctr = ((uint64_t)hdr.w << 32) | hdr.z;
        k = found = rx_find(a.table, a.cap, hdr.y);
        if (found != RG_KEY_SKIP && found < a.nkeys) {
            const rg_antireplay &win = a.windows[found];
            const uint64_t last = win.last;
            if (ctr <= last && (last - ctr >= RG_REPLAY_WINDOW || ((win.bitmap[(ctr >> 6) & 31] >> (ctr & 63)) & 1ull)))
                k = RG_KEY_SKIP;
        }
    }
    d.key_idx = k;
    a.rdesc[i] = d;
    a.ctr[i] = ctr;
    a.widx[i] = found;
    if (a.key_out) a.key_out[i] = found;
}

// Re-seal descriptors of the frames the open decrypted and the commit then rejected (payload W - 32, the
// open's key row; RG_KEY_SKIP for every other packet), and the header counter of a gated packet, which
// the open kernels did not report.
__global__ __launch_bounds__(256) void resident_undo_kernel(ResidentArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const rg_pkt_desc d = a.rdesc[i];
    rg_pkt_desc u{0, 0, RG_KEY_SKIP};
    if (a.undo[i]) u = rg_pkt_desc{d.offset, d.len - 32, d.key_idx};
    a.udesc[i] = u;
    if (a.counters_out && d.key_idx == RG_KEY_SKIP && a.widx[i] != RG_KEY_SKIP) a.counters_out[i] = a.ctr[i];
}

} // namespace
} // namespace rg

extern "C" size_t rg_replay_workspace_size(size_t n, uint32_t nwin) { return (size_t)rg::replay_layout(n, nwin).total; }

extern "C" int rg_replay_batch_dev(rg_ctx *ctx, rg_antireplay *windows, uint32_t nwin, const uint32_t *win_idx,
                                   const uint64_t *counters, size_t n, uint8_t *status, uint8_t *undo,
                                   void *workspace, size_t workspace_len, void *stream) {
    using namespace rg::host;
    rg::DeviceGuard dg_;
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!windows || !win_idx || !counters || !status || !workspace || n > 0xFFFFFFFFull)
        return set_err(RG_EINVAL, "replay: bad args");
    const rg::ReplayLayout L = rg::replay_layout(n, nwin);
    rc = check_workspace("replay", windows, workspace, workspace_len, L.total);
    if (rc) return rc;
    RG_HIP(rg::launch_commit(windows, nwin, win_idx, counters, (uint32_t)n, status, undo,
                             static_cast<uint8_t *>(workspace), L, (hipStream_t)stream),
           "replay launch");
    return RG_OK;
}

extern "C" int rg_recv_batch_dev_resident(rg_ctx *ctx, const uint8_t *keys, uint32_t nkeys,
                                          const rg_rx_entry *rx_table, uint32_t rx_cap, rg_antireplay *windows,
                                          const rg_pkt_desc *desc, size_t n, uint8_t *buf, size_t buf_len,
                                          uint8_t *status, uint64_t *counters_out, uint32_t *key_idx_out,
                                          void *workspace, size_t workspace_len, void *stream) {
    using namespace rg::host;
    rg::DeviceGuard dg_;
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!keys || nkeys == 0 || !rx_table || !pow2(rx_cap) || !windows || !desc || !buf ||
        !status || !workspace || n > 0xFFFFFFFFull)
        return set_err(RG_EINVAL, "recv resident: bad args");
    const rg::ReplayLayout L = rg::replay_layout(n, nkeys);
    rc = check_workspace("recv resident", windows, workspace, workspace_len, L.total);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = claim_stream(ctx, st); // before anything is enqueued
    if (rc) return rc;
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    rg::ResidentArgs a{};
    a.desc = desc;
    a.buf = buf;
    a.buf_len = buf_len;
    a.table = rx_table;
    a.cap = rx_cap;
    a.windows = windows;
    a.nkeys = nkeys;
    a.n = (uint32_t)n;
    a.rdesc = reinterpret_cast<rg_pkt_desc *>(ws + L.rdesc);
    a.ctr = reinterpret_cast<uint64_t *>(ws + L.ctr);
    a.widx = reinterpret_cast<uint32_t *>(ws + L.widx);
    a.key_out = key_idx_out;
    uint8_t *undo = ws + L.undo;
    a.undo = undo;
    a.udesc = reinterpret_cast<rg_pkt_desc *>(ws + L.udesc);
    a.counters_out = counters_out;
    const dim3 grid = lanes(n), wg = kWg;
    hipLaunchKernelGGL(rg::resident_gate_kernel, grid, wg, 0, st, a);
    RG_HIP(hipGetLastError(), "recv resident: gate launch");
    rc = rg_open_batch_dev(ctx, keys, nkeys, a.rdesc, n, buf, buf_len, status, counters_out, stream);
    if (rc) return rc;
    RG_HIP(rg::launch_commit(windows, nkeys, a.widx, a.ctr, (uint32_t)n, status, undo, ws, L, st),
           "recv resident: commit launch");
    hipLaunchKernelGGL(rg::resident_undo_kernel, grid, wg, 0, st, a);
    RG_HIP(hipGetLastError(), "recv resident: undo launch");
    // re-seal under the same key row and counter: ciphertext and tag come back byte for byte; without
    // receivers the header is not rewritten (rg_recv_batch_dev_finish)
    return rg_seal_batch_dev(ctx, keys, nullptr, nkeys, a.udesc, a.ctr, n, buf, buf_len, ws + L.ustatus, stream);
}
