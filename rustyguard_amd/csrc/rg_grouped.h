// rg_grouped.h -- what a batch pass over packets grouped by a row shares: the device anti-replay commit
// (rg_replay.hip: row = window, a segmented prefix maximum), the peers' timestamp check (rg_peerstate.hip:
// row = peer, a segmented prefix maximum), the handshake rate limiter (rg_ratelimit.hip: row = sketch bucket,
// a segmented count) and the device send-counter reservation (rg_send.hip: row = session, a segmented
// count).  Device code and its launchers only.
//   Grouped          the device view of a batch and its grouped order; also the key of the radix passes
//   SegPair          the segmented-scan monoid over a value type and an operation; Tally the plain sum
//   AggLayout        the tiles' aggregates in a workspace, Agg their typed pointers
//   block_prefix     exclusive scan of one SegPair per lane over a workgroup, carry_kernel over the tiles'
//                    aggregates
//   compact          the ordered compaction of an array: count, carry, rank.  Its users say what an item
//                    contributes and what a ranked item does: the eligible handshakes and the free rows of
//                    the session install (rg_session.hip), the two lists of the timer turn (rg_timers.hip),
//                    of the pending turn (rg_pending.hip), the three of the inbound demux (rg_demux.hip)
//   GroupLayout      the workspace arrays every grouped pass has, group_rows their typed pointers and the order
//   segscan          the segmented scan over the grouped order: reduce, carry, verdict.  Its users say what an
//                    item loads and contributes, how it is judged with the prefix of its row and what the
//                    row's last item hands on: the first three files above
// Both cores walk a tile of kGroupTile positions the same way, kTileItems consecutive positions a lane and
// the lanes' runs scanned through LDS, which serves any monoid.  rg_send.hip shares everything here but
// that walk: its value is a count of flags, so a wave ranks 64 positions a round by ballots and popcounts
// with one meeting in LDS per tile where block_prefix takes eight steps (with its measured
// times).
//
// The grouping is stable, by the passes of an LSD radix sort over the 32-bit key, 8 bits per pass.  KeyOf is
// a small struct passed by value with `__device__ uint32_t operator()(uint32_t i) const`: the grouping key
// of packet i (Grouped is one).  One pass:
//   radix_hist_kernel     digit counts per workgroup of kGroupTile positions
//   radix_scan_kernel     exclusive prefix sum over the digit-major counts, one workgroup
//   radix_scatter_kernel  stable scatter behind those offsets
// group_by_key runs as many passes as the key range needs and returns the grouped order (nullptr for no
// pass: the array is its own grouping).
#pragma once
#include "rg_internal.h"

namespace rg {

constexpr uint32_t kGroupTile = 2048; // packets per workgroup of 256 lanes, in the scans and the radix passes
constexpr uint32_t kTileItems = kGroupTile / 256; // positions per lane of a tile

// A batch of n packets, each with a row word (rows[i]; RG_KEY_SKIP or >= nrows: no row), and the packet
// indices grouped by row.  A packet without a row rides along in row 0's group.
struct Grouped {
    const uint32_t *rows;  // [n]
    const uint32_t *order; // [n] packet indices grouped by row, or nullptr: array order
    uint32_t nrows;
    uint32_t n;
    __device__ __forceinline__ bool has_row(uint32_t w) const { return w != RG_KEY_SKIP && w < nrows; }
    // the grouping key: a packet's row, 0 for a packet without one
    __device__ __forceinline__ uint32_t key_of(uint32_t i) const {
        const uint32_t w = rows[i];
        return has_row(w) ? w : 0u;
    }
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return key_of(i); }
    // (the grouped order is a permutation of [0, n); the bound keeps every later access inside the batch's
    // arrays whatever the workspace holds)
    __device__ __forceinline__ uint32_t index_at(uint64_t pos) const {
        return order ? min(order[pos], n - 1) : (uint32_t)pos;
    }
    __device__ __forceinline__ uint32_t key_at(uint64_t pos) const { return key_of(index_at(pos)); }
    // the key ahead of a lane's or wave's first position `base` (a row's head is a change of key)
    __device__ __forceinline__ uint32_t key_before(uint64_t base) const {
        return base > 0 && base < n ? key_at(base - 1) : 0u;
    }
    // pos holds the last grouped packet of the row `key`: the lane that updates the row
    __device__ __forceinline__ bool is_tail(uint64_t pos, uint32_t key) const {
        return pos + 1 == n || key_at(pos + 1) != key;
    }
};

// (f, v) of a run of grouped packets: f = the run holds a row's first packet, v = Op over the values since
// the last such packet.  join is associative; {0, 0} is its identity for the two operations in use.
template <class V, class Op>
struct SegPair {
    using value_type = V;
    uint32_t f;
    V v;
};
template <class V, class Op>
__device__ __forceinline__ SegPair<V, Op> join(const SegPair<V, Op> &a, const SegPair<V, Op> &b) {
    return SegPair<V, Op>{a.f | b.f, b.f ? b.v : Op{}(a.v, b.v)};
}

// The per-tile aggregates of a scan over n items, in this order in the caller's workspace.
struct AggLayout {
    uint64_t agg_val;  // [nblk] V and
    uint64_t agg_flag; // [nblk] u32
    uint32_t nblk;     // tiles of kGroupTile items
    void take_agg(WorkspaceCursor &ws, uint64_t n, uint64_t value_size) {
        nblk = (uint32_t)((n + kGroupTile - 1) / kGroupTile);
        agg_val = ws.take((uint64_t)nblk * value_size);
        agg_flag = ws.take((uint64_t)nblk * 4);
    }
};
template <class V>
struct Agg {
    V *val;
    uint32_t *flag;
    uint32_t nblk;
    Agg() = default;
    Agg(uint8_t *ws, const AggLayout &L)
        : val(reinterpret_cast<V *>(ws + L.agg_val)), flag(reinterpret_cast<uint32_t *>(ws + L.agg_flag)),
          nblk(L.nblk) {}
};
// the workgroup's tile: lane 0 stores its aggregate; what the tile starts from, once carry_kernel has run
template <class Pair>
__device__ __forceinline__ void store_tile(const Agg<typename Pair::value_type> &agg, const Pair &total) {
    if (threadIdx.x == 0) {
        agg.flag[blockIdx.x] = total.f;
        agg.val[blockIdx.x] = total.v;
    }
}
template <class Pair>
__device__ __forceinline__ Pair tile_start(const Agg<typename Pair::value_type> &agg) {
    return Pair{agg.flag[blockIdx.x], agg.val[blockIdx.x]};
}

// exclusive prefix of one Pair per lane over the workgroup's 256 lanes (returned), and their total
template <class Pair>
__device__ __forceinline__ Pair block_prefix(const Pair &mine, Pair &total) {
    using V = typename Pair::value_type;
    __shared__ uint32_t s_f[256];
    __shared__ V s_v[256];
    const uint32_t t = threadIdx.x;
    s_f[t] = mine.f;
    s_v[t] = mine.v;
    __syncthreads();
    Pair cur = mine;
    for (uint32_t off = 1; off < 256; off <<= 1) {
        const bool has = t >= off;
        Pair o{0u, V(0)};
        if (has) o = Pair{s_f[t - off], s_v[t - off]};
        __syncthreads();
        if (has) {
            cur = join(o, cur);
            s_f[t] = cur.f;
            s_v[t] = cur.v;
        }
        __syncthreads();
    }
    total = Pair{s_f[255], s_v[255]};
    return t ? Pair{s_f[t - 1], s_v[t - 1]} : Pair{0u, V(0)};
}

// the tiles' aggregates -> what each tile starts from (exclusive), in place; one workgroup
template <class Pair>
__global__ __launch_bounds__(256) void carry_kernel(Agg<typename Pair::value_type> agg) {
    const uint32_t t = threadIdx.x, nblk = agg.nblk;
    const uint32_t per = (nblk + 255) / 256, lo = min(t * per, nblk), hi = min(lo + per, nblk);
    Pair run{0u, 0u};
    for (uint32_t j = lo; j < hi; ++j) run = join(run, Pair{agg.flag[j], agg.val[j]});
    Pair total;
    Pair ex = block_prefix(run, total);
    for (uint32_t j = lo; j < hi; ++j) {
        const Pair cur{agg.flag[j], agg.val[j]};
        agg.flag[j] = ex.f;
        agg.val[j] = ex.v;
        ex = join(ex, cur);
    }
}

// ------------------------------------------------------ ordered compaction
// the plain sum: a SegPair whose f stays 0
template <class V>
struct Plus {
    __device__ __forceinline__ V operator()(V a, V b) const { return a + b; }
};
template <class V>
using Tally = SegPair<V, Plus<V>>;

// A pass is a small struct passed by value.  Both walks call `V item(uint64_t pos) const` for every pos < n:
// what the position contributes to the sum (several counts may share a V, each in bits of its own).  The
// rank walk then calls `void emit(uint64_t pos, V v, V ex) const` with the contribution and the sum over
// all positions below pos, and `void total(V all) const` once, with the sum over [0, n).  The passes of the
// two walks may differ where the first has something to do once (the install's judging).
template <class V, class Pass>
__global__ __launch_bounds__(256) void compact_count_kernel(Pass p, uint32_t n, Agg<V> agg) {
    const uint64_t base = (uint64_t)blockIdx.x * kGroupTile + threadIdx.x * kTileItems;
    V cnt = 0;
    for (uint32_t k = 0; k < kTileItems; ++k)
        if (base + k < n) cnt += p.item(base + k);
    Tally<V> total;
    (void)block_prefix(Tally<V>{0u, cnt}, total);
    if (threadIdx.x == 0) {
        agg.flag[blockIdx.x] = 0;
        agg.val[blockIdx.x] = total.v;
    }
}
template <class V, class Pass>
__global__ __launch_bounds__(256) void compact_rank_kernel(Pass p, uint32_t n, Agg<V> agg) {
    const uint64_t base = (uint64_t)blockIdx.x * kGroupTile + threadIdx.x * kTileItems;
    V v[kTileItems], cnt = 0;
#pragma unroll
    for (uint32_t k = 0; k < kTileItems; ++k) {
        v[k] = base + k < n ? p.item(base + k) : V(0);
        cnt += v[k];
    }
    Tally<V> total;
    V ex = agg.val[blockIdx.x] + block_prefix(Tally<V>{0u, cnt}, total).v;
    const V all = agg.val[blockIdx.x] + total.v; // everything up to this tile's end
#pragma unroll
    for (uint32_t k = 0; k < kTileItems; ++k) {
        if (base + k < n) p.emit(base + k, v[k], ex);
        ex += v[k];
    }
    if (blockIdx.x == agg.nblk - 1 && threadIdx.x == 0) p.total(all);
}
// count -> carry -> rank over [0, n) on st
template <class V, class CountPass, class RankPass>
inline void compact(CountPass count, RankPass rank, uint32_t n, const Agg<V> &agg, hipStream_t st) {
    const dim3 tiles(agg.nblk), wg(256);
    hipLaunchKernelGGL((compact_count_kernel<V, CountPass>), tiles, wg, 0, st, count, n, agg);
    hipLaunchKernelGGL(carry_kernel<Tally<V>>, dim3(1), wg, 0, st, agg);
    hipLaunchKernelGGL((compact_rank_kernel<V, RankPass>), tiles, wg, 0, st, rank, n, agg);
}

// 8-bit passes that order keys below nkeys (0: one key, no grouping)
__host__ __device__ inline uint32_t radix_passes(uint32_t nkeys) {
    uint32_t p = 0;
    for (uint32_t top = nkeys ? nkeys - 1 : 0; top; top >>= 8) ++p;
    return p;
}

// One pass of a stable LSD radix sort: workgroup b owns positions [b, b + 1) x kGroupTile of src
// (src == nullptr: the identity).
template <class KeyOf>
__global__ __launch_bounds__(256) void radix_hist_kernel(KeyOf key, uint32_t n, uint32_t nblk, const uint32_t *src,
                                                         uint32_t shift, uint32_t *hist) {
    __shared__ uint32_t s_h[256];
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kGroupTile;
    for (uint32_t k = 0; k < kTileItems; ++k) {
        const uint64_t pos = base + k * 256 + threadIdx.x;
        if (pos < n) atomicAdd(&s_h[(key(src ? src[pos] : (uint32_t)pos) >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(uint64_t)threadIdx.x * nblk + blockIdx.x] = s_h[threadIdx.x];
}

// exclusive prefix sum over hist[0, total), digit-major: one workgroup, a contiguous run per lane (a
// template like its neighbours, so that it is emitted beside them in each file that groups)
template <class KeyOf>
__global__ __launch_bounds__(1024) void radix_scan_kernel(uint32_t *hist, uint64_t total) {
    __shared__ uint32_t s_sum[1024];
    const uint32_t t = threadIdx.x;
    const uint64_t per = (total + 1023) / 1024, lo = min(t * per, total), hi = min(lo + per, total);
    uint32_t sum = 0;
    for (uint64_t j = lo; j < hi; ++j) sum += hist[j];
    s_sum[t] = sum;
    __syncthreads();
    uint32_t cur = sum;
    for (uint32_t off = 1; off < 1024; off <<= 1) {
        const uint32_t o = t >= off ? s_sum[t - off] : 0u;
        __syncthreads();
        cur += o;
        s_sum[t] = cur;
        __syncthreads();
    }
    uint32_t run = cur - sum;
    for (uint64_t j = lo; j < hi; ++j) {
        const uint32_t c = hist[j];
        hist[j] = run;
        run += c;
    }
}

// Stable scatter: wave v of the workgroup owns the contiguous quarter v of the tile and walks it 64
// positions at a time; lanes of one round with the same digit find each other by ballots and take
// consecutive places behind the digit's running offset.
template <class KeyOf>
__global__ __launch_bounds__(256) void radix_scatter_kernel(KeyOf key, uint32_t n, uint32_t nblk, const uint32_t *src,
                                                            uint32_t *dst, uint32_t shift, const uint32_t *hist) {
    __shared__ uint32_t s_off[4][256];
    const uint32_t t = threadIdx.x, v = t >> 6, lane = t & 63;
    for (uint32_t q = 0; q < 4; ++q) s_off[q][t] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kGroupTile + v * (kGroupTile / 4);
    uint32_t idx[kTileItems], dg[kTileItems];
#pragma unroll
    for (uint32_t r = 0; r < kTileItems; ++r) {
        const uint64_t pos = base + r * 64 + lane;
        const bool ok = pos < n;
        idx[r] = ok ? (src ? src[pos] : (uint32_t)pos) : 0u;
        dg[r] = ok ? (key(idx[r]) >> shift) & 255u : 256u;
        if (ok) atomicAdd(&s_off[v][dg[r]], 1u);
    }
    __syncthreads();
    { // counts -> first place of (wave, digit): the workgroup's base, then the waves in order
        uint32_t run = hist[(uint64_t)t * nblk + blockIdx.x];
        for (uint32_t q = 0; q < 4; ++q) {
            const uint32_t c = s_off[q][t];
            s_off[q][t] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kTileItems; ++r) {
        const bool ok = dg[r] < 256u;
        uint64_t same = __ballot(ok);
#pragma unroll
        for (uint32_t b = 0; b < 8; ++b) {
            const bool bit = (dg[r] >> b) & 1u;
            const uint64_t m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1));
        const uint32_t off = ok ? s_off[v][dg[r]] : 0u;
        __syncthreads();
        if (ok && rank == 0) s_off[v][dg[r]] = off + (uint32_t)__popcll(same);
        if (ok) dst[(uint64_t)off + rank] = idx[r];
        __syncthreads();
    }
}

// The grouped order of [0, n) under `key`: `passes` passes ping-ponging between order0 and order1 (order1
// is touched only from the second pass on), hist = [256][nblk] u32.  Returns where the last pass wrote, or
// nullptr when passes == 0.
template <class KeyOf>
inline const uint32_t *group_by_key(KeyOf key, uint32_t n, uint32_t nblk, uint32_t passes, uint32_t *hist,
                                    uint32_t *order0, uint32_t *order1, hipStream_t st) {
    const dim3 tiles(nblk), wg(256);
    const uint32_t *src = nullptr;
    for (uint32_t p = 0; p < passes; ++p) {
        uint32_t *dst = (p & 1) ? order1 : order0;
        hipLaunchKernelGGL(radix_hist_kernel<KeyOf>, tiles, wg, 0, st, key, n, nblk, src, 8 * p, hist);
        hipLaunchKernelGGL(radix_scan_kernel<KeyOf>, dim3(1), dim3(1024), 0, st, hist, 256ull * nblk);
        hipLaunchKernelGGL(radix_scatter_kernel<KeyOf>, tiles, wg, 0, st, key, n, nblk, src, dst, 8 * p,
                           (const uint32_t *)hist);
        src = dst;
    }
    return src;
}

// The workspace arrays of a grouped scan, contiguous and in this order in the caller's workspace: the two
// orders, the histogram, then the per-tile aggregates of the segmented scan.
struct GroupLayout : AggLayout {
    uint64_t order[2]; // [n] u32 each: packet indices grouped by row (ping-pong of the radix passes)
    uint64_t hist;     // [256][nblk] u32: digit counts per workgroup
    uint32_t passes;   // 8-bit radix passes over the row index (0: one row, no grouping)
    void take(WorkspaceCursor &ws, uint64_t n, uint32_t nrows, uint64_t value_size) {
        const uint64_t tiles = (n + kGroupTile - 1) / kGroupTile;
        passes = radix_passes(nrows);
        order[0] = ws.take(passes > 0 ? n * 4 : 0);
        order[1] = ws.take(passes > 1 ? n * 4 : 0);
        hist = ws.take(passes > 0 ? 256ull * tiles * 4 : 0);
        take_agg(ws, n, value_size);
    }
};

// What the scan kernels of a grouped pass take: the view and the tiles' aggregates.
template <class V>
struct GroupScan : Grouped {
    Agg<V> agg;
};
// Groups the batch by row on `st` and returns the scan's arguments, out of the workspace at ws.
template <class V>
inline GroupScan<V> group_rows(const uint32_t *rows, uint32_t nrows, uint32_t n, uint8_t *ws, const GroupLayout &L,
                               hipStream_t st) {
    Grouped g{rows, nullptr, nrows, n};
    g.order = group_by_key(g, n, L.nblk, L.passes, reinterpret_cast<uint32_t *>(ws + L.hist),
                           reinterpret_cast<uint32_t *>(ws + L.order[0]),
                           reinterpret_cast<uint32_t *>(ws + L.order[1]), st);
    return GroupScan<V>{g, Agg<V>(ws, L)};
}

// ------------------------------------------------------ segmented scan
// One grouped packet as the scan sees it; a pass's Item derives from it.
struct SegItem {
    uint32_t i, key; // the packet; its row, 0 for a packet that rides along
    bool head, row;  // the first of its key in the grouped order; it has a row
};

// A pass is a small struct passed by value, all of its hooks const and __forceinline__ (the verdict walk keeps a
// lane's kTileItems items in registers):
//   Pair, Item, g     its SegPair, its item and the GroupScan that group_rows returned
//   void load(Item &)                  the item's own fields, once the core has filled SegItem's
//   V value(const Item &)              what the item contributes; V(0) is the identity
//   void seen(const Item &)            the reduce walk only, once per item
//   void judge(const Item &, V before, V upto)   the verdict walk: Op over the values of the item's row ahead
//                                      of it (the identity at the row's head), and up to and with it
//   void tail(uint64_t pos, const Item &, V upto)   behind judge, at the last grouped position of a row
template <class Pass>
__device__ __forceinline__ typename Pass::Item seg_load(const Pass &p, uint64_t pos, uint32_t prev_key) {
    typename Pass::Item it{};
    it.i = p.g.index_at(pos);
    const uint32_t w = p.g.rows[it.i];
    it.row = p.g.has_row(w);
    it.key = it.row ? w : 0u;
    it.head = pos == 0 || it.key != prev_key;
    p.load(it);
    return it;
}
template <class Pass>
__device__ __forceinline__ typename Pass::Pair seg_pair(const Pass &p, const typename Pass::Item &it) {
    return typename Pass::Pair{it.head ? 1u : 0u, p.value(it)};
}

template <class Pass>
__global__ __launch_bounds__(256) void seg_reduce_kernel(Pass p) {
    using Pair = typename Pass::Pair;
    const uint64_t base = (uint64_t)blockIdx.x * kGroupTile + threadIdx.x * kTileItems;
    uint32_t prev = p.g.key_before(base);
    Pair run{0u, 0u};
    for (uint32_t k = 0; k < kTileItems; ++k) {
        const uint64_t pos = base + k;
        if (pos >= p.g.n) break;
        const typename Pass::Item it = seg_load(p, pos, prev);
        prev = it.key;
        p.seen(it);
        run = join(run, seg_pair(p, it));
    }
    Pair total;
    (void)block_prefix(run, total);
    store_tile(p.g.agg, total);
}

template <class Pass>
__global__ __launch_bounds__(256) void seg_verdict_kernel(Pass p) {
    using Pair = typename Pass::Pair;
    using V = typename Pair::value_type;
    const uint64_t base = (uint64_t)blockIdx.x * kGroupTile + threadIdx.x * kTileItems;
    uint32_t prev = p.g.key_before(base);
    typename Pass::Item items[kTileItems];
    Pair run{0u, 0u};
#pragma unroll
    for (uint32_t k = 0; k < kTileItems; ++k) {
        const uint64_t pos = base + k;
        if (pos < p.g.n) {
            items[k] = seg_load(p, pos, prev);
            prev = items[k].key;
            run = join(run, seg_pair(p, items[k]));
        } else items[k] = typename Pass::Item{};
    }
    Pair total;
    const Pair mine = block_prefix(run, total);
    Pair ex = join(tile_start<Pair>(p.g.agg), mine);
#pragma unroll
    for (uint32_t k = 0; k < kTileItems; ++k) {
        const uint64_t pos = base + k;
        if (pos >= p.g.n) break;
        const typename Pass::Item &it = items[k];
        const V before = it.head ? V(0) : ex.v;
        ex = join(ex, seg_pair(p, it));
        p.judge(it, before, ex.v);
        if (p.g.is_tail(pos, it.key)) p.tail(pos, it, ex.v);
    }
}

// reduce -> carry -> verdict over the grouped batch p.g on st
template <class Pass>
inline void segscan(const Pass &p, hipStream_t st) {
    const dim3 tiles(p.g.agg.nblk), wg(256);
    hipLaunchKernelGGL(seg_reduce_kernel<Pass>, tiles, wg, 0, st, p);
    hipLaunchKernelGGL(carry_kernel<typename Pass::Pair>, dim3(1), wg, 0, st, p.g.agg);
    hipLaunchKernelGGL(seg_verdict_kernel<Pass>, tiles, wg, 0, st, p);
}

} // namespace rg
