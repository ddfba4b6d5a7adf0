// rg_ratelimit.hip -- the responder's handshake rate limiter kept on the device: DynamicState::overloaded
// (rustyguard-core/src/lib.rs:508-514), a count-min sketch over source addresses (rustyguard-utils/src/
// rate_limiter.rs) that handle_handshake_init / _resp bump once per handshake message before the MACs are looked at
// (handshake.rs:47, :151), and the wipe and reseed of Sessions::turn (lib.rs:406-408).
//
//   rg_rate_count_batch_dev  every counted message bumps its depth buckets; its estimate and overload flag come back
//   rg_rate_turn_dev         once the period has passed: buckets zero, new seeds, last_reset_ns = now
//   rg_rate_column           the column of one address in one sketch row, on the host (rg_ratehash.h)
//
// The count equals an in-order loop (include/rg_aead.h has it) with nothing decided by the order the lanes arrive
// in.  A batch of n messages is n * depth items, item i * depth + r = (message i, sketch row r).  An item's bucket
// is r * width + col: one stable grouping of all items by that word and one segmented count serve every sketch row
// at once (a loop of depth groupings would be as correct and launch depth times the radix passes).  The item of
// rank k among its bucket's counted items reads min(bucket + k + 1, 2^32 - 1), which is what the loop's k + 1
// saturating increments leave, and a message's estimate is the minimum over its depth items.  Kernels, all on the
// call's stream:
//   rate_key      one lane per message: counted or not (the filter's frame rules and the type word), the key of its
//                 address, then the bucket word of each of its items, RG_KEY_SKIP for a message that is not counted
//   radix_hist / radix_scan / radix_scatter   rg_grouped.h: the items grouped by bucket; none for a sketch of one
//                 bucket
//   seg_reduce / carry / seg_verdict   rg_grouped.h's segscan with CountArgs as its pass: per tile of 2048 grouped
//                 items the aggregate of the segmented count, one workgroup scans the aggregates, then every counted
//                 item's estimate (judge) and the count of its bucket at the bucket's last item (tail)
//   rate_finish   one lane per item: the lane of a bucket's last item stores the bucket; one lane per message: the
//                 minimum over its items, counts_out, then overload_out
// An item that is not counted rides along in bucket 0's group and adds nothing.  Buckets are read by the scan's judge
// and written by rate_finish, never both in one kernel.  Plain vector stores only; no atomics on global memory.
// The turn's kernels: rate_decide, one lane, reads the clock and writes reset_out and last_reset_ns; rate_wipe
// behind it reads reset_out alone, so the decision is taken once and a replayed graph reads its clock when it runs.
//
// The entry points' host side is here too (rg_pending.hip's precedent).  Every argument rule is answered before the
// device is selected.  All scratch is the caller's; nothing is allocated, waited for or kept in the context, and
// every fill is a kernel, so the calls capture into a graph without memset nodes.
#include "rg_host.h"
#include "rg_grouped.h"
#include "rg_ratehash.h"

namespace rg {
namespace {

constexpr uint32_t kInitLen = 148, kRespLen = 92; // HandshakeInit, HandshakeResp (rustyguard-types)

static_assert(sizeof(rg_rate_seed) == 16 && sizeof(rg_src_addr) == 24 && sizeof(rg_pkt_desc) == 16, "layouts");

// rg_rate_tables as the kernels take it
struct Tables {
    uint32_t *buckets;       // [depth][width]
    ulonglong2 *seeds;       // [depth]: a in .x, b in .y
    uint64_t *last_reset_ns; // [1]
    uint32_t width, depth;
};

// segmented count: v = counted items since the bucket's first item
struct AddOp {
    __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; }
};

// Workspace of the count call (WorkspaceCursor, rg_internal.h).  total == 0: a size is out of range.  Every term is
// non-decreasing in n, width and depth.
struct RateLayout {
    uint64_t rows; // [n * depth] u32: the bucket word of a counted item, RG_KEY_SKIP otherwise
    GroupLayout g; // the grouped order and the aggregates (u32) of the segmented count
    uint64_t tot;  // [n * depth] u32: the counted items of a bucket, at its last grouped item
    uint64_t est;  // [n * depth] u32: the estimate of each counted item
    uint64_t total;
};
bool shape_ok(uint64_t width, uint64_t depth) {
    return width != 0 && depth != 0 && depth <= RG_RATE_MAX_DEPTH && width <= 0xFFFFFFFFull &&
           width * depth <= 0xFFFFFFFFull;
}
RateLayout rate_layout(uint64_t n, uint64_t width, uint64_t depth) {
    RateLayout L{};
    if (!shape_ok(width, depth) || n > 0xFFFFFFFFull || n * depth > 0xFFFFFFFFull) return L; // total = 0
    const uint64_t items = n * depth;
    WorkspaceCursor ws;
    L.rows = ws.take(items * 4);
    L.g.take(ws, items, (uint32_t)(width * depth), sizeof(uint32_t));
    L.tot = ws.take(items * 4);
    L.est = ws.take(items * 4);
    L.total = ws.total();
    return L;
}

__device__ __forceinline__ uint32_t sat_add(uint32_t a, uint32_t b) {
    const uint32_t s = a + b;
    return s < a ? 0xFFFFFFFFu : s;
}

// ---------------------------------------------------------------- the count
// The call's arguments; the scan kernels take them as the pass of rg_grouped.h's segscan.
struct CountArgs {
    using Pair = SegPair<uint32_t, AddOp>;
    using Item = SegItem; // key = the item's bucket
    Tables t;
    const rg_pkt_desc *desc; // [n]
    const uint64_t *addrs;   // [n][3]: rg_src_addr as three words
    const uint8_t *buf;
    uint64_t buf_len;
    uint32_t limit;
    uint32_t *counts_out;  // [n] or nullptr
    uint8_t *overload_out; // [n]
    uint32_t *rows;        // [n * depth] workspace
    uint32_t *tot;         // [n * depth] workspace
    uint32_t *est;         // [n * depth] workspace
    uint32_t n;
    GroupScan<uint32_t> g; // over the items: g.rows = rows, g.nrows = width * depth, g.n = n * depth

    __device__ __forceinline__ void load(Item &) const {}
    __device__ __forceinline__ uint32_t value(const Item &it) const { return it.row ? 1u : 0u; }
    __device__ __forceinline__ void seen(const Item &) const {}
    // upto = the bucket's counted items up to and with this one (the bucket is read only here; rate_finish
    // writes it)
    __device__ __forceinline__ void judge(const Item &it, uint32_t, uint32_t upto) const {
        if (it.row) est[it.i] = sat_add(t.buckets[it.key], upto);
    }
    // the bucket's last item of the batch hands the count to rate_finish
    __device__ __forceinline__ void tail(uint64_t pos, const Item &, uint32_t upto) const { tot[pos] = upto; }
};

// The filter goes on to read this message's MACs: its frame rules in its order (rg_noise.h frame_verdict), then the
// type word.  Nothing outside [buf, buf + buf_len) is read.
__device__ __forceinline__ bool counted(const CountArgs &a, const rg_pkt_desc &d) {
    if ((d.offset & 15u) != 0) return false;
    if (d.offset > a.buf_len || d.len > a.buf_len - d.offset || (d.len != kInitLen && d.len != kRespLen)) return false;
    if (d.key_idx == RG_KEY_SKIP) return false;
    return *reinterpret_cast<const uint32_t *>(a.buf + d.offset) == (d.len == kInitLen ? 1u : 2u);
}

__global__ __launch_bounds__(256) void rate_key_kernel(CountArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const bool cnt = counted(a, a.desc[i]);
    const uint64_t *ap = a.addrs + 3ull * i;
    const uint64_t key = cnt ? rate_key(ap[0], ap[1]) : 0ull;
    uint32_t *out = a.rows + (uint64_t)i * a.t.depth;
    for (uint32_t r = 0; r < a.t.depth; ++r) {
        uint32_t w = RG_KEY_SKIP;
        if (cnt) {
            const ulonglong2 s = a.t.seeds[r];
            w = r * a.t.width + rate_column(key, s.x, s.y, a.t.width); // < width * depth <= 2^32 - 1
        }
        out[r] = w;
    }
}

// One lane per item: the lane of a bucket's last grouped item stores the bucket.  One lane per message: the
// minimum over its items, counts_out, then overload_out.
__global__ __launch_bounds__(256) void rate_finish_kernel(CountArgs a) {
    const uint64_t pos = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (pos >= a.g.n) return;
    const uint32_t key = a.g.key_at(pos);
    if (a.g.is_tail(pos, key) && key < a.g.nrows) {
        const uint32_t c = a.tot[pos];
        if (c) a.t.buckets[key] = sat_add(a.t.buckets[key], c); // a bucket without a counted item stays as it is
    }
    if (pos >= a.n) return;
    const uint64_t first = pos * a.t.depth; // message pos
    uint32_t est = 0;
    if (a.rows[first] != RG_KEY_SKIP) { // counted: all of its items are
        est = 0xFFFFFFFFu;
        for (uint32_t r = 0; r < a.t.depth; ++r) est = min(est, a.est[first + r]);
    }
    if (a.counts_out) a.counts_out[pos] = est;
    a.overload_out[pos] = est > a.limit ? 1 : 0;
}

// ----------------------------------------------------------------- the turn
struct TurnArgs {
    Tables t;
    const uint64_t *now_ns;
    uint64_t period_ns;
    const ulonglong2 *new_seeds; // [depth]
    uint32_t *reset_out;         // [1]
};

__global__ void rate_decide_kernel(TurnArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint64_t now = *a.now_ns, last = *a.t.last_reset_ns;
    const bool reset = now > last && now - last > a.period_ns;
    if (reset) *a.t.last_reset_ns = now;
    *a.reset_out = reset ? 1u : 0u;
}

// one lane per bucket (and per seed: depth <= width * depth)
__global__ __launch_bounds__(256) void rate_wipe_kernel(TurnArgs a) {
    if (*a.reset_out == 0) return;
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < (uint64_t)a.t.width * a.t.depth) a.t.buckets[k] = 0;
    if (k < a.t.depth) a.t.seeds[k] = a.new_seeds[k];
}

} // namespace
} // namespace rg

using namespace rg::host;

namespace {
// the struct's rules (include/rg_aead.h), answered without a look at the device; RG_OK with the kernels' view in *out
int check_tables(const char *what, const rg_rate_tables *t, rg::Tables *out) {
    if (!t) return bad(what, "bad args");
    if (!t->buckets || !t->seeds || !t->last_reset_ns) return bad(what, "a null array in the tables");
    if (!rg::shape_ok(t->width, t->depth))
        return bad(what, "width must be 1 or more, depth 1 to RG_RATE_MAX_DEPTH and width * depth at most 2^32 - 1");
    if (misaligned(t->seeds, 16) || misaligned(t->last_reset_ns, 8) || misaligned(t->buckets, 4))
        return bad(what, "seeds must be 16-byte, last_reset_ns 8-byte and buckets 4-byte aligned");
    out->buckets = t->buckets;
    out->seeds = reinterpret_cast<ulonglong2 *>(t->seeds);
    out->last_reset_ns = t->last_reset_ns;
    out->width = t->width;
    out->depth = t->depth;
    return RG_OK;
}
} // namespace

extern "C" uint32_t rg_rate_column(const rg_rate_seed *seed, const rg_src_addr *addr, uint32_t width) {
    if (!seed || !addr) return 0;
    uint64_t w[2] = {0, 0}; // the address as two little-endian words, whatever the host's byte order
    for (int k = 0; k < 16; ++k) w[k >> 3] |= (uint64_t)addr->ip[k] << (8 * (k & 7));
    return rg::rate_column(rg::rate_key(w[0], w[1]), seed->a, seed->b, width);
}

extern "C" size_t rg_rate_workspace_size(size_t n, uint32_t width, uint32_t depth) {
    return (size_t)rg::rate_layout(n, width, depth).total;
}

extern "C" int rg_rate_count_batch_dev(rg_ctx *ctx, const rg_rate_tables *tables, const rg_pkt_desc *desc,
                                       const rg_src_addr *addrs, size_t n, const uint8_t *buf, size_t buf_len,
                                       uint32_t limit, uint32_t *counts_out, uint8_t *overload_out, void *workspace,
                                       size_t workspace_len, void *stream) {
    const char *what = "rate count";
    if (!ctx) return set_err(RG_EINVAL, "null context");
    if (n == 0) return RG_OK;
    if (!desc || !addrs || !buf || !overload_out || !workspace || n > 0xFFFFFFFFull) return bad(what, "bad args");
    rg::CountArgs a{};
    int rc = check_tables(what, tables, &a.t);
    if (rc) return rc;
    if ((uint64_t)n * a.t.depth > 0xFFFFFFFFull) return bad(what, "n * depth above 2^32 - 1");
    if (misaligned(addrs, 8) || misaligned(counts_out, 4))
        return bad(what, "addrs must be 8-byte and counts_out 4-byte aligned");
    const rg::RateLayout L = rg::rate_layout(n, a.t.width, a.t.depth);
    rc = check_workspace(what, tables->last_reset_ns, workspace, workspace_len, L.total);
    if (rc) return rc;
    rg::DeviceGuard dg_;
    rc = check_ctx(ctx);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    const uint32_t items = (uint32_t)(n * a.t.depth);
    a.desc = desc;
    a.addrs = reinterpret_cast<const uint64_t *>(addrs);
    a.buf = buf;
    a.buf_len = buf_len;
    a.limit = limit;
    a.counts_out = counts_out;
    a.overload_out = overload_out;
    a.rows = reinterpret_cast<uint32_t *>(ws + L.rows);
    a.tot = reinterpret_cast<uint32_t *>(ws + L.tot);
    a.est = reinterpret_cast<uint32_t *>(ws + L.est);
    a.n = (uint32_t)n;
    hipLaunchKernelGGL(rg::rate_key_kernel, lanes(n), kWg, 0, st, a);
    a.g = rg::group_rows<uint32_t>(a.rows, a.t.width * a.t.depth, items, ws, L.g, st);
    rg::segscan(a, st);
    hipLaunchKernelGGL(rg::rate_finish_kernel, lanes(items), kWg, 0, st, a);
    RG_HIP(hipGetLastError(), what);
    return RG_OK;
}

extern "C" int rg_rate_turn_dev(rg_ctx *ctx, const rg_rate_tables *tables, const uint64_t *now_ns, uint64_t period_ns,
                                const rg_rate_seed *new_seeds, uint32_t *reset_out, void *stream) {
    const char *what = "rate turn";
    if (!ctx) return set_err(RG_EINVAL, "null context");
    if (!now_ns || !new_seeds || !reset_out) return bad(what, "bad args");
    rg::TurnArgs a{};
    int rc = check_tables(what, tables, &a.t);
    if (rc) return rc;
    if (misaligned(new_seeds, 16) || misaligned(now_ns, 8) || misaligned(reset_out, 4))
        return bad(what, "new_seeds must be 16-byte, now_ns 8-byte and reset_out 4-byte aligned");
    rg::DeviceGuard dg_;
    rc = check_ctx(ctx);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    a.now_ns = now_ns;
    a.period_ns = period_ns;
    a.new_seeds = reinterpret_cast<const ulonglong2 *>(new_seeds);
    a.reset_out = reset_out;
    hipLaunchKernelGGL(rg::rate_decide_kernel, dim3(1), dim3(64), 0, st, a);
    hipLaunchKernelGGL(rg::rate_wipe_kernel, lanes((uint64_t)a.t.width * a.t.depth), kWg, 0, st, a);
    RG_HIP(hipGetLastError(), what);
    return RG_OK;
}
