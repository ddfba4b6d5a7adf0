// rg_demux.hip -- the dispatch of Sessions::recv_message (rustyguard-core/src/lib.rs:605-630) kept on the device:
// one array of datagrams in arrival order, message types 1-4 and junk interleaved, comes out as the descriptor
// lists the resident chains take, and the chains' verdicts go back to the datagrams' own order.
//
//   rg_demux_batch_dev          desc[n] -> the handshake, cookie and data lists, (status, cls, pos) per datagram
//   rg_demux_verdict_batch_dev  the chains' status arrays -> status[n], by (cls, pos)
//
// The split equals an in-order loop (include/rg_aead.h has it) with nothing decided by the order the lanes arrive
// in.  Its kernels:
//   compact  rg_grouped.h's count / carry / rank over the datagrams with ListCounts, three 32-bit counts, as the
//            sum.  The count walk (Classify) judges datagram i: its frame rules, then the type word at
//            buf + offset -- the one scattered load, made once.  It stores cls[i], and for a datagram that goes on no
//            list pos[i] and the verdict.  The rank walk (Place) reads cls[i] back instead of buf, and a datagram
//            whose rank is below its list's capacity stores its rows, pos[i] and RG_PKT_PENDING; one past the
//            capacity reads RG_PKT_FULL.  Which of init_desc / resp_desc gets a handshake row follows from its
//            length, which the count walk has tied to the type.  The totals go to counts.
//   pad      one lane per list row behind the compact: row r >= counts[list] of each list becomes the inert row.
//            Rows below the count were stored by Place, so every row of every list is written exactly once a call
//            and the cost of the tail follows the capacities, not n.
// The verdict is one lane per datagram; no index is taken from pos before it is compared with the list's capacity.
//
// The entry points' host side is here too (rg_endpoint.hip's precedent).  Every argument rule is answered before
// the device is selected.  All scratch is the caller's; nothing is allocated, waited for or kept in the context.
#include "rg_host.h"
#include "rg_grouped.h"

namespace rg {
namespace {

constexpr uint32_t kInitLen = 148, kRespLen = 92, kCookieLen = 64; // HandshakeInit, HandshakeResp, CookieMessage

static_assert(sizeof(rg_pkt_desc) == 16 && sizeof(rg_src_addr) == 24, "layouts");

// The sum of the compact: how many datagrams of a run go on each list.  A value of the scan needs `+`, `+=` and a
// conversion from 0; the default constructor stays trivial for the scan's LDS arrays.
struct ListCounts {
    uint32_t hs, ck, data;
    ListCounts() = default;
    __host__ __device__ ListCounts(uint32_t v) : hs(v), ck(v), data(v) {}
    __host__ __device__ ListCounts(uint32_t h, uint32_t c, uint32_t d) : hs(h), ck(c), data(d) {}
    __host__ __device__ ListCounts &operator+=(const ListCounts &o) {
        hs += o.hs;
        ck += o.ck;
        data += o.data;
        return *this;
    }
};
__host__ __device__ inline ListCounts operator+(const ListCounts &a, const ListCounts &b) {
    return ListCounts(a.hs + b.hs, a.ck + b.ck, a.data + b.data);
}

struct DemuxArgs {
    const uint4 *desc;     // [n] rg_pkt_desc: offset (x, y), len (z), key_idx (w)
    const uint64_t *addrs; // [n][3]: rg_src_addr as three words
    const uint8_t *buf;
    uint64_t buf_len;
    uint4 *hs_desc, *init_desc, *resp_desc; // [cap_hs]
    uint64_t *hs_addrs;                     // [cap_hs][3]
    uint4 *ck_desc;                         // [cap_ck]
    uint4 *data_desc;                       // [cap_data]
    uint64_t *data_addrs;                   // [cap_data][3]
    uint32_t cap_hs, cap_ck, cap_data;
    uint8_t *status, *cls; // [n]
    uint32_t *pos;         // [n]
    uint32_t *counts;      // [6]: rank of hs, ck, data, then seen
};

// what a datagram of class c (0: on no list) adds to the sum
__device__ __forceinline__ ListCounts one_of(uint32_t c) {
    return ListCounts(c == 1u || c == 2u ? 1u : 0u, c == 3u ? 1u : 0u, c == 4u ? 1u : 0u);
}

__device__ __forceinline__ uint4 inert_row() { return make_uint4(0u, 0u, 0u, RG_KEY_SKIP); }

// a source address with its pad zeroed, or 24 zero bytes
__device__ __forceinline__ void put_addr(uint64_t *rows, uint64_t k, const uint64_t *src) {
    uint64_t *d = rows + 3ull * k;
    d[0] = src ? src[0] : 0ull;
    d[1] = src ? src[1] : 0ull;
    d[2] = src ? src[2] & 0xFFFFull : 0ull; // port_le
}

// The count walk: recv_message's rules in its order, the class into cls[i], the verdict of what is listed nowhere.
struct Classify {
    DemuxArgs a;
    __device__ __forceinline__ ListCounts item(uint64_t i) const {
        const uint4 d = a.desc[i];
        const uint64_t off = d.x | ((uint64_t)d.y << 32);
        const uint32_t len = d.z;
        uint32_t c = 0, st = RG_PKT_INVALID;
        if (d.w == RG_KEY_SKIP) st = RG_PKT_REJECTED; // an empty slot: nothing read
        else if ((off & 15u) != 0) st = RG_PKT_UNALIGNED;
        else if (len >= 4 && off <= a.buf_len && len <= a.buf_len - off) { // inside [buf, buf + buf_len), no wrap
            const uint32_t t = *reinterpret_cast<const uint32_t *>(a.buf + off);
            if (t == 1u) c = len == kInitLen ? 1u : 0u;
            else if (t == 2u) c = len == kRespLen ? 2u : 0u;
            else if (t == 3u) c = len == kCookieLen ? 3u : 0u;
            else if (t == 4u) c = 4u; // framing verdicts stay the receive's own
        }
        a.cls[i] = (uint8_t)c;
        if (c == 0) {
            a.pos[i] = RG_KEY_SKIP;
            a.status[i] = (uint8_t)st; // the verdict last
        }
        return one_of(c);
    }
};

// The rank walk: a listed datagram takes row `rank` of its list while the list has room.
struct Place {
    DemuxArgs a;
    __device__ __forceinline__ ListCounts item(uint64_t i) const { return one_of(a.cls[i]); }
    __device__ __forceinline__ void emit(uint64_t i, const ListCounts &v, const ListCounts &ex) const {
        if ((v.hs | v.ck | v.data) == 0) return; // answered by the count walk
        const uint32_t k = v.hs ? ex.hs : v.ck ? ex.ck : ex.data;
        const uint32_t cap = v.hs ? a.cap_hs : v.ck ? a.cap_ck : a.cap_data;
        if (k >= cap) { // dropped, like a full socket buffer; cls[i] keeps the type
            a.pos[i] = RG_KEY_SKIP;
            a.status[i] = RG_PKT_FULL;
            return;
        }
        uint4 d = a.desc[i];
        d.w = 0; // key_idx: any value but RG_KEY_SKIP reads the same to the chains
        if (v.hs) {
            const bool init = d.z == kInitLen; // the count walk listed 148 bytes only as type 1, 92 only as type 2
            a.hs_desc[k] = d;
            a.init_desc[k] = init ? d : inert_row();
            a.resp_desc[k] = init ? inert_row() : d;
            put_addr(a.hs_addrs, k, a.addrs + 3ull * i);
        } else if (v.ck) {
            a.ck_desc[k] = d;
        } else {
            a.data_desc[k] = d;
            put_addr(a.data_addrs, k, a.addrs + 3ull * i);
        }
        a.pos[i] = k;
        a.status[i] = RG_PKT_PENDING; // the verdict is the chain's
    }
    __device__ __forceinline__ void total(const ListCounts &all) const {
        a.counts[0] = min(all.hs, a.cap_hs);
        a.counts[1] = min(all.ck, a.cap_ck);
        a.counts[2] = min(all.data, a.cap_data);
        a.counts[3] = all.hs;
        a.counts[4] = all.ck;
        a.counts[5] = all.data;
    }
};

// one lane per row index: every row of every list beyond its count becomes the inert row
__global__ __launch_bounds__(256) void demux_pad_kernel(DemuxArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < a.cap_hs && r >= a.counts[0]) {
        a.hs_desc[r] = inert_row();
        a.init_desc[r] = inert_row();
        a.resp_desc[r] = inert_row();
        put_addr(a.hs_addrs, r, nullptr);
    }
    if (r < a.cap_ck && r >= a.counts[1]) a.ck_desc[r] = inert_row();
    if (r < a.cap_data && r >= a.counts[2]) {
        a.data_desc[r] = inert_row();
        put_addr(a.data_addrs, r, nullptr);
    }
}

// ------------------------------------------------------------ the way back
struct VerdictArgs {
    const uint8_t *cls; // [n]
    const uint32_t *pos; // [n]
    const uint8_t *filter, *init, *finish; // [cap_hs] or nullptr
    const uint8_t *cookie;                 // [cap_ck] or nullptr
    const uint8_t *data;                   // [cap_data] or nullptr
    uint32_t cap_hs, cap_ck, cap_data;
    uint8_t *status; // [n]
    uint32_t n;
};

__global__ __launch_bounds__(256) void demux_verdict_kernel(VerdictArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    if (a.status[i] != RG_PKT_PENDING) return;
    const uint32_t c = a.cls[i], k = a.pos[i];
    uint32_t st = RG_PKT_PENDING;
    if (c == 1u || c == 2u) {
        const uint8_t *own = c == 1u ? a.init : a.finish;
        if (k < a.cap_hs && a.filter) {
            st = a.filter[k];
            if (st == RG_PKT_OK) st = own ? own[k] : (uint32_t)RG_PKT_PENDING;
        }
    } else if (c == 3u) {
        if (k < a.cap_ck && a.cookie) st = a.cookie[k];
    } else if (c == 4u) {
        if (k < a.cap_data && a.data) st = a.data[k];
    }
    if (st != RG_PKT_PENDING) a.status[i] = (uint8_t)st;
}

struct DemuxLayout {
    AggLayout agg; // ListCounts sums of the datagrams' tiles
    uint64_t total;
};
DemuxLayout demux_layout(uint64_t n) {
    DemuxLayout L{};
    if (n > 0xFFFFFFFFull) return L; // total = 0
    WorkspaceCursor ws;
    L.agg.take_agg(ws, n, sizeof(ListCounts));
    L.total = ws.total();
    return L;
}

} // namespace
} // namespace rg

using namespace rg::host;

extern "C" size_t rg_demux_workspace_size(size_t n) { return (size_t)rg::demux_layout(n).total; }

extern "C" int rg_demux_batch_dev(rg_ctx *ctx, const rg_pkt_desc *desc, const rg_src_addr *addrs, size_t n,
                                  const uint8_t *buf, size_t buf_len, const rg_demux_lists *lists, uint8_t *status,
                                  uint8_t *cls, uint32_t *pos, uint32_t *counts, void *workspace, size_t workspace_len,
                                  void *stream) {
    const char *what = "demux";
    if (!ctx) return set_err(RG_EINVAL, "null context");
    if (n == 0) return RG_OK;
    if (!desc || !addrs || !buf || !lists || !status || !cls || !pos || !counts || !workspace || n > 0xFFFFFFFFull)
        return bad(what, "bad args");
    const rg_demux_lists &l = *lists;
    if ((l.cap_hs && (!l.hs_desc || !l.hs_addrs || !l.init_desc || !l.resp_desc)) || (l.cap_ck && !l.ck_desc) ||
        (l.cap_data && (!l.data_desc || !l.data_addrs)))
        return bad(what, "a list with a capacity and a null array");
    if (misaligned(desc, 16) || misaligned(l.hs_desc, 16) || misaligned(l.init_desc, 16) ||
        misaligned(l.resp_desc, 16) || misaligned(l.ck_desc, 16) || misaligned(l.data_desc, 16) ||
        misaligned(l.hs_addrs, 8) || misaligned(l.data_addrs, 8) || misaligned(buf, 4) || misaligned(pos, 4) ||
        misaligned(counts, 4))
        return bad(what, "descriptor arrays must be 16-byte, rg_src_addr rows 8-byte, buf and the word arrays 4-byte aligned");
    const rg::DemuxLayout L = rg::demux_layout(n);
    int rc = check_workspace(what, addrs, workspace, workspace_len, L.total); // addrs: 8-byte aligned
    if (rc) return rc;
    rg::DeviceGuard dg_;
    rc = check_ctx(ctx);
    if (rc) return rc;
    rg::DemuxArgs a{};
    a.desc = reinterpret_cast<const uint4 *>(desc);
    a.addrs = reinterpret_cast<const uint64_t *>(addrs);
    a.buf = buf;
    a.buf_len = buf_len;
    a.hs_desc = reinterpret_cast<uint4 *>(l.hs_desc);
    a.init_desc = reinterpret_cast<uint4 *>(l.init_desc);
    a.resp_desc = reinterpret_cast<uint4 *>(l.resp_desc);
    a.hs_addrs = reinterpret_cast<uint64_t *>(l.hs_addrs);
    a.ck_desc = reinterpret_cast<uint4 *>(l.ck_desc);
    a.data_desc = reinterpret_cast<uint4 *>(l.data_desc);
    a.data_addrs = reinterpret_cast<uint64_t *>(l.data_addrs);
    a.cap_hs = l.cap_hs;
    a.cap_ck = l.cap_ck;
    a.cap_data = l.cap_data;
    a.status = status;
    a.cls = cls;
    a.pos = pos;
    a.counts = counts;
    hipStream_t st = (hipStream_t)stream;
    rg::compact(rg::Classify{a}, rg::Place{a}, (uint32_t)n,
                rg::Agg<rg::ListCounts>(static_cast<uint8_t *>(workspace), L.agg), st);
    const uint32_t cap = std::max(a.cap_hs, std::max(a.cap_ck, a.cap_data));
    if (cap) hipLaunchKernelGGL(rg::demux_pad_kernel, lanes(cap), kWg, 0, st, a);
    RG_HIP(hipGetLastError(), what);
    return RG_OK;
}

extern "C" int rg_demux_verdict_batch_dev(rg_ctx *ctx, const uint8_t *cls, const uint32_t *pos, size_t n,
                                          const uint8_t *hs_filter_status, const uint8_t *init_status,
                                          const uint8_t *finish_status, uint32_t cap_hs, const uint8_t *cookie_status,
                                          uint32_t cap_ck, const uint8_t *data_status, uint32_t cap_data,
                                          uint8_t *status, void *stream) {
    const char *what = "demux verdict";
    if (!ctx) return set_err(RG_EINVAL, "null context");
    if (n == 0) return RG_OK;
    if (!cls || !pos || !status || n > 0xFFFFFFFFull) return bad(what, "bad args");
    if (misaligned(pos, 4)) return bad(what, "pos must be 4-byte aligned");
    rg::DeviceGuard dg_;
    const int rc = check_ctx(ctx);
    if (rc) return rc;
    rg::VerdictArgs a{};
    a.cls = cls;
    a.pos = pos;
    a.filter = hs_filter_status;
    a.init = init_status;
    a.finish = finish_status;
    a.cookie = cookie_status;
    a.data = data_status;
    a.cap_hs = cap_hs;
    a.cap_ck = cap_ck;
    a.cap_data = cap_data;
    a.status = status;
    a.n = (uint32_t)n;
    hipLaunchKernelGGL(rg::demux_verdict_kernel, lanes(n), kWg, 0, (hipStream_t)stream, a);
    RG_HIP(hipGetLastError(), what);
    return RG_OK;
}
