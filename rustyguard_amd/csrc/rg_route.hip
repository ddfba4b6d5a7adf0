// rg_route.hip -- cryptokey routing on the device, batched: the AllowedIPs decisions of the reference's tun
// loop (rustyguard-tun/src/lib.rs).  Outbound, handle_intern (:214-243): peer_net.lookup(&dest) names the peer
// and the packet is zero-padded to a multiple of 16 before send_message.  Inbound, handle_extern (:174-202): a
// decrypted packet whose inner source address is not the opening peer's is dropped.  The table, its builder and
// the lookup are rg_route.h's, one text for host and device.
//
// Kernels, all on the call's stream, one lane per packet in 256-lane workgroups:
//   route_kernel     (rg_route_batch_dev) descriptor checks, the IPv4 rule, lookup(dst), peer -> key row, the
//            zero padding; writes slot, working descriptor, peer and status of every packet
//   check_kernel     (rg_route_check_batch_dev) the IPv4 rule and lookup(src) against the peer of the key row
//            that opened the packet; statuses in place, total_length out
//   routed_overlay   (rg_send_batch_dev_routed) the route's verdicts of the packets it did not route over the
//            resident send's
// The inner packet starts 16-byte aligned.  Inbound a lane reads its first 16 bytes in one load (version, IHL,
// total length, source); outbound the first word and the word at +16 (destination) -- one 128-byte line either
// way -- then at most three table words: latency-bound gathers, nothing shared between lanes, no LDS, no
// atomics.  The padding is a masked rewrite of the packet's last 16-byte chunk, which lies inside
// roundup16(L).  Plain vector loads and stores only.
//
// The entry points' host side is here too (rg_send.hip's precedent), on rg_host.h like the host units.  All
// scratch is the caller's workspace; nothing is allocated, waited for or kept.
#include "rg_device.h"
#include "rg_host.h"
#include "rg_route.h"

namespace rg {
namespace {

struct RouteArgs {
    const uint32_t *table;
    uint64_t table_words;
    const uint32_t *peer_slot; // [npeers]
    uint32_t npeers;
    const rg_pkt_desc *desc; // [n]
    uint32_t n;
    uint8_t *buf;
    uint64_t buf_len;
    uint32_t *peers_out; // [n] or nullptr
    uint32_t *slots_out; // [n]
    rg_pkt_desc *desc_out; // [n]
    uint8_t *status;     // [n]
};

struct CheckArgs {
    const uint32_t *table;
    uint64_t table_words;
    const uint32_t *slot_peer; // [nkeys]
    uint32_t nkeys;
    const rg_pkt_desc *desc;  // [n]
    const uint32_t *key_idx;  // [n]
    uint32_t n;
    const uint8_t *buf;
    uint64_t buf_len;
    uint8_t *status;         // [n]
    uint32_t *inner_len_out; // [n] or nullptr
};

// the frame [off, off + 32 + body) lies in the buffer; no sum of caller's numbers can wrap (body < 2^33)
__device__ __forceinline__ bool frame_fits(uint64_t off, uint64_t body, uint64_t buf_len) {
    const uint64_t need = body + 32u;
    return need <= buf_len && off <= buf_len - need;
}

__device__ __forceinline__ uint32_t bswap32(uint32_t x) {
    return (x << 24) | ((x & 0xFF00u) << 8) | ((x >> 8) & 0xFF00u) | (x >> 24);
}

__global__ __launch_bounds__(256) void route_kernel(RouteArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const rg_pkt_desc d = a.desc[i];
    const uint32_t L = d.len;
    const uint64_t padded = ((uint64_t)L + 15u) & ~15ull;
    uint8_t st;
    uint32_t peer = RG_PEER_NONE, slot = RG_KEY_SKIP;
    if (d.offset & 15u) st = RG_PKT_UNALIGNED;
    else if (!frame_fits(d.offset, padded, a.buf_len)) st = RG_PKT_INVALID;
    else {
        uint8_t *inner = a.buf + d.offset + 16;
        st = RG_PKT_INVALID;
        // L >= 20 before a byte of the packet is read: the first word and the word at +16 lie inside it
        if (L >= 20u && route::ipv4_total_length(*reinterpret_cast<const uint32_t *>(inner), L)) {
            const uint32_t dst = bswap32(*reinterpret_cast<const uint32_t *>(inner + 16));
            const uint32_t p = route::lookup(a.table, a.table_words, dst);
            st = RG_PKT_UNROUTABLE;
            if (p != RG_PEER_NONE && p < a.npeers) {
                peer = p;
                slot = a.peer_slot[p];
                st = slot == RG_KEY_SKIP ? RG_PKT_REJECTED : RG_PKT_OK;
            }
        }
        if (st == RG_PKT_OK && (L & 15u)) {
            // bytes [L, roundup16(L)) of the packet's last chunk to zero, the first L % 16 kept
            uint4 *chunk = reinterpret_cast<uint4 *>(inner + (L & ~15u));
            uint4 v = *chunk;
            const uint32_t keep = L & 15u;
            uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t kb = keep > 4 * k ? keep - 4 * k : 0u; // bytes of word k that stay
                w[k] &= kb >= 4u ? 0xFFFFFFFFu : (1u << (8u * kb)) - 1u;
            }
            *chunk = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    rg_pkt_desc out = d;
    out.key_idx = slot;
    if (st == RG_PKT_OK) out.len = (uint32_t)padded; // L >= 20 here and the frame fits: no wrap
    if (a.peers_out) a.peers_out[i] = peer;
    a.slots_out[i] = slot;
    a.desc_out[i] = out;
    a.status[i] = st;
}

__global__ __launch_bounds__(256) void check_kernel(CheckArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    uint8_t st = a.status[i];
    uint32_t inner_len = 0;
    if (st == RG_PKT_OK) {
        const rg_pkt_desc d = a.desc[i];
        const uint32_t W = d.len;
        if (W != 32u) { // a keepalive stays RG_PKT_OK, inner length 0
            st = RG_PKT_INVALID;
            // a frame the receive accepted is aligned, in the buffer and W >= 32; checked again, since this call
            // reads what the descriptor names
            if (!(d.offset & 15u) && W >= 32u && frame_fits(d.offset, (uint64_t)W - 32u, a.buf_len) && W - 32u >= 20u) {
                const uint4 head = *reinterpret_cast<const uint4 *>(a.buf + d.offset + 16);
                const uint32_t total = route::ipv4_total_length(head.x, W - 32u);
                if (total) {
                    const uint32_t p = route::lookup(a.table, a.table_words, bswap32(head.w));
                    const uint32_t k = a.key_idx[i];
                    if (p != RG_PEER_NONE && k < a.nkeys && a.slot_peer[k] == p) {
                        st = RG_PKT_OK;
                        inner_len = total;
                    } else {
                        st = RG_PKT_UNROUTABLE;
                    }
                }
            }
        }
    }
    a.status[i] = st;
    if (a.inner_len_out) a.inner_len_out[i] = inner_len;
}

// a packet the route did not route keeps the route's verdict; every other one the resident send's
__global__ __launch_bounds__(256) void routed_overlay_kernel(const uint8_t *verdict, uint8_t *status, uint32_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint8_t v = verdict[i];
    if (v != RG_PKT_OK) status[i] = v;
}

// Workspace of rg_send_batch_dev_routed (WorkspaceCursor, rg_internal.h): the route's arrays, then the resident
// send's workspace.  total == 0: the batch is too large.  Every term is non-decreasing in n and in nkeys.
struct RoutedLayout {
    uint64_t wdesc;   // [n] rg_pkt_desc: the route's working descriptors; = 0
    uint64_t slots;   // [n] u32
    uint64_t verdict; // [n] u8: the route's statuses
    uint64_t send;    // the resident send's workspace
    uint64_t send_len;
    uint64_t total;
};
RoutedLayout routed_layout(uint64_t n, uint32_t nkeys) {
    RoutedLayout L{};
    if (n > 0xFFFFFFFFull) return L;
    L.send_len = rg_send_workspace_size((size_t)n, nkeys);
    if (L.send_len == 0) return L;
    WorkspaceCursor ws;
    L.wdesc = ws.take(n * sizeof(rg_pkt_desc));
    L.slots = ws.take(n * 4);
    L.verdict = ws.take(n);
    L.send = ws.take(L.send_len);
    L.total = ws.total();
    return L;
}

} // namespace
} // namespace rg

extern "C" size_t rg_route_table_words(const rg_route_prefix *p, uint32_t np) { return rg::route::table_words(p, np); }

extern "C" int rg_route_table_build(const rg_route_prefix *p, uint32_t np, uint32_t *table, size_t cap_words) {
    const int rc = rg::route::table_build(p, np, table, cap_words);
    if (rc == RG_EINVAL) return rg::host::set_err(rc, "route table: null pointer, prefix_len > 32 or peer > 0x7FFFFFFF");
    if (rc == RG_EFULL) return rg::host::set_err(rc, "route table: cap_words smaller than rg_route_table_words");
    return rc;
}

extern "C" uint32_t rg_route_lookup(const uint32_t *table, size_t table_words, const uint8_t addr[4]) {
    if (!table || !addr || table_words < rg::route::kRootWords) return RG_PEER_NONE;
    return rg::route::lookup(table, table_words, rg::route::addr_be(addr));
}

extern "C" size_t rg_route_workspace_size(size_t n, uint32_t nkeys) {
    return (size_t)rg::routed_layout(n, nkeys).total;
}

extern "C" int rg_route_batch_dev(rg_ctx *ctx, const uint32_t *table, size_t table_words, const uint32_t *peer_slot,
                                  uint32_t npeers, const rg_pkt_desc *desc, size_t n, uint8_t *buf, size_t buf_len,
                                  uint32_t *peers_out, uint32_t *slots_out, rg_pkt_desc *desc_out, uint8_t *status,
                                  void *stream) {
    using namespace rg::host;
    rg::DeviceGuard dg_;
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!table || !peer_slot || !desc || !buf || !slots_out || !desc_out || !status || n > 0xFFFFFFFFull ||
        table_words < rg::route::kRootWords || misaligned(buf, 16))
        return set_err(RG_EINVAL, "route: bad args");
    const rg::RouteArgs a{table, table_words, peer_slot, npeers, desc, (uint32_t)n, buf, buf_len,
                          peers_out, slots_out, desc_out, status};
    hipLaunchKernelGGL(rg::route_kernel, lanes(n), kWg, 0, (hipStream_t)stream, a);
    RG_HIP(hipGetLastError(), "route launch");
    return RG_OK;
}

extern "C" int rg_route_check_batch_dev(rg_ctx *ctx, const uint32_t *table, size_t table_words,
                                        const uint32_t *slot_peer, uint32_t nkeys, const rg_pkt_desc *desc,
                                        const uint32_t *key_idx, size_t n, const uint8_t *buf, size_t buf_len,
                                        uint8_t *status, uint32_t *inner_len_out, void *stream) {
    using namespace rg::host;
    rg::DeviceGuard dg_;
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!table || !slot_peer || !desc || !key_idx || !buf || !status || n > 0xFFFFFFFFull ||
        table_words < rg::route::kRootWords || misaligned(buf, 16))
        return set_err(RG_EINVAL, "route check: bad args");
    const rg::CheckArgs a{table, table_words, slot_peer, nkeys, desc, key_idx, (uint32_t)n, buf, buf_len,
                          status, inner_len_out};
    hipLaunchKernelGGL(rg::check_kernel, lanes(n), kWg, 0, (hipStream_t)stream, a);
    RG_HIP(hipGetLastError(), "route check launch");
    return RG_OK;
}

extern "C" int rg_send_batch_dev_routed(rg_ctx *ctx, const uint8_t *keys, const uint32_t *receivers, uint32_t nkeys,
                                        rg_send_state *state, const uint32_t *table, size_t table_words,
                                        const uint32_t *peer_slot, uint32_t npeers, const rg_pkt_desc *desc, size_t n,
                                        const uint64_t *now_ns, uint8_t *buf, size_t buf_len, uint32_t *peers_out,
                                        uint8_t *status, uint64_t *counters_out, uint8_t *rekey_out, void *workspace,
                                        size_t workspace_len, void *stream) {
    using namespace rg::host;
    rg::DeviceGuard dg_;
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    // everything the resident send would refuse is refused here, before the route kernel is enqueued
    if (!keys || !receivers || nkeys == 0 || !state || !table || !peer_slot || !desc || !buf || !status || !workspace ||
        n > 0xFFFFFFFFull || table_words < rg::route::kRootWords || misaligned(buf, 16))
        return set_err(RG_EINVAL, "send routed: bad args");
    const rg::RoutedLayout L = rg::routed_layout(n, nkeys);
    rc = check_workspace("send routed", state, workspace, workspace_len, L.total);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = claim_stream(ctx, st); // before a byte is padded
    if (rc) return rc;
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    rg_pkt_desc *wdesc = reinterpret_cast<rg_pkt_desc *>(ws + L.wdesc);
    uint32_t *slots = reinterpret_cast<uint32_t *>(ws + L.slots);
    uint8_t *verdict = ws + L.verdict;
    const rg::RouteArgs a{table, table_words, peer_slot, npeers, desc, (uint32_t)n, buf, buf_len,
                          peers_out, slots, wdesc, verdict};
    hipLaunchKernelGGL(rg::route_kernel, lanes(n), kWg, 0, st, a);
    RG_HIP(hipGetLastError(), "send routed: route launch");
    rc = rg_send_batch_dev_resident(ctx, keys, receivers, nkeys, state, slots, wdesc, n, now_ns, buf, buf_len, status,
                                    counters_out, rekey_out, ws + L.send, (size_t)L.send_len, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(rg::routed_overlay_kernel, lanes(n), kWg, 0, st, (const uint8_t *)verdict, status,
                       (uint32_t)n);
    RG_HIP(hipGetLastError(), "send routed: overlay launch");
    return RG_OK;
}
