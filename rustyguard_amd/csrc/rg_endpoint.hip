// rg_endpoint.hip -- PeerState.endpoint of the resident path kept on the device: where a peer's packets last came
// from, moved only by what was authenticated, and read back as the destination array of the next send.  The
// reference moves it in decrypt_packet (rustyguard-core/src/lib.rs:659-671) and handle_handshake_resp
// (handshake.rs:205) and reads it in send_message (lib.rs:550-553) and tick_timers (time.rs:67, :135).
//
//   rg_endpoint_note_recv_batch_dev    behind the resident receive: the peer of key_idx[i]'s row
//   rg_endpoint_note_peers_batch_dev   the same with the peer named directly
//   rg_endpoint_note_finish_batch_dev  behind the finish call: the peer of pend_idx_out[i]'s pending row
//   rg_endpoint_gate_batch_dev         in front of a send: slots -> (slots or RG_KEY_SKIP, destination addresses)
//   rg_endpoint_peers_batch_dev        the same by peer: peers -> (peers or RG_PEER_NONE, destination addresses)
//
// The three notes equal an in-order loop (include/rg_aead.h has it) in which the last eligible item of a peer in
// array order wins, with nothing decided by the order the lanes arrive in.  One kernel pair serves all three; they
// differ in how item i names its peer (NoteArgs::map).
//   claim   one lane per item: atomicMax(claim[p], i + 1), reduced within the wave first.  Lanes ascend with i, so
//           of the eligible lanes that name one peer the highest lane carries the highest index and issues the one
//           atomic; up to kWaveRounds peers of a wave are served that way, one per round, and the lanes left after
//           that (a wave of many peers) issue their own.  A batch of one session is one atomic a wave.
//   commit  one lane per item: the lane whose i + 1 is the claim stores the row in two 16-byte pieces and then puts
//           the claim word back to zero.  No index is taken from the claim word: it is only compared.
// The claim array is zero between calls: the caller zeroes it once, and every call leaves it as it found it, so the
// cost follows n and not npeers and no fill is enqueued.  The two gathers are one lane per item with no atomics.
//
// The entry points' host side is here too (rg_timers.hip's precedent).  Every argument rule is answered before the
// device is selected.  Nothing is allocated, waited for or kept in the context.
#include "rg_host.h"

namespace rg {
namespace {

constexpr int kWaveRounds = 4; // peers of one wave that get a single atomic each

static_assert(sizeof(rg_endpoint) == 32 && sizeof(rg_src_addr) == 24, "layouts");

// word 4 of an rg_endpoint row: port_le in the low half, `set` in the high half; words 5..7 are `zero`
__device__ __forceinline__ bool endpoint_set(const uint4 &hi) { return (hi.x >> 16) != 0; }

// ------------------------------------------------------------ the three notes
struct NoteArgs {
    uint4 *endpoints;      // [npeers][2]
    uint32_t npeers;
    const uint32_t *idx;   // [n]: key_idx, peer_idx or pend_idx_out
    const uint32_t *map;   // [nmap]: slot_peer or pend_peers; nullptr: idx names the peer
    uint32_t nmap;
    const uint8_t *status; // [n]
    const uint64_t *src;   // [n][3]: rg_src_addr as three words
    uint32_t *claim;       // [npeers], zero between calls
    uint32_t n;
};

// the peer item i moves, RG_PEER_NONE (never below npeers) when it moves none; every index is compared first
__device__ __forceinline__ uint32_t note_peer(const NoteArgs &a, uint32_t i) {
    if (a.status[i] != RG_PKT_OK) return RG_PEER_NONE;
    uint32_t p = a.idx[i];
    if (a.map) {
        if (p >= a.nmap) return RG_PEER_NONE;
        p = a.map[p];
    }
    return p < a.npeers ? p : RG_PEER_NONE;
}

__global__ __launch_bounds__(256) void endpoint_claim_kernel(NoteArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t p = i < a.n ? note_peer(a, i) : RG_PEER_NONE;
    bool todo = p != RG_PEER_NONE;
    for (int round = 0; round < kWaveRounds; ++round) {
        const uint64_t pending = __ballot(todo);
        if (pending == 0) return; // the whole wave
        const uint32_t lp = __shfl(p, __ffsll((unsigned long long)pending) - 1);
        const bool mine = todo && p == lp;
        const uint64_t same = __ballot(mine);
        if (mine) {
            if ((same >> lane) == 1ull) atomicMax(&a.claim[p], i + 1); // the group's highest lane: its highest index
            todo = false;
        }
    }
    if (todo) atomicMax(&a.claim[p], i + 1);
}

__global__ __launch_bounds__(256) void endpoint_commit_kernel(NoteArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t p = note_peer(a, i);
    if (p == RG_PEER_NONE) return;
    // the peer's other lanes read their own i + 1's absence here, before or after the winner's reset: never equal
    if (a.claim[p] != i + 1) return;
    const uint64_t *s = a.src + 3ull * i;
    const uint64_t w0 = s[0], w1 = s[1], w2 = s[2];
    uint4 *row = a.endpoints + 2ull * p;
    row[0] = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
    row[1] = make_uint4(((uint32_t)w2 & 0xFFFFu) | 0x10000u, 0u, 0u, 0u); // port_le, set = 1, zero
    a.claim[p] = 0;
}

// ------------------------------------------------------------ the two gathers
struct GatherArgs {
    const uint4 *endpoints; // [npeers][2]
    uint32_t npeers;
    const uint32_t *idx;    // [n]: slots or peer_idx
    const uint32_t *map;    // [nmap]: slot_peer; nullptr: idx names the peer
    uint32_t nmap;
    uint32_t *idx_out;      // [n]; may be idx
    uint64_t *dst_out;      // [n][3]: rg_src_addr as three words
    uint32_t none;          // RG_KEY_SKIP or RG_PEER_NONE
    uint32_t n;
};

__global__ __launch_bounds__(256) void endpoint_gather_kernel(GatherArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t x = a.idx[i];
    uint32_t p = x;
    bool ok = true;
    if (a.map) {
        ok = x < a.nmap;
        if (ok) p = a.map[x];
    }
    ok = ok && p < a.npeers;
    uint64_t w0 = 0, w1 = 0, w2 = 0;
    if (ok) {
        const uint4 hi = a.endpoints[2ull * p + 1];
        ok = endpoint_set(hi);
        if (ok) {
            const uint4 lo = a.endpoints[2ull * p];
            w0 = lo.x | ((uint64_t)lo.y << 32);
            w1 = lo.z | ((uint64_t)lo.w << 32);
            w2 = hi.x & 0xFFFFu; // port_le; pad zero
        }
    }
    uint64_t *d = a.dst_out + 3ull * i;
    d[0] = w0;
    d[1] = w1;
    d[2] = w2;
    a.idx_out[i] = ok ? x : a.none; // the verdict last
}

} // namespace
} // namespace rg

using namespace rg::host;

namespace {
// the three notes behind their kernel pair: a carries how item i names its peer
int note(const char *what, rg_ctx *ctx, rg_endpoint *endpoints, uint32_t npeers, rg::NoteArgs a, bool mapped,
         const uint8_t *status, const rg_src_addr *src, size_t n, uint32_t *claim, void *stream) {
    if (!ctx) return set_err(RG_EINVAL, "null context");
    if (n == 0) return RG_OK;
    if (!endpoints || !a.idx || (mapped && !a.map) || !status || !src || !claim || n > 0xFFFFFFFFull)
        return bad(what, "bad args");
    if (misaligned(endpoints, 16) || misaligned(src, 8) || misaligned(a.idx, 4) || misaligned(a.map, 4) ||
        misaligned(claim, 4))
        return bad(what, "endpoints must be 16-byte, src 8-byte and the word arrays 4-byte aligned");
    rg::DeviceGuard dg_;
    const int rc = check_ctx(ctx);
    if (rc) return rc;
    a.endpoints = reinterpret_cast<uint4 *>(endpoints);
    a.npeers = npeers;
    a.status = status;
    a.src = reinterpret_cast<const uint64_t *>(src);
    a.claim = claim;
    a.n = (uint32_t)n;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rg::endpoint_claim_kernel, lanes(n), kWg, 0, st, a);
    hipLaunchKernelGGL(rg::endpoint_commit_kernel, lanes(n), kWg, 0, st, a);
    RG_HIP(hipGetLastError(), what);
    return RG_OK;
}

int gather(const char *what, rg_ctx *ctx, const rg_endpoint *endpoints, uint32_t npeers, rg::GatherArgs a, bool mapped,
           size_t n, rg_src_addr *dst_out, void *stream) {
    if (!ctx) return set_err(RG_EINVAL, "null context");
    if (n == 0) return RG_OK;
    if (!endpoints || !a.idx || (mapped && !a.map) || !a.idx_out || !dst_out || n > 0xFFFFFFFFull)
        return bad(what, "bad args");
    if (misaligned(endpoints, 16) || misaligned(dst_out, 8) || misaligned(a.idx, 4) || misaligned(a.map, 4) ||
        misaligned(a.idx_out, 4))
        return bad(what, "endpoints must be 16-byte, dst_out 8-byte and the word arrays 4-byte aligned");
    rg::DeviceGuard dg_;
    const int rc = check_ctx(ctx);
    if (rc) return rc;
    a.endpoints = reinterpret_cast<const uint4 *>(endpoints);
    a.npeers = npeers;
    a.dst_out = reinterpret_cast<uint64_t *>(dst_out);
    a.n = (uint32_t)n;
    hipLaunchKernelGGL(rg::endpoint_gather_kernel, lanes(n), kWg, 0, (hipStream_t)stream, a);
    RG_HIP(hipGetLastError(), what);
    return RG_OK;
}
} // namespace

extern "C" int rg_endpoint_note_recv_batch_dev(rg_ctx *ctx, rg_endpoint *endpoints, uint32_t npeers,
                                               const uint32_t *slot_peer, uint32_t nkeys, const uint32_t *key_idx,
                                               const uint8_t *status, const rg_src_addr *src, size_t n,
                                               uint32_t *claim, void *stream) {
    rg::NoteArgs a{};
    a.idx = key_idx;
    a.map = slot_peer;
    a.nmap = nkeys;
    return note("endpoint note recv", ctx, endpoints, npeers, a, true, status, src, n, claim, stream);
}

extern "C" int rg_endpoint_note_peers_batch_dev(rg_ctx *ctx, rg_endpoint *endpoints, uint32_t npeers,
                                                const uint32_t *peer_idx, const uint8_t *status,
                                                const rg_src_addr *src, size_t n, uint32_t *claim, void *stream) {
    rg::NoteArgs a{};
    a.idx = peer_idx;
    return note("endpoint note peers", ctx, endpoints, npeers, a, false, status, src, n, claim, stream);
}

extern "C" int rg_endpoint_note_finish_batch_dev(rg_ctx *ctx, rg_endpoint *endpoints, uint32_t npeers,
                                                 const uint32_t *pend_idx_out, const uint32_t *pend_peers,
                                                 uint32_t npending, const uint8_t *status, const rg_src_addr *src,
                                                 size_t n, uint32_t *claim, void *stream) {
    rg::NoteArgs a{};
    a.idx = pend_idx_out;
    a.map = pend_peers;
    a.nmap = npending;
    return note("endpoint note finish", ctx, endpoints, npeers, a, true, status, src, n, claim, stream);
}

extern "C" int rg_endpoint_gate_batch_dev(rg_ctx *ctx, const rg_endpoint *endpoints, uint32_t npeers,
                                          const uint32_t *slot_peer, uint32_t nkeys, const uint32_t *slots, size_t n,
                                          uint32_t *slots_out, rg_src_addr *dst_out, void *stream) {
    rg::GatherArgs a{};
    a.idx = slots;
    a.map = slot_peer;
    a.nmap = nkeys;
    a.idx_out = slots_out;
    a.none = RG_KEY_SKIP;
    return gather("endpoint gate", ctx, endpoints, npeers, a, true, n, dst_out, stream);
}

extern "C" int rg_endpoint_peers_batch_dev(rg_ctx *ctx, const rg_endpoint *endpoints, uint32_t npeers,
                                           const uint32_t *peer_idx, size_t n, uint32_t *peers_out,
                                           rg_src_addr *dst_out, void *stream) {
    rg::GatherArgs a{};
    a.idx = peer_idx;
    a.idx_out = peers_out;
    a.none = RG_PEER_NONE;
    return gather("endpoint peers", ctx, endpoints, npeers, a, false, n, dst_out, stream);
}
