// rg_timers.hip -- the transport timers of the resident path kept on the device: which sessions owe a keepalive
// and which peers owe a new handshake is decided on the stream that sends and receives, and comes out as the
// arrays the resident send and the initiator chain take.  The reference does this in Sessions::turn
// (rustyguard-core/src/time.rs:42-140, tick_timers) over a heap of timer entries that send_message
// (lib.rs:564-570), decrypt_packet (lib.rs:664-669) and handle_handshake_resp (handshake.rs:218-222) push.
//
//   rg_timer_arm_batch_dev        behind an install: the row's RekeyAttempt entry set or cleared, its flags cleared
//   rg_timer_note_send_batch_dev  behind a send: a packet past REKEY_AFTER_MESSAGES makes the entry due at once
//   rg_timer_note_recv_batch_dev  behind a receive: a packet on a session silent for KEEPALIVE_TIMEOUT flags it
//   rg_timer_turn_dev             tick_timers over the whole table -> (keepalive rows, rekey peers, gate, counts)
//
// One rg_session_timer row per key-table row holds what the heap holds for a transport session.  The turn equals
// an in-order loop (include/rg_aead.h has it) with nothing decided by the order the lanes arrive in.  Its kernels:
//   clear    one lane per peer: want_ka[p] = want_rk[p] = 0, the lists and the gate all padding, the counts zero
//   row      one lane per live row: the pending flag and a due entry are taken off the row; what they ask for goes
//            to want_ka[p] / want_rk[p], the same value from every row of the peer
//   compact  rg_grouped.h's count / carry / rank over the peers, PeerWants in both walks: (keepalive, rekey) of
//            each peer, both counts in one 64-bit sum; ka_slots_out[rank] = the peer's current row,
//            rekey_peers_out[rank] = the peer, rekey_gate_out[rank] = RG_PKT_OK; the totals go to counts_out
// The row kernel writes timers only and the peer kernels read the tables only, so every decision sees the state
// before the call.
//
// The entry points' host side is here too (rg_session.hip's precedent).  All scratch is the caller's; nothing is
// allocated, waited for or kept in the context.
#include "rg_host.h"
#include "rg_grouped.h"

namespace rg {
namespace {

constexpr uint64_t kKeepaliveNs = RG_KEEPALIVE_TIMEOUT_NS;
constexpr uint64_t kRekeyAfterNs = RG_REKEY_AFTER_TIME_NS;
constexpr uint64_t kRejectAfterNs = RG_REJECT_AFTER_TIME_NS;

constexpr uint64_t kOneKa = 1ull, kOneRk = 1ull << 32; // one sum: keepalives in the low word, rekeys in the high

// rg_session_timer as the kernels take it: word 0 rekey_at_ns, word 1 flags (low half) and pad
__device__ __forceinline__ uint64_t *timer_row(uint64_t *timers, uint32_t r) { return timers + 2ull * r; }
__device__ __forceinline__ uint32_t *timer_flags(uint64_t *timers, uint32_t r) {
    return reinterpret_cast<uint32_t *>(timers + 2ull * r + 1);
}

// ------------------------------------------------------- the three notes
struct NoteArgs {
    uint64_t *timers;           // [nkeys][2]
    const uint64_t *send_state; // [nkeys][3]; note_recv only
    uint32_t nkeys;
    const uint32_t *rows;     // [n]
    const uint8_t *gate;      // [n]; arm: or nullptr
    const uint8_t *rekey_out; // [n]; note_send only
    const uint64_t *now_ns;   // arm: or nullptr when rekey_after_ns == 0
    uint64_t rekey_after_ns;  // arm only
    uint32_t n;
};

__global__ __launch_bounds__(256) void timer_arm_kernel(NoteArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    if (a.gate && a.gate[i] != RG_PKT_OK) return;
    const uint32_t r = a.rows[i];
    if (r >= a.nkeys) return;
    uint64_t *t = timer_row(a.timers, r);
    t[1] = 0; // flags, pad
    t[0] = a.rekey_after_ns ? *a.now_ns + a.rekey_after_ns : 0; // the same value from every lane that names r
}

__global__ __launch_bounds__(256) void timer_note_send_kernel(NoteArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    if (a.gate[i] != RG_PKT_OK || a.rekey_out[i] == 0) return;
    const uint32_t r = a.rows[i];
    if (r >= a.nkeys) return;
    const uint64_t now = *a.now_ns;
    uint64_t *t = timer_row(a.timers, r);
    const uint64_t at = t[0]; // the row as it stood or `now` from another lane of this call: the row ends the same
    if (at == 0 || at > now) t[0] = now;
}

__global__ __launch_bounds__(256) void timer_note_recv_kernel(NoteArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    if (a.gate[i] != RG_PKT_OK) return;
    const uint32_t r = a.rows[i];
    if (r >= a.nkeys) return;
    if (a.send_state[3ull * r + 2] + kKeepaliveNs < *a.now_ns) // wrapping, strict
        atomicOr(timer_flags(a.timers, r), RG_TIMER_KEEPALIVE_PENDING);
}

// ---------------------------------------------------------------- the turn
struct TurnArgs {
    uint64_t *timers;           // [nkeys][2]
    const uint64_t *send_state; // [nkeys][3]
    const uint32_t *slot_peer;  // [nkeys]
    const uint32_t *peer_slot;  // [npeers]
    uint32_t nkeys, npeers;
    const uint64_t *now_ns;
    uint32_t *want_ka, *want_rk; // [npeers]
    uint32_t *ka_slots_out, *rekey_peers_out; // [npeers]
    uint8_t *rekey_gate_out;                  // [npeers]
    uint32_t *counts_out;                     // [2]
};

// one lane per peer: nothing wanted, both lists and the gate all padding, the counts zero
__global__ __launch_bounds__(256) void timer_clear_kernel(TurnArgs a) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p == 0) a.counts_out[0] = a.counts_out[1] = 0;
    if (p >= a.npeers) return;
    a.want_ka[p] = 0;
    a.want_rk[p] = 0;
    a.ka_slots_out[p] = RG_KEY_SKIP;
    a.rekey_peers_out[p] = RG_PEER_NONE;
    a.rekey_gate_out[p] = RG_PKT_REJECTED;
}

__global__ __launch_bounds__(256) void timer_row_kernel(TurnArgs a) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.nkeys) return;
    const uint32_t p = a.slot_peer[r];
    if (p == RG_PEER_NONE || p >= a.npeers) return; // a free row is not touched
    const uint64_t now = *a.now_ns;
    const uint64_t *s = a.send_state + 3ull * r;
    uint64_t *t = timer_row(a.timers, r);
    const uint64_t at = t[0];
    const uint32_t flags = *timer_flags(a.timers, r);
    if (flags & RG_TIMER_KEEPALIVE_PENDING) {
        *timer_flags(a.timers, r) = flags & ~RG_TIMER_KEEPALIVE_PENDING;
        if (s[2] + kKeepaliveNs < now) a.want_ka[p] = 1; // should_keepalive
    }
    if (at != 0 && at < now) {
        t[0] = 0; // the entry is popped
        if (s[1] + kRekeyAfterNs < now || s[0] >= RG_REKEY_AFTER_MESSAGES) a.want_rk[p] = 1; // should_rekey
    }
}

// The pass of rg_grouped.h's compact over the peers: what peer p puts on the two lists, kOneKa and / or kOneRk,
// and where its ranks send it.
struct PeerWants {
    TurnArgs a;
    __device__ __forceinline__ uint64_t item(uint64_t pos) const {
        const uint32_t p = (uint32_t)pos;
        uint64_t w = a.want_rk[p] ? kOneRk : 0;
        const uint32_t c = a.peer_slot[p];
        if (a.want_ka[p] && c < a.nkeys && a.slot_peer[c] == p) {
            const uint64_t *s = a.send_state + 3ull * c;
            if (!(s[1] + kRejectAfterNs < *a.now_ns || s[0] >= RG_REJECT_AFTER_MESSAGES)) w |= kOneKa; // should_reject
        }
        return w;
    }
    __device__ __forceinline__ void emit(uint64_t pos, uint64_t w, uint64_t ex) const {
        const uint32_t p = (uint32_t)pos, ka = (uint32_t)ex, rk = (uint32_t)(ex >> 32);
        if ((w & kOneKa) && ka < a.npeers) a.ka_slots_out[ka] = a.peer_slot[p]; // its current row
        if ((w & kOneRk) && rk < a.npeers) {
            a.rekey_peers_out[rk] = p;
            a.rekey_gate_out[rk] = RG_PKT_OK;
        }
    }
    __device__ __forceinline__ void total(uint64_t all) const {
        a.counts_out[0] = (uint32_t)all;
        a.counts_out[1] = (uint32_t)(all >> 32);
    }
};

struct TimerLayout {
    uint64_t want; // [2][npeers] u32: want_ka, want_rk
    AggLayout agg; // u64 sums of the peers' tiles
    uint64_t total;
};
TimerLayout timer_layout(uint64_t nkeys, uint64_t npeers) {
    TimerLayout L{};
    if (nkeys > 0xFFFFFFFFull || npeers > 0xFFFFFFFFull) return L; // total = 0
    WorkspaceCursor ws;
    L.want = ws.take(2 * npeers * 4);
    L.agg.take_agg(ws, npeers, 8);
    L.total = ws.total();
    return L;
}

} // namespace
} // namespace rg

using namespace rg::host;

namespace {
// the three notes behind their kernels: a carries the kernel's arrays
template <class Kernel>
int note(const char *what, Kernel kernel, rg_ctx *ctx, rg_session_timer *timers, rg::NoteArgs a, size_t n,
         bool args_ok, void *stream) {
    rg::DeviceGuard dg_;
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!args_ok || !a.rows || (a.nkeys && !timers) || n > 0xFFFFFFFFull) return bad(what, "bad args");
    if (misaligned(timers, 8) || misaligned(a.send_state, 8) || misaligned(a.now_ns, 8) || misaligned(a.rows, 4))
        return bad(what, "timers, send_state and now_ns must be 8-byte and the row array 4-byte aligned");
    a.timers = reinterpret_cast<uint64_t *>(timers);
    a.n = (uint32_t)n;
    hipLaunchKernelGGL(kernel, lanes(n), kWg, 0, (hipStream_t)stream, a);
    RG_HIP(hipGetLastError(), what);
    return RG_OK;
}
} // namespace

extern "C" size_t rg_timer_workspace_size(size_t nkeys, size_t npeers) {
    return (size_t)rg::timer_layout(nkeys, npeers).total;
}

extern "C" int rg_timer_arm_batch_dev(rg_ctx *ctx, rg_session_timer *timers, uint32_t nkeys, const uint32_t *rows,
                                      const uint8_t *gate, size_t n, const uint64_t *now_ns, uint64_t rekey_after_ns,
                                      void *stream) {
    rg::NoteArgs a{};
    a.nkeys = nkeys;
    a.rows = rows;
    a.gate = gate;
    a.now_ns = now_ns;
    a.rekey_after_ns = rekey_after_ns;
    return note("timer arm", rg::timer_arm_kernel, ctx, timers, a, n, now_ns || !rekey_after_ns, stream);
}

extern "C" int rg_timer_note_send_batch_dev(rg_ctx *ctx, rg_session_timer *timers, uint32_t nkeys,
                                            const uint32_t *slots, const uint8_t *status, const uint8_t *rekey_out,
                                            size_t n, const uint64_t *now_ns, void *stream) {
    rg::NoteArgs a{};
    a.nkeys = nkeys;
    a.rows = slots;
    a.gate = status;
    a.rekey_out = rekey_out;
    a.now_ns = now_ns;
    return note("timer note send", rg::timer_note_send_kernel, ctx, timers, a, n, status && rekey_out && now_ns, stream);
}

extern "C" int rg_timer_note_recv_batch_dev(rg_ctx *ctx, rg_session_timer *timers, const rg_send_state *send_state,
                                            uint32_t nkeys, const uint32_t *key_idx, const uint8_t *status, size_t n,
                                            const uint64_t *now_ns, void *stream) {
    rg::NoteArgs a{};
    a.send_state = reinterpret_cast<const uint64_t *>(send_state);
    a.nkeys = nkeys;
    a.rows = key_idx;
    a.gate = status;
    a.now_ns = now_ns;
    return note("timer note recv", rg::timer_note_recv_kernel, ctx, timers, a, n,
                status && now_ns && (send_state || !nkeys), stream);
}

extern "C" int rg_timer_turn_dev(rg_ctx *ctx, const rg_session_tables *tables, rg_session_timer *timers,
                                 const uint64_t *now_ns, uint32_t *ka_slots_out, uint32_t *rekey_peers_out,
                                 uint8_t *rekey_gate_out, uint32_t *counts_out, void *workspace, size_t workspace_len,
                                 void *stream) {
    const char *what = "timer turn";
    rg::DeviceGuard dg_;
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if (!tables || !now_ns || !counts_out || !workspace) return bad(what, "bad args");
    rg::TurnArgs a{};
    a.nkeys = tables->nkeys;
    a.npeers = tables->npeers;
    // of the tables the turn reads slot_peer, send_state and peer_slot
    if ((a.nkeys && (!tables->slot_peer || !tables->send_state || !timers)) ||
        (a.npeers && (!tables->peer_slot || !ka_slots_out || !rekey_peers_out || !rekey_gate_out)))
        return bad(what, "a null array");
    if (misaligned(tables->send_state, 8) || misaligned(now_ns, 8) || misaligned(tables->slot_peer, 4) ||
        misaligned(tables->peer_slot, 4) || misaligned(ka_slots_out, 4) || misaligned(rekey_peers_out, 4) ||
        misaligned(counts_out, 4))
        return bad(what, "send_state and now_ns must be 8-byte and the word arrays 4-byte aligned");
    const rg::TimerLayout L = rg::timer_layout(a.nkeys, a.npeers);
    rc = check_workspace(what, timers, workspace, workspace_len, L.total);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    a.timers = reinterpret_cast<uint64_t *>(timers);
    a.send_state = reinterpret_cast<const uint64_t *>(tables->send_state);
    a.slot_peer = tables->slot_peer;
    a.peer_slot = tables->peer_slot;
    a.now_ns = now_ns;
    a.want_ka = reinterpret_cast<uint32_t *>(ws + L.want);
    a.want_rk = a.want_ka + a.npeers;
    a.ka_slots_out = ka_slots_out;
    a.rekey_peers_out = rekey_peers_out;
    a.rekey_gate_out = rekey_gate_out;
    a.counts_out = counts_out;
    hipLaunchKernelGGL(rg::timer_clear_kernel, lanes(a.npeers ? a.npeers : 1), kWg, 0, st, a);
    if (a.npeers == 0) { // a row of such a table has no peer below npeers: nothing else is touched
        RG_HIP(hipGetLastError(), what);
        return RG_OK;
    }
    if (a.nkeys) hipLaunchKernelGGL(rg::timer_row_kernel, lanes(a.nkeys), kWg, 0, st, a);
    const rg::PeerWants wants{a};
    rg::compact(wants, wants, a.npeers, rg::Agg<uint64_t>(ws, L.agg), st);
    RG_HIP(hipGetLastError(), what);
    return RG_OK;
}
