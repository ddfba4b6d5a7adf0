// rg_sessions.cpp -- the host-side transport session layer of include/rg_aead.h (EncryptionKey /
// DecryptionKey / AntiReplay, rustyguard-crypto/src/prim.rs:376-437,
// rustyguard-utils/src/anti_replay.rs:1-64, rustyguard-core/src/lib.rs:249-681): the host anti-replay
// window, the session table, its host-frame send and receive, and its device half (the *_dev session calls).
#include <algorithm>
#include <cstdio>
#include <new>
#include <unordered_map>

#include "rg_host.h"

using namespace rg::host;
using rg::DeviceGuard;

extern "C" {

// ------------------------------------------------------------- AntiReplay
// rustyguard-utils/src/anti_replay.rs:1-64 with usize = u64:
// BITMAP_LEN = 32 words, REDUNDANT_BIT_SHIFTS = 6, WINDOW_SIZE = 2048 - 64.
void rg_antireplay_init(rg_antireplay *r) {
    if (r) memset(r, 0, sizeof *r);
}

int rg_antireplay_would_accept(const rg_antireplay *r, uint64_t n) {
    if (n > r->last) return 1;
    const uint64_t d = r->last - n;
    if (d >= RG_REPLAY_WINDOW) return 0;
    const uint64_t index = n >> 6, shift = n & 63;
    return ((r->bitmap[index & 31] >> shift) & 1) == 0;
}

void rg_antireplay_mark_seen(rg_antireplay *r, uint64_t n) {
    const uint64_t index = n >> 6, shift = n & 63;
    if (n > r->last) {
        const uint64_t next_index = (r->last >> 6) + 1;
        if (index > next_index && index - next_index > 32) {
            memset(r->bitmap, 0, sizeof r->bitmap); // the window skipped entirely ahead
        } else {
            for (uint64_t i = next_index; i <= index; ++i) r->bitmap[i & 31] = 0;
        }
        r->last = n;
    }
    r->bitmap[index & 31] |= 1ull << shift;
}

} // extern "C"

// ----------------------------------------------------------- session table
namespace {
struct Session {
    bool used = false;
    uint32_t local_id = 0, remote_id = 0;
    uint64_t send_ctr = 0;
    rg_antireplay replay{};
    // rustyguard-core/src/lib.rs:185-191: when the session started and last sent, whether a
    // keepalive is already scheduled; plus the peer endpoint learned from authenticated packets
    uint64_t started = 0, sent = 0;
    bool keepalive_pending = false;
    bool has_endpoint = false; // sessions without a peer (rg_sessions_insert) keep their own endpoint
    uint64_t endpoint = 0;
    uint32_t peer = RG_PEER_NONE;
};
// PeerState's endpoint (rustyguard-core/src/lib.rs:160-181, :670-671): shared by the peer's sessions
struct Peer {
    bool has_endpoint = false;
    uint64_t endpoint = 0;
};
constexpr uint64_t kNsPerSec = 1000000000ull;
constexpr uint64_t kKeepaliveTimeout = 10 * kNsPerSec; // KEEPALIVE_TIMEOUT, lib.rs:70
constexpr uint64_t kRejectAfterTime = 180 * kNsPerSec; // REJECT_AFTER_TIME, lib.rs:67

// Device half of the session table for rg_send_batch_dev / rg_recv_batch_dev: mirrors of the key
// rows, the receivers and a receiver-id -> recv-row table, refreshed before the next device call
// after a session change (once the device work that reads them has drained).
struct SendStage { // one device send in flight per stage; two stages alternate
    DevBuf d_desc, d_kidx, d_ctr;
    HostBuf h_kidx, h_ctr;
    Event ev; // the stage's seal has consumed its buffers
};
struct RecvStage { // the device receive between rg_recv_batch_dev and rg_recv_batch_dev_finish
    DevBuf d_rdesc, d_ctr, d_key, d_idx, d_udesc, d_uctr, d_ustatus;
    HostBuf h_status, h_ctr, h_key, h_fix, h_idx;
    Event ev_meta, ev_done;
    bool pending = false;
    size_t n = 0;
    hipStream_t st = nullptr;
    uint8_t *buf = nullptr, *status = nullptr;
    size_t buf_len = 0;
};
struct SessDev {
    SecretBuf keys; // send rows [0, cap), recv rows [cap, 2 cap)
    HostBuf h_keys; // their pinned staging copy (zeroed when freed)
    Event ev_keys;  // the staging copy's upload is done
    DevBuf recv, rx;
    uint32_t rx_cap = 0;
    bool dirty = true;
    SendStage send[2];
    int send_next = 0;
    RecvStage rv;
};
} // namespace

struct rg_sessions {
    rg_ctx *ctx = nullptr;
    rg_group *group = nullptr; // host-frame batches on every context of the group (ctx = its first)
    uint32_t cap = 0;
    uint64_t now = 0; // Sessions' clock (state.now, advanced by turn: lib.rs:396-413), nanoseconds
    std::vector<Session> s;
    std::vector<uint8_t> keys;       // rows [0,cap): send keys, [cap,2cap): recv keys
    std::vector<uint32_t> receivers; // remote ids for send rows
    std::unordered_map<uint32_t, uint32_t> by_local;
    std::unordered_map<uint32_t, Peer> peers;
    SessDev dev;
};

namespace {

// The send rule for one packet of session `slot`, shared by rg_send_batch and rg_send_batch_dev: an
// unused slot is RG_PKT_REJECTED (no transport session: the caller must handshake), as is a session
// past REJECT_AFTER_MESSAGES or REJECT_AFTER_TIME (should_reject / should_expire, lib.rs:204-209);
// otherwise the packet takes the session's counter (EncryptionKey::encrypt, prim.rs:387-388), the
// session has sent now (force_encrypt, lib.rs:285), and rekey tells whether it should rekey
// (lib.rs:564-570).  A packet that is not RG_PKT_OK has no side effect and counter 0.
// len: the payload length where the host knows it (rg_send_batch), else nullptr.  A known length with
// len % 16 != 0 is RG_PKT_INVALID here, before a counter is taken (force_encrypt's padding assert,
// lib.rs:273-277).  rg_send_batch_dev's lengths live on the device: such a packet takes its counter
// here and the seal kernel then reports it RG_PKT_INVALID.
struct SendVerdict {
    uint8_t status = RG_PKT_REJECTED;
    uint64_t ctr = 0;
    bool rekey = false;
};
// (inlined into both loops: as a call it cost rg_send_batch_dev 0.5 ns per packet, 0.5 ms on 1 Mi packets)
[[gnu::always_inline]] inline SendVerdict send_step(rg_sessions *s, uint32_t slot, const uint32_t *len) {
    SendVerdict v;
    if (slot >= s->cap || !s->s[slot].used) return v;
    Session &x = s->s[slot];
    if (len && *len % 16 != 0) {
        v.status = RG_PKT_INVALID;
        return v;
    }
    if (x.send_ctr >= RG_REJECT_AFTER_MESSAGES || x.started + kRejectAfterTime < s->now) return v;
    v.status = RG_PKT_OK;
    v.ctr = x.send_ctr++;
    x.sent = s->now;
    v.rekey = x.send_ctr >= RG_REKEY_AFTER_MESSAGES;
    return v;
}

// the table's host-frame calls: on every context of its group, or on its one context
int table_seal_host(rg_sessions *s, const uint32_t *receivers, uint32_t nkeys, const rg_pkt_desc *d,
                    const uint64_t *ctr, size_t n, uint8_t *buf, size_t buf_len, uint8_t *status) {
    return s->group ? rg_seal_batch_host_multi(s->group, s->keys.data(), receivers, nkeys, d, ctr, n, buf, buf_len, status)
                    : rg_seal_batch_host(s->ctx, s->keys.data(), receivers, nkeys, d, ctr, n, buf, buf_len, status);
}
int table_open_host(rg_sessions *s, const rg_pkt_desc *d, size_t n, uint8_t *buf, size_t buf_len, uint8_t *status) {
    return s->group ? rg_open_batch_host_multi(s->group, s->keys.data(), 2 * s->cap, d, n, buf, buf_len, status, nullptr)
                    : rg_open_batch_host(s->ctx, s->keys.data(), 2 * s->cap, d, n, buf, buf_len, status, nullptr);
}

// The in-order tail of DecryptionKey::decrypt (prim.rs:414-437) and decrypt_packet
// (rustyguard-core/src/lib.rs:655-679) for packet i of session `slot`, whose GPU verdict
// `st` is RG_PKT_OK or RG_PKT_DECRYPT_ERR: would_accept comes first (Error::Rejected, also
// for a frame too short or with a bad tag), then the AEAD's verdict; an accepted packet
// advances the window (only authenticated counters do, RFC 6479 §3.4.3), may move the
// endpoint (whitepaper §6.5) and may ask for a keepalive.  *undo: the GPU left plaintext in
// a frame the reference would not have decrypted.
uint8_t replay_step(rg_sessions *s, uint32_t slot, uint64_t ctr, uint8_t st, const uint64_t *src, size_t i,
                    uint8_t *fl, bool *undo) {
    Session &x = s->s[slot];
    *undo = false;
    *fl = 0;
    if (!rg_antireplay_would_accept(&x.replay, ctr)) {
        *undo = st == RG_PKT_OK;
        return RG_PKT_REJECTED;
    }
    if (st != RG_PKT_OK) return st;
    rg_antireplay_mark_seen(&x.replay, ctr);
    uint8_t f = RG_RECV_AUTHENTICATED;
    if (x.sent + kKeepaliveTimeout < s->now && !x.keepalive_pending) {
        x.keepalive_pending = true;
        f |= RG_RECV_KEEPALIVE;
    }
    if (src) { // the peer's endpoint moves (the session's own without a peer)
        if (x.peer != RG_PEER_NONE) {
            Peer &p = s->peers[x.peer];
            p.endpoint = src[i];
            p.has_endpoint = true;
        } else {
            x.endpoint = src[i];
            x.has_endpoint = true;
        }
    }
    *fl = f;
    return RG_PKT_OK;
}

// every device batch of the table has finished with its tables (bounded waits)
int drain_device_work(rg_sessions *s) {
    SessDev &D = s->dev;
    const uint32_t ms = s->ctx->wait_ms;
    for (auto &g : D.send) RG_WAIT(g.ev.get(), ms, "session tables in use");
    RG_WAIT(D.rv.ev_meta.get(), ms, "session tables in use");
    RG_WAIT(D.rv.ev_done.get(), ms, "session tables in use");
    RG_WAIT(D.ev_keys.get(), ms, "session key upload");
    return RG_OK;
}

// refresh the device mirrors after session changes, on the call's stream st (the key rows are
// rewritten in place; a regrow wipes the old rows behind their last readers, SecretBuf).  The key rows
// go through a pinned staging copy whose upload is fenced by an event (round 5 synchronised the caller's
// stream here, waiting for all of the caller's queued work: ADVICE r5); the next refresh waits for that
// event before it rewrites the staging copy.  Inside a stream capture the refresh would be replayed by the
// graph from a staging copy that changes under it: refused.
int sync_tables(rg_sessions *s, hipStream_t st) {
    SessDev &D = s->dev;
    if (!D.dirty) return RG_OK;
    if (capturing(st))
        return set_err(RG_EDEVICE, "session tables changed since the last device call: refresh them (one device "
                                   "call) outside the stream capture");
    int rc = drain_device_work(s);
    if (rc) return rc;
    RG_HIP(D.ev_keys.ensure(), "session key event");
    RG_HIP(D.keys.reserve(s->keys.size(), st), "alloc session keys");
    D.h_keys.secret = true;
    RG_HIP(D.h_keys.reserve(s->keys.size()), "alloc session key staging");
    memcpy(D.h_keys.p, s->keys.data(), s->keys.size());
    RG_HIP(hipMemcpyAsync(D.keys.p, D.h_keys.p, s->keys.size(), hipMemcpyHostToDevice, st), "H2D session keys");
    RG_HIP(hipEventRecord(D.ev_keys.get(), st), "session key event");
    RG_HIP(D.recv.reserve((size_t)s->cap * 4), "alloc session receivers");
    RG_HIP(hipMemcpy(D.recv.p, s->receivers.data(), (size_t)s->cap * 4, hipMemcpyHostToDevice),
           "H2D session receivers");
    std::vector<uint32_t> ids, rows;
    for (uint32_t i = 0; i < s->cap; ++i)
        if (s->s[i].used) {
            ids.push_back(s->s[i].local_id);
            rows.push_back(s->cap + i); // the session's recv-key row
        }
    uint32_t rx_cap = 2;
    while (rx_cap < 2 * ids.size()) rx_cap <<= 1;
    std::vector<rg_rx_entry> t(rx_cap);
    rc = rg_rx_table_build(ids.data(), rows.data(), ids.size(), t.data(), rx_cap);
    if (rc) return rc;
    RG_HIP(D.rx.reserve((size_t)rx_cap * sizeof(rg_rx_entry)), "alloc rx table");
    RG_HIP(hipMemcpy(D.rx.p, t.data(), (size_t)rx_cap * sizeof(rg_rx_entry), hipMemcpyHostToDevice), "H2D rx table");
    D.rx_cap = rx_cap;
    D.dirty = false;
    return RG_OK;
}

} // namespace

extern "C" {

int rg_sessions_create(rg_ctx *ctx, uint32_t capacity, rg_sessions **out) {
    if (!ctx || !out || capacity == 0 || capacity > (1u << 24)) return set_err(RG_EINVAL, "sessions: bad args");
    rg_sessions *s = new (std::nothrow) rg_sessions();
    if (!s) return set_err(RG_ENOMEM, "alloc sessions");
    s->ctx = ctx;
    s->cap = capacity;
    s->s.resize(capacity);
    s->keys.assign((size_t)capacity * 64, 0);
    s->receivers.assign((size_t)capacity * 2, 0);
    *out = s;
    return RG_OK;
}

int rg_sessions_create_group(rg_group *g, uint32_t capacity, rg_sessions **out) {
    if (!g || g->ctx.empty()) return set_err(RG_EINVAL, "sessions: null group");
    int rc = rg_sessions_create(g->ctx[0], capacity, out);
    if (rc == RG_OK) (*out)->group = g;
    return rc;
}

// Only what has an order is spelled out; the staging buffers and events go with their owners' destructors
// (the pinned key copy zeroed first), while the context's device is still selected.
void rg_sessions_destroy(rg_sessions *s) {
    if (!s) return;
    std::fill(s->keys.begin(), s->keys.end(), 0); // zeroize, as prim.rs:227-231 / lib.rs:216-228
    DeviceGuard dg_;
    (void)hipSetDevice(s->ctx->device);
    (void)drain_device_work(s);
    (void)s->dev.keys.release(s->ctx->gen_stream); // zeroed behind its last readers, then freed
    (void)hipStreamSynchronize(s->ctx->gen_stream);
    delete s;
}

int rg_sessions_insert(rg_sessions *s, uint32_t local_id, uint32_t remote_id, const uint8_t send_key[32],
                       const uint8_t recv_key[32]) {
    return rg_sessions_insert_peer(s, local_id, remote_id, send_key, recv_key, RG_PEER_NONE);
}

int rg_sessions_insert_peer(rg_sessions *s, uint32_t local_id, uint32_t remote_id, const uint8_t send_key[32],
                            const uint8_t recv_key[32], uint32_t peer) {
    if (!s || !send_key || !recv_key) return set_err(RG_EINVAL, "insert: bad args");
    if (s->dev.rv.pending) return set_err(RG_EINVAL, "insert: a device receive batch is pending");
    if (s->by_local.count(local_id)) return set_err(RG_EINVAL, "insert: local id in use");
    for (uint32_t i = 0; i < s->cap; ++i) {
        Session &x = s->s[i];
        if (x.used) continue;
        x = Session();
        x.used = true;
        x.local_id = local_id;
        x.remote_id = remote_id;
        x.started = x.sent = s->now; // handshake.rs:119-124, :215-216
        x.peer = peer;
        if (peer != RG_PEER_NONE) (void)s->peers[peer]; // the record exists from the peer's first session
        memcpy(&s->keys[(size_t)i * 32], send_key, 32);
        memcpy(&s->keys[((size_t)s->cap + i) * 32], recv_key, 32);
        s->receivers[i] = remote_id;
        s->by_local[local_id] = i;
        s->dev.dirty = true;
        return (int)i;
    }
    return set_err(RG_EFULL, "insert: table full");
}

int rg_sessions_remove(rg_sessions *s, uint32_t slot) {
    if (!s || slot >= s->cap || !s->s[slot].used) return set_err(RG_EINVAL, "remove: bad slot");
    if (s->dev.rv.pending) return set_err(RG_EINVAL, "remove: a device receive batch is pending");
    s->dev.dirty = true;
    s->by_local.erase(s->s[slot].local_id);
    s->s[slot] = Session();
    memset(&s->keys[(size_t)slot * 32], 0, 32);
    memset(&s->keys[((size_t)s->cap + slot) * 32], 0, 32);
    return RG_OK;
}

int rg_sessions_lookup(const rg_sessions *s, uint32_t local_id) {
    if (!s) return set_err(RG_EINVAL, "lookup: null");
    auto it = s->by_local.find(local_id);
    return it == s->by_local.end() ? RG_ENOTFOUND : (int)it->second;
}

uint64_t rg_sessions_send_counter(const rg_sessions *s, uint32_t slot) {
    if (!s || slot >= s->cap) return 0;
    return s->s[slot].send_ctr;
}

int rg_sessions_set_send_counter(rg_sessions *s, uint32_t slot, uint64_t counter) {
    if (!s || slot >= s->cap || !s->s[slot].used) return set_err(RG_EINVAL, "set_counter: bad slot");
    s->s[slot].send_ctr = counter;
    return RG_OK;
}

rg_antireplay *rg_sessions_replay(rg_sessions *s, uint32_t slot) {
    if (!s || slot >= s->cap) return nullptr;
    return &s->s[slot].replay;
}

void rg_sessions_set_time(rg_sessions *s, uint64_t now_ns) {
    if (s) s->now = now_ns;
}

int rg_peer_endpoint(const rg_sessions *s, uint32_t peer, uint64_t *src_out) {
    if (!s || !src_out || peer == RG_PEER_NONE) return set_err(RG_EINVAL, "peer_endpoint: bad args");
    auto it = s->peers.find(peer);
    if (it == s->peers.end() || !it->second.has_endpoint) return RG_ENOTFOUND;
    *src_out = it->second.endpoint;
    return RG_OK;
}

int rg_sessions_endpoint(const rg_sessions *s, uint32_t slot, uint64_t *src_out) {
    if (!s || slot >= s->cap || !s->s[slot].used || !src_out) return set_err(RG_EINVAL, "endpoint: bad slot");
    const Session &x = s->s[slot];
    if (x.peer != RG_PEER_NONE) return rg_peer_endpoint(s, x.peer, src_out);
    if (!x.has_endpoint) return RG_ENOTFOUND;
    *src_out = x.endpoint;
    return RG_OK;
}

int rg_sessions_keepalive_due(rg_sessions *s, uint32_t slot) {
    if (!s || slot >= s->cap || !s->s[slot].used) return set_err(RG_EINVAL, "keepalive: bad slot");
    Session &x = s->s[slot];
    x.keepalive_pending = false;                     // time.rs:118
    return x.sent + kKeepaliveTimeout < s->now ? 1 : 0; // should_keepalive, lib.rs:201-203
}

int rg_sessions_keepalive(rg_sessions *s, uint32_t slot, uint64_t *dst_out) {
    if (!dst_out) return set_err(RG_EINVAL, "keepalive: null dst");
    const int due = rg_sessions_keepalive_due(s, slot);
    if (due <= 0) return due;
    const int rc = rg_sessions_endpoint(s, slot, dst_out); // peer.endpoint, time.rs:135
    return rc == RG_OK ? 1 : rc;
}

int rg_send_batch(rg_sessions *s, const uint32_t *slots, const rg_pkt_desc *desc, size_t n, uint8_t *buf,
                  size_t buf_len, uint8_t *status, uint8_t *rekey_out) {
    if (!s || !slots || !desc || !buf || !status) return fail_closed(set_err(RG_EINVAL, "send_batch: bad args"), status, n);
    if (n == 0) return RG_OK;
    std::vector<rg_pkt_desc> d(desc, desc + n);
    std::vector<uint64_t> ctr(n, 0);
    std::vector<uint8_t> host_status(n, RG_PKT_OK);
    for (size_t i = 0; i < n; ++i) {
        const SendVerdict v = send_step(s, slots[i], &d[i].len);
        host_status[i] = v.status;
        ctr[i] = v.ctr;
        d[i].key_idx = v.status == RG_PKT_OK ? slots[i] : RG_KEY_SKIP;
        if (rekey_out) rekey_out[i] = v.rekey;
    }
    int rc = table_seal_host(s, s->receivers.data(), s->cap, d.data(), ctr.data(), n, buf, buf_len, status);
    if (rc) return rc;
    for (size_t i = 0; i < n; ++i)
        if (host_status[i] != RG_PKT_OK) status[i] = host_status[i];
    return RG_OK;
}

int rg_recv_batch(rg_sessions *s, const rg_pkt_desc *desc, size_t n, uint8_t *buf, size_t buf_len,
                  uint8_t *status, uint32_t *slots_out) {
    return rg_recv_batch_ex(s, desc, n, buf, buf_len, nullptr, status, slots_out, nullptr);
}

int rg_recv_batch_ex(rg_sessions *s, const rg_pkt_desc *desc, size_t n, uint8_t *buf, size_t buf_len,
                     const uint64_t *src, uint8_t *status, uint32_t *slots_out, uint8_t *flags_out) {
    if (!s || !desc || !buf || !status) return fail_closed(set_err(RG_EINVAL, "recv_batch: bad args"), status, n);
    if (n == 0) return RG_OK;
    std::vector<rg_pkt_desc> d(desc, desc + n);
    std::vector<uint8_t> host_status(n, 0xFF);
    std::vector<uint32_t> slot_of(n, 0xFFFFFFFFu);
    std::vector<uint64_t> ctr(n, 0);
    for (size_t i = 0; i < n; ++i) {
        const uint64_t off = d[i].offset;
        const uint32_t w = d[i].len;
        uint8_t st = 0xFF;
        if (off > buf_len || buf_len - off < w) st = RG_PKT_INVALID;
        else if (((uintptr_t)(buf + off) & 15) != 0) st = RG_PKT_UNALIGNED; // lib.rs:613-615
        else if (w < 4) st = RG_PKT_INVALID;
        else {
            uint32_t type, recv;
            memcpy(&type, buf + off, 4);
            if (type != 4u) st = type - 1u < 3u ? RG_PKT_NOT_DATA : RG_PKT_INVALID; // 1-3: control plane; else lib.rs:627
            else if (w % 16 != 0 || w < 16) st = RG_PKT_INVALID; // message_mut_from
            else {
                memcpy(&recv, buf + off + 4, 4);
                memcpy(&ctr[i], buf + off + 8, 8);
                auto it = s->by_local.find(recv);
                if (it == s->by_local.end()) st = RG_PKT_REJECTED; // lib.rs:646-650
                else {
                    slot_of[i] = it->second;
                    // replay pre-filter with the pre-batch window: a counter rejected now is
                    // rejected by any later window state too (the window only advances)
                    if (!rg_antireplay_would_accept(&s->s[it->second].replay, ctr[i])) st = RG_PKT_REJECTED;
                    else if (w < 32) st = RG_PKT_DECRYPT_ERR; // prim.rs:427-429
                }
            }
        }
        host_status[i] = st;
        d[i].key_idx = st == 0xFF ? s->cap + slot_of[i] : RG_KEY_SKIP;
    }
    int rc = table_open_host(s, d.data(), n, buf, buf_len, status);
    if (rc) { // statuses pending (the open call's fail-closed contract); no packet is flagged either
        if (flags_out) memset(flags_out, 0, n);
        return rc;
    }
    // in-order post-pass (RFC 6479 §3.4.3: only authenticated counters advance the window)
    std::vector<rg_pkt_desc> undo;
    std::vector<uint64_t> undo_ctr;
    if (flags_out) memset(flags_out, 0, n);
    for (size_t i = 0; i < n; ++i) {
        uint8_t st = host_status[i] != 0xFF ? host_status[i] : status[i];
        // a frame that reached the session (GPU verdict, or too short for a tag) takes the
        // in-order window check first: a second copy of a counter accepted earlier in this
        // batch, or one the window has moved past since, is Rejected before decrypting
        // (prim.rs:420-423), and a GPU plaintext there is put back to ciphertext
        if (slot_of[i] != 0xFFFFFFFFu && (st == RG_PKT_OK || st == RG_PKT_DECRYPT_ERR)) {
            uint8_t fl;
            bool back;
            st = replay_step(s, slot_of[i], ctr[i], st, src, i, &fl, &back);
            if (flags_out) flags_out[i] = fl;
            if (back) {
                undo.push_back(rg_pkt_desc{d[i].offset, d[i].len - 32, d[i].key_idx});
                undo_ctr.push_back(ctr[i]);
            }
        }
        status[i] = st;
        if (slots_out) slots_out[i] = slot_of[i];
    }
    if (!undo.empty()) {
        // Re-sealing the plaintext under the same key and nonce reproduces the ciphertext and,
        // since the tag is the MAC of that ciphertext, the frame's own (verified) tag; without
        // receivers the header is not rewritten.  The frame is byte-for-byte what arrived.
        std::vector<uint8_t> st2(undo.size());
        rc = table_seal_host(s, nullptr, 2 * s->cap, undo.data(), undo_ctr.data(), undo.size(), buf, buf_len, st2.data());
        for (uint8_t x : st2)
            if (rc == RG_OK && x != RG_PKT_OK) rc = set_err(RG_EDEVICE, "recv_batch: restoring a replayed frame failed");
        if (rc) { // a failed batch hands nothing up (include/rg_aead.h)
            if (flags_out) memset(flags_out, 0, n);
            return fail_closed(rc, status, n);
        }
    }
    return RG_OK;
}

int rg_send_batch_dev(rg_sessions *s, const uint32_t *slots, const rg_pkt_desc *desc, size_t n, uint8_t *buf,
                      size_t buf_len, uint8_t *status, uint8_t *rekey_out, void *stream) {
    if (!s || !slots || !desc || !buf || !status) return set_err(RG_EINVAL, "send_batch_dev: bad args (status is required)");
    if (s->group) return set_err(RG_EINVAL, "send_batch_dev: a group's table takes host frames (rg_send_batch)");
    if (n > 0xFFFFFFFFull) return set_err(RG_EINVAL, "send_batch_dev: too many packets");
    if (n == 0) return RG_OK;
    DeviceGuard dg_;
    int rc = check_ctx(s->ctx);
    if (rc) return rc;
    rc = claim_stream(s->ctx, static_cast<hipStream_t>(stream)); // before any counter is taken
    if (rc) return rc;
    rc = sync_tables(s, static_cast<hipStream_t>(stream));
    if (rc) return rc;
    SessDev &D = s->dev;
    SendStage &g = D.send[D.send_next];
    RG_HIP(g.ev.ensure(), "send event");
    RG_WAIT(g.ev.get(), s->ctx->wait_ms, "send staging"); // the stage's previous batch has been sealed
    D.send_next ^= 1;
    RG_HIP(g.h_kidx.reserve(n * 4), "alloc send staging");
    RG_HIP(g.h_ctr.reserve(n * 8), "alloc send staging");
    RG_HIP(g.d_kidx.reserve(n * 4), "alloc send key rows");
    RG_HIP(g.d_ctr.reserve(n * 8), "alloc send counters");
    RG_HIP(g.d_desc.reserve(n * sizeof(rg_pkt_desc)), "alloc send descriptors");
    uint32_t *kx = static_cast<uint32_t *>(g.h_kidx.p);
    uint64_t *cx = static_cast<uint64_t *>(g.h_ctr.p);
    // rg_send_batch's session checks, in array order, without the lengths (send_step); a packet without a
    // counter is RG_KEY_SKIP, which the kernel reports RG_PKT_REJECTED
    for (size_t i = 0; i < n; ++i) {
        const SendVerdict v = send_step(s, slots[i], nullptr);
        kx[i] = v.status == RG_PKT_OK ? slots[i] : RG_KEY_SKIP;
        cx[i] = v.ctr;
        if (rekey_out) rekey_out[i] = v.rekey;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    RG_HIP(hipMemcpyAsync(g.d_kidx.p, kx, n * 4, hipMemcpyHostToDevice, st), "H2D send key rows");
    RG_HIP(hipMemcpyAsync(g.d_ctr.p, cx, n * 8, hipMemcpyHostToDevice, st), "H2D send counters");
    auto *bd = static_cast<rg_pkt_desc *>(g.d_desc.p);
    RG_HIP(rg::launch_bind_keys(desc, static_cast<const uint32_t *>(g.d_kidx.p), (uint32_t)n, bd, st), "bind launch");
    rc = rg_seal_batch_dev(s->ctx, static_cast<const uint8_t *>(D.keys.p), static_cast<const uint32_t *>(D.recv.p),
                           s->cap, bd, static_cast<const uint64_t *>(g.d_ctr.p), n, buf, buf_len, status, stream);
    if (rc) return rc;
    RG_HIP(D.keys.use(st), "session keys event");
    RG_HIP(hipEventRecord(g.ev.get(), st), "send event record");
    return RG_OK;
}

int rg_recv_batch_dev(rg_sessions *s, const rg_pkt_desc *desc, size_t n, uint8_t *buf, size_t buf_len,
                      uint8_t *status, void *stream) {
    if (!s || !desc || !buf || !status) return set_err(RG_EINVAL, "recv_batch_dev: bad args");
    if (s->group) return set_err(RG_EINVAL, "recv_batch_dev: a group's table takes host frames (rg_recv_batch_ex)");
    if (n > 0xFFFFFFFFull) return set_err(RG_EINVAL, "recv_batch_dev: too many packets");
    RecvStage &R = s->dev.rv;
    if (R.pending) return set_err(RG_EINVAL, "recv_batch_dev: finish the pending batch first");
    DeviceGuard dg_;
    int rc = check_ctx(s->ctx);
    if (rc) return rc;
    rc = claim_stream(s->ctx, static_cast<hipStream_t>(stream));
    if (rc) return rc;
    rc = sync_tables(s, static_cast<hipStream_t>(stream));
    if (rc) return rc;
    SessDev &D = s->dev;
    RG_HIP(R.ev_meta.ensure(), "recv event");
    RG_HIP(R.ev_done.ensure(), "recv event");
    RG_WAIT(R.ev_done.get(), s->ctx->wait_ms, "recv staging"); // the previous batch's fix-ups are done
    hipStream_t st = static_cast<hipStream_t>(stream);
    // The batch becomes pending only once every buffer is reserved and every step is enqueued: a
    // failure leaves no pending batch (finish then reports none), and work already enqueued is
    // fenced by ev_done, which the next call waits for before it reuses the staging buffers.
    if (n > 0) {
        RG_HIP(R.d_rdesc.reserve(n * sizeof(rg_pkt_desc)), "alloc recv descriptors");
        RG_HIP(R.d_ctr.reserve(n * 8), "alloc recv counters");
        RG_HIP(R.d_key.reserve(n * 4), "alloc recv key rows");
        RG_HIP(R.h_status.reserve(n), "alloc recv staging");
        RG_HIP(R.h_ctr.reserve(n * 8), "alloc recv staging");
        RG_HIP(R.h_key.reserve(n * 4), "alloc recv staging");
        auto fenced = [&](int code) {
            (void)hipEventRecord(R.ev_done.get(), st);
            return code;
        };
        auto *rd = static_cast<rg_pkt_desc *>(R.d_rdesc.p);
        hipError_t e = rg::launch_rx_resolve(desc, (uint32_t)n, buf, buf_len, static_cast<const rg_rx_entry *>(D.rx.p),
                                             D.rx_cap, rd, static_cast<uint32_t *>(R.d_key.p), st);
        if (e != hipSuccess) return fenced(set_err(RG_EDEVICE, "rx resolve launch", e));
        rc = rg_open_batch_dev(s->ctx, static_cast<const uint8_t *>(D.keys.p), 2 * s->cap, rd, n, buf, buf_len, status,
                               static_cast<uint64_t *>(R.d_ctr.p), stream);
        if (rc) return fenced(rc);
        e = D.keys.use(st);
        if (e == hipSuccess) e = hipMemcpyAsync(R.h_status.p, status, n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(R.h_ctr.p, R.d_ctr.p, n * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(R.h_key.p, R.d_key.p, n * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipEventRecord(R.ev_meta.get(), st);
        if (e != hipSuccess) return fenced(set_err(RG_EDEVICE, "recv metadata copies", e));
    }
    R.n = n;
    R.st = st;
    R.buf = buf;
    R.buf_len = buf_len;
    R.status = status;
    R.pending = true;
    return RG_OK;
}

int rg_recv_batch_dev_finish(rg_sessions *s, const uint64_t *src, uint8_t *status_out, uint32_t *slots_out,
                             uint8_t *flags_out) {
    if (!s) return set_err(RG_EINVAL, "recv_batch_dev_finish: null");
    RecvStage &R = s->dev.rv;
    if (!R.pending) return set_err(RG_EINVAL, "recv_batch_dev_finish: no pending batch");
    R.pending = false;
    const size_t n = R.n;
    if (n == 0) return RG_OK;
    DeviceGuard dg_;
    int rc = check_ctx(s->ctx);
    if (rc) return rc;
    RG_WAIT(R.ev_meta.get(), s->ctx->wait_ms, "recv metadata");
    RG_HIP(R.h_fix.reserve(n), "alloc recv staging");
    RG_HIP(R.h_idx.reserve(n * 4), "alloc recv staging");
    const uint8_t *gs = static_cast<const uint8_t *>(R.h_status.p);
    const uint64_t *cx = static_cast<const uint64_t *>(R.h_ctr.p);
    const uint32_t *kx = static_cast<const uint32_t *>(R.h_key.p);
    uint8_t *fx = static_cast<uint8_t *>(R.h_fix.p);
    uint32_t *ix = static_cast<uint32_t *>(R.h_idx.p);
    size_t m = 0, pending = 0;
    bool changed = false;
    for (size_t i = 0; i < n; ++i) {
        uint8_t st = gs[i], fl = 0;
        pending += st == RG_PKT_PENDING; // never reached by the kernel: no replay step, no side effect
        const uint32_t k = kx[i];
        const uint32_t slot = k != RG_KEY_SKIP && k >= s->cap && k < 2 * s->cap ? k - s->cap : 0xFFFFFFFFu;
        if (slot != 0xFFFFFFFFu && (st == RG_PKT_OK || st == RG_PKT_DECRYPT_ERR)) {
            bool back;
            const uint8_t st2 = replay_step(s, slot, cx[i], st, src, i, &fl, &back);
            if (back) ix[m++] = (uint32_t)i;
            changed |= st2 != st;
            st = st2;
        }
        fx[i] = st;
        if (status_out) status_out[i] = st;
        if (slots_out) slots_out[i] = slot;
        if (flags_out) flags_out[i] = fl;
    }
    hipStream_t st = R.st;
    if (changed) RG_HIP(hipMemcpyAsync(R.status, fx, n, hipMemcpyHostToDevice, st), "H2D recv status");
    if (m) {
        // re-seal under the same key and nonce: ciphertext and tag come back byte for byte
        RG_HIP(R.d_idx.reserve(m * 4), "alloc undo list");
        RG_HIP(R.d_udesc.reserve(m * sizeof(rg_pkt_desc)), "alloc undo list");
        RG_HIP(R.d_uctr.reserve(m * 8), "alloc undo list");
        RG_HIP(hipMemcpyAsync(R.d_idx.p, ix, m * 4, hipMemcpyHostToDevice, st), "H2D undo list");
        auto *ud = static_cast<rg_pkt_desc *>(R.d_udesc.p);
        RG_HIP(rg::launch_undo_gather(static_cast<const rg_pkt_desc *>(R.d_rdesc.p),
                                      static_cast<const uint64_t *>(R.d_ctr.p), static_cast<const uint32_t *>(R.d_idx.p),
                                      (uint32_t)m, ud, static_cast<uint64_t *>(R.d_uctr.p), st),
               "undo gather launch");
        RG_HIP(R.d_ustatus.reserve(m), "alloc undo list");
        rc = rg_seal_batch_dev(s->ctx, static_cast<const uint8_t *>(s->dev.keys.p), nullptr, 2 * s->cap, ud,
                               static_cast<const uint64_t *>(R.d_uctr.p), m, R.buf, R.buf_len,
                               static_cast<uint8_t *>(R.d_ustatus.p), st);
        if (rc) return rc;
        RG_HIP(s->dev.keys.use(st), "session keys event");
    }
    RG_HIP(hipEventRecord(R.ev_done.get(), st), "recv event record");
    if (pending) {
        char what[128];
        snprintf(what, sizeof what, "recv_batch_dev_finish: %zu of %zu packets were never finished (RG_PKT_PENDING)",
                 pending, n);
        return set_err(RG_EDEVICE, what);
    }
    return RG_OK;
}

} // extern "C"
