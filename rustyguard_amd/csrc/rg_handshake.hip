// rg_handshake.hip -- both ends of the Noise IKpsk2 handshake for a batch, one message per lane:
//
//   x25519_kernel              CryptoPrimatives::x25519 / x25519_pubkey (prim.rs:79-80, :159-177)
//   handshake_init_kernel      decrypt_handshake_init (rustyguard-crypto/src/lib.rs:346-384) and
//                              Config::get_peer_idx (rustyguard-core/src/handshake.rs:75-82)
//   handshake_resp_kernel      encrypt_handshake_resp (lib.rs:386-433) and HandshakeState::split(false)
//                              (prim.rs:299-313)
//   handshake_initiate_kernel  encrypt_handshake_init (lib.rs:287-344), the cryptography of new_handshake
//                              (handshake.rs:260-325)
//   handshake_finish_kernel    decrypt_handshake_resp (lib.rs:435-465) and split(true) behind the session
//                              lookup of handle_handshake_resp (handshake.rs:140-230); it reads the pending
//                              rows and claims them by atomicMin of the message index
//   handshake_commit_kernel    the verdict of the finish: the lowest claiming message of a pending row gets
//                              RG_PKT_OK and wipes the row (hs.zeroize()), every other claimant is rejected
//
// What lives where: this file holds each kernel's line of the Noise pattern (which token follows which, under
// which keys), the layout of its messages and rows, and the entry points' host side (on rg_host.h, like
// rg_cookie.hip's).  rg_noise.h holds what the lines are made of: the symmetric state (Noise: mix_hash,
// mix_chain, mix_key, mix_key_and_hash, split, encrypt_and_hash, decrypt_and_hash), the fields' AEAD, mac1 and
// mac2, the frame preamble and the row helpers.  rg_blake2s.h holds the hash, HMAC and HKDF under them, and
// rg_x25519.h the ladder.
//
// The cost is the X25519 ladder of rg_x25519.h: two per initiation consumed, three per response built, three
// per initiation built, two per response consumed, ~2800 field multiplications each; everything else (some
// fifty BLAKE2s compressions, a few ChaCha20 blocks) is noise beside it.  So the kernels are laid out for code
// size, not for the hash: the ladders of one kernel share one call site (a `#pragma unroll 1` loop over the
// kernel's Diffie-Hellman steps, with the work that follows each step chosen by the loop count, which is
// public; a step that failed falls through the rest of the loop, which has a single exit), and the HKDF steps
// share b2s_hkdf's.  Workgroups are one wave, so that a batch of a thousand messages still spreads over
// sixteen CUs.
//
// Constant time: no branch and no address depends on a private key, a shared secret, a chaining key or an
// AEAD key.  Branches follow the descriptor, the gate, the loop counts and the verdicts that the status array
// publishes anyway (a zero shared secret, a failed tag, an unknown static key); tag and key comparisons are
// OR-folds over all their words.  Nothing derived from a key is written to global memory except the rows
// the interface defines, and a row whose message fails is written as zeros.
#include "rg_host.h"
#include "rg_noise.h"
#include "rg_x25519.h"

namespace rg {
namespace {

constexpr int kHsWG = 64; // one wave per workgroup

// ------------------------------------------------------------------ X25519
struct X25519Args {
    const uint32_t *scalars; // [n][8]
    const uint32_t *points;  // [n][8] or nullptr = the base point
    uint32_t *out;           // [n][8]
    uint8_t *status;         // [n]
    uint32_t n;
};

__global__ __launch_bounds__(kHsWG) void x25519_kernel(X25519Args a) {
    const uint32_t i = blockIdx.x * kHsWG + threadIdx.x;
    if (i >= a.n) return;
    uint32_t k[8], u[8] = {9, 0, 0, 0, 0, 0, 0, 0}, o[8];
    load8(a.scalars + 8ull * i, k);
    if (a.points) load8(a.points + 8ull * i, u);
    const uint32_t nz = x25519_words(k, u, o);
#pragma unroll
    for (int w = 0; w < 8; ++w) a.out[8ull * i + w] = o[w];
    a.status[i] = nz ? RG_PKT_OK : RG_PKT_KEYEXCHANGE;
}

// ----------------------------------------------------------- init consume
struct HsInitArgs {
    const uint32_t *own;   // rg_hs_static: private key, public key
    const uint32_t *peers; // [npeers] rg_hs_peer rows of 24 words
    uint32_t npeers;
    const uint32_t *table; // [cap] peer rows, 0xFFFFFFFF = empty
    uint32_t cap;
    const rg_pkt_desc *desc;
    const uint8_t *gate; // [n] or nullptr
    const uint8_t *buf;
    uint64_t buf_len;
    uint4 *results; // [n] rows of 8 uint4
    uint8_t *status;
    uint32_t n;
};

// -> e, es, s, ss, {timestamp}, read
__global__ __launch_bounds__(kHsWG) void handshake_init_kernel(HsInitArgs a) {
    __shared__ uint32_t s_hash[8]; // the transcript hash after mix_hash(own public key): the same for every message
    if (threadIdx.x == 0) {
        uint32_t chain[8], hash[8], pk[12] = {};
        Noise ns{chain, hash};
        load8(a.own + 8, pk);
        ns.init();
        ns.mix_hash(pk, 8);
#pragma unroll
        for (int w = 0; w < 8; ++w) s_hash[w] = ns.hash[w];
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * kHsWG + threadIdx.x;
    if (i >= a.n) return;
    const rg_pkt_desc d = a.desc[i];
    uint32_t st = frame_verdict(d, a.gate ? a.gate[i] : (uint32_t)RG_PKT_OK, a.buf_len, kInitLen);

    uint32_t m[32] = {}; // the message's first 128 bytes: type, sender, ephemeral 2..10, static 10..22, timestamp 22..29
    uint32_t chain[8] = {}, hash[8] = {};
    Noise ns{chain, hash};
    uint32_t point[8], spk[8] = {}, ts[3] = {};
    uint32_t peer = RG_PEER_NONE;
    if (st == kGoing) {
        load_words<32>(reinterpret_cast<const uint4 *>(a.buf + d.offset), m);
        if (m[0] != 1u) st = RG_PKT_INVALID; // Error::InvalidMessage
    }
    if (st == kGoing) {
        // -> e
        uint32_t e[12] = {}, sk[8];
        ns.init();
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            e[w] = point[w] = m[2 + w];
            ns.hash[w] = s_hash[w];
        }
        ns.mix_hash(e, 8);
        ns.mix_chain(e);
        load8(a.own, sk);
        // -> es, s (step 0: the ephemeral key, the encrypted static key) and -> ss, payload (step 1: the
        // decrypted static key, the encrypted timestamp)
#pragma unroll 1
        for (int step = 0; step < 2; ++step) {
            if (st != kGoing) continue; // a step that failed ends the message (no break: single-exit loop)
            uint32_t dh[8], key[8], f[12], pt[8];
            if (x25519_words(sk, point, dh) == 0) {
                st = RG_PKT_KEYEXCHANGE;
                continue;
            }
            ns.mix_key(dh, key);
#pragma unroll
            for (int w = 0; w < 12; ++w) f[w] = step ? (w < 7 ? m[22 + w] : 0u) : m[10 + w]; // ciphertext || tag
            if (!ns.decrypt_and_hash(key, f, step ? 12u : 32u, pt)) {
                st = RG_PKT_DECRYPT_ERR;
                continue;
            }
#pragma unroll
            for (int w = 0; w < 8; ++w) {
                if (step == 0) spk[w] = point[w] = pt[w];
                else if (w < 3) ts[w] = pt[w];
            }
        }
    }
    if (st == kGoing) {
        // Config::get_peer_idx: after both fields opened (handshake.rs:75-82)
        st = RG_PKT_REJECTED;
        uint32_t s = rx_slot(spk[0], a.cap);
        for (uint32_t probe = 0; probe < a.cap; ++probe) {
            const uint32_t row = a.table[s];
            if (row == RG_PEER_NONE) break;
            if (row < a.npeers) {
                uint32_t pk[8], diff = 0;
                load8(a.peers + 24ull * row, pk);
#pragma unroll
                for (int w = 0; w < 8; ++w) diff |= pk[w] ^ spk[w];
                if (diff == 0) {
                    peer = row;
                    st = RG_PKT_OK;
                    break;
                }
            }
            s = (s + 1) & (a.cap - 1);
        }
    }
    const bool ok = st == RG_PKT_OK;
    uint4 *row = a.results + 8ull * i;
    store_or_zero(row, ns.chain, 2, ok);
    store_or_zero(row + 2, ns.hash, 2, ok);
    store_or_zero(row + 4, m + 2, 2, ok); // the initiator's ephemeral key
    row[6] = ok ? make_uint4(ts[0], ts[1], ts[2], peer) : make_uint4(0, 0, 0, RG_PEER_NONE);
    row[7] = make_uint4(ok ? m[1] : 0u, 0, 0, 0);
    a.status[i] = (uint8_t)st; // after the row
}

// --------------------------------------------------------------- response
struct HsRespArgs {
    const uint32_t *peers;
    uint32_t npeers;
    uint4 *results;
    const uint8_t *gate;
    const uint32_t *esk;         // [n][8]
    const uint32_t *session_ids; // [n]
    const uint32_t *cookies;     // [n][4] or nullptr
    const uint8_t *has_cookie;   // [n], with cookies
    uint4 *responses;            // [n] rows of 6 uint4
    uint4 *tkeys;                // [n] rows of 4 uint4
    uint8_t *status;
    uint32_t n;
};

// <- e, ee, se, psk, {}, written; split(false)
__global__ __launch_bounds__(kHsWG) void handshake_resp_kernel(HsRespArgs a) {
    const uint32_t i = blockIdx.x * kHsWG + threadIdx.x;
    if (i >= a.n) return;
    if (a.gate && a.gate[i] != RG_PKT_OK) { // nothing of the row is read or written
        a.status[i] = RG_PKT_REJECTED;
        return;
    }
    uint4 *row = a.results + 8ull * i;
    uint32_t chain[8], hash[8];
    Noise ns{chain, hash};
    uint32_t eph[8], epk_r[8] = {}, w[24] = {}, send[8] = {};
    load_words<8>(row, ns.chain);
    load_words<8>(row + 2, ns.hash);
    load_words<8>(row + 4, eph);
    const uint32_t peer = row[6].w, sender = row[7].x;
    uint32_t st = peer < a.npeers ? kGoing : (uint32_t)RG_PKT_INVALID;
    if (st == kGoing) {
        const uint32_t *pr = a.peers + 24ull * peer; // public key, preshared key, mac1 key
        uint32_t esk[8], spk[8];
        load8(a.esk + 8ull * i, esk);
        load8(pr, spk);
        // <- e (step 0: the base point; our ephemeral public key goes into the chain and the hash), ee (step 1),
        // se (step 2): every step ends in mix_chain of the ladder's output
#pragma unroll 1
        for (int step = 0; step < 3; ++step) {
            uint32_t point[8], out[12] = {};
#pragma unroll
            for (int q = 0; q < 8; ++q) point[q] = step == 0 ? (q == 0 ? 9u : 0u) : step == 1 ? eph[q] : spk[q];
            if (st != kGoing) continue; // a step that failed ends the row (no break: single-exit loop)
            if (x25519_words(esk, point, out) == 0) { // never for the base point
                st = RG_PKT_KEYEXCHANGE;
                continue;
            }
            ns.mix_chain(out);
            if (step == 0) {
                ns.mix_hash(out, 8);
#pragma unroll
                for (int q = 0; q < 8; ++q) epk_r[q] = out[q];
            }
        }
        if (st == kGoing) {
            // <- psk, then the empty payload
            uint32_t psk[8], key[8], tag[4];
            load8(pr + 8, psk);
            ns.mix_key_and_hash(psk, key);
            ns.empty_tag(key, tag);
            // HandshakeResp: type, sender = our session id, receiver = the initiation's sender, ephemeral 3..11,
            // empty 11..15, mac1 15..19, mac2 19..23
            w[0] = 2u;
            w[1] = a.session_ids[i];
            w[2] = sender;
#pragma unroll
            for (int q = 0; q < 8; ++q) w[3 + q] = epk_r[q];
#pragma unroll
            for (int q = 0; q < 4; ++q) w[11 + q] = tag[q];
            hs_macs<23>(w, pr + 16, a.cookies && a.has_cookie[i] != 0 ? a.cookies + 4ull * i : nullptr);
            ns.split(send); // split(false): send under HKDF's second output, receive under the new chain
            st = RG_PKT_OK;
        }
    }
    const bool ok = st == RG_PKT_OK;
    uint4 *tk = a.tkeys + 4ull * i;
    store_or_zero(a.responses + 6ull * i, w, 6, ok);
    store_or_zero(tk, send, 2, ok);
    store_or_zero(tk + 2, ns.chain, 2, ok);
    // HandshakeState::zeroize: the row's chaining key and hash are consumed, whatever the verdict
#pragma unroll
    for (int q = 0; q < 4; ++q) row[q] = make_uint4(0, 0, 0, 0);
    a.status[i] = (uint8_t)st;
}

// --------------------------------------------------------------- initiate
struct HsInitiateArgs {
    const uint32_t *own;   // rg_hs_static
    const uint32_t *peers; // [npeers] rg_hs_peer rows of 24 words
    uint32_t npeers;
    const uint32_t *peer_idx; // [n]
    const uint8_t *gate;      // [n] or nullptr
    const uint32_t *esk;      // [n][8]
    const uint32_t *ts;       // [n][3]
    const uint32_t *session_ids;
    const uint32_t *cookies;   // [n][4] or nullptr
    const uint8_t *has_cookie; // [n], with cookies
    uint4 *messages;           // [n] rows of 10 uint4
    uint4 *pending;            // [n] rg_hs_pending rows of 8 uint4
    uint8_t *status;
    uint32_t n;
};

// -> e, es, s, ss, {timestamp}, written
__global__ __launch_bounds__(kHsWG) void handshake_initiate_kernel(HsInitiateArgs a) {
    const uint32_t i = blockIdx.x * kHsWG + threadIdx.x;
    if (i >= a.n) return;
    if (a.gate && a.gate[i] != RG_PKT_OK) { // nothing of the row is read or written
        a.status[i] = RG_PKT_REJECTED;
        return;
    }
    const uint32_t peer = a.peer_idx[i];
    uint32_t st = peer < a.npeers ? kGoing : (uint32_t)RG_PKT_INVALID;
    // the message: type, sender, ephemeral 2..10, static 10..22, timestamp 22..29, mac1 29..33, mac2 33..37
    uint32_t chain[8] = {}, hash[8] = {};
    Noise ns{chain, hash};
    uint32_t esk[8] = {}, w[40] = {};
    if (st == kGoing) {
        const uint32_t *pr = a.peers + 24ull * peer; // public key, preshared key, mac1 key
        uint32_t sk[8], pk[8], spk[12] = {}, ts[3];
        load8(a.esk + 8ull * i, esk);
        load8(a.own, sk);
        load8(a.own + 8, pk);
        load8(pr, spk);
#pragma unroll
        for (int q = 0; q < 3; ++q) ts[q] = a.ts[3ull * i + q];
        ns.init();
        ns.mix_hash(spk, 8); // the responder's static public key
        w[0] = 1u;
        w[1] = a.session_ids[i];
        // -> e (step 0: the base point; no key yet, so our ephemeral public key goes in the clear), es and s
        // (step 1: the sealed static key), ss and the payload (step 2: the sealed timestamp): every step mixes
        // its ladder's output into the chain and ends in mix_hash of what it put into the message
#pragma unroll 1
        for (int step = 0; step < 3; ++step) {
            uint32_t scalar[8], point[8], dh[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                scalar[q] = step == 2 ? sk[q] : esk[q];
                point[q] = step == 0 ? (q == 0 ? 9u : 0u) : spk[q];
            }
            if (st != kGoing) continue; // a step that failed ends the row (no break: single-exit loop)
            if (x25519_words(scalar, point, dh) == 0) { // never for the base point
                st = RG_PKT_KEYEXCHANGE;
                continue;
            }
            uint32_t key[8], field[8], out[12];
            ns.mix_key(dh, key, step != 0);
#pragma unroll
            for (int q = 0; q < 8; ++q) field[q] = step == 0 ? dh[q] : step == 1 ? pk[q] : (q < 3 ? ts[q] : 0u);
            ns.encrypt_and_hash(key, step != 0, field, step == 2 ? 12u : 32u, out);
#pragma unroll
            for (int q = 0; q < 12; ++q) { // 8 words of the ephemeral key, 12 of the static field, 7 of the timestamp
                if (step == 0 && q < 8) w[2 + q] = out[q];
                if (step == 1) w[10 + q] = out[q];
                if (step == 2 && q < 7) w[22 + q] = out[q];
            }
        }
        if (st == kGoing) {
            hs_macs<37>(w, pr + 16, a.cookies && a.has_cookie[i] != 0 ? a.cookies + 4ull * i : nullptr);
            st = RG_PKT_OK;
        }
    }
    const bool ok = st == RG_PKT_OK;
    uint4 *pend = a.pending + 8ull * i;
    store_or_zero(a.messages + 10ull * i, w, 10, ok);
    store_or_zero(pend, ns.chain, 2, ok);
    store_or_zero(pend + 2, ns.hash, 2, ok);
    store_or_zero(pend + 4, esk, 2, ok);
    pend[6] = ok ? make_uint4(peer, w[1], 0, 0) : make_uint4(RG_PEER_NONE, 0, 0, 0);
    pend[7] = make_uint4(0, 0, 0, 0);
    a.status[i] = (uint8_t)st; // after the rows
}

// ----------------------------------------------------------------- finish
struct HsFinishArgs {
    const uint32_t *own;   // rg_hs_static
    const uint32_t *peers; // [npeers] rg_hs_peer rows of 24 words
    uint32_t npeers;
    const rg_rx_entry *table; // [cap]: receiver id -> pending row
    uint32_t cap;
    uint4 *pending; // [npending] rg_hs_pending rows of 8 uint4: read by the finish, wiped by the commit
    uint32_t npending;
    const rg_pkt_desc *desc;
    const uint8_t *gate; // [n] or nullptr
    const uint8_t *buf;
    uint64_t buf_len;
    uint4 *tkeys;       // [n] rows of 4 uint4
    uint32_t *pend_idx; // [n]
    uint32_t *remote;   // [n]
    uint32_t *claim;    // [npending], 0xFFFFFFFF before the finish
    uint8_t *status;
    uint32_t n;
};

// <- e, ee, se, psk, {}, read; split(true)
__global__ __launch_bounds__(kHsWG) void handshake_finish_kernel(HsFinishArgs a) {
    const uint32_t i = blockIdx.x * kHsWG + threadIdx.x;
    if (i >= a.n) return;
    const rg_pkt_desc d = a.desc[i];
    uint32_t st = frame_verdict(d, a.gate ? a.gate[i] : (uint32_t)RG_PKT_OK, a.buf_len, kRespLen);

    uint32_t m[16] = {}; // the message's first 64 bytes: type, sender, receiver, ephemeral 3..11, empty 11..15
    uint32_t chain[8] = {}, hash[8] = {};
    Noise ns{chain, hash};
    uint32_t esk[8] = {}, recv[8] = {};
    uint32_t row = RG_PEER_NONE, peer = RG_PEER_NONE;
    if (st == kGoing) {
        load_words<16>(reinterpret_cast<const uint4 *>(a.buf + d.offset), m);
        if (m[0] != 2u) st = RG_PKT_INVALID; // Error::InvalidMessage
    }
    if (st == kGoing) {
        // handshake.rs:171-189: the receiver id names no session, or one that is already past its handshake
        row = rx_find(a.table, a.cap, m[2]);
        if (row == RG_KEY_SKIP) st = RG_PKT_REJECTED;
        else if (row >= a.npending) st = RG_PKT_INVALID;
    }
    if (st == kGoing) {
        peer = a.pending[8ull * row + 6].x;
        if (peer == RG_PEER_NONE) st = RG_PKT_REJECTED;
        else if (peer >= a.npeers) st = RG_PKT_INVALID;
    }
    if (st == kGoing) {
        const uint4 *pr = a.pending + 8ull * row;
        load_words<8>(pr, ns.chain);
        load_words<8>(pr + 2, ns.hash);
        load_words<8>(pr + 4, esk);
        uint32_t sk[8], e[12] = {};
        load8(a.own, sk);
#pragma unroll
        for (int q = 0; q < 8; ++q) e[q] = m[3 + q];
        ns.mix_hash(e, 8); // <- e; its mix_chain is step 0 below
        // every step ends in mix_chain: of the responder's ephemeral key (step 0, no ladder), of ee (step 1,
        // under our ephemeral key) and of se (step 2, under our static key)
#pragma unroll 1
        for (int step = 0; step < 3; ++step) {
            uint32_t scalar[8], mix[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                scalar[q] = step == 1 ? esk[q] : sk[q];
                mix[q] = e[q];
            }
            if (st != kGoing) continue; // a step that failed ends the message (no break: single-exit loop)
            if (step != 0 && x25519_words(scalar, e, mix) == 0) {
                st = RG_PKT_KEYEXCHANGE;
                continue;
            }
            ns.mix_chain(mix);
        }
        if (st == kGoing) {
            // <- psk, then the empty payload's tag
            uint32_t psk[8], key[8], tag[4];
            load8(a.peers + 24ull * peer + 8, psk);
            ns.mix_key_and_hash(psk, key);
            ns.empty_tag(key, tag);
            if (tag_diff(tag, m + 11) != 0) {
                st = RG_PKT_DECRYPT_ERR;
            } else {
                ns.split(recv);      // split(true): send under the new chain, receive under HKDF's second output
                st = RG_PKT_PENDING; // the commit kernel decides between the messages that got this far
            }
        }
    }
    const bool ok = st == RG_PKT_PENDING;
    uint4 *tk = a.tkeys + 4ull * i;
    store_or_zero(tk, ns.chain, 2, ok);
    store_or_zero(tk + 2, recv, 2, ok);
    a.pend_idx[i] = ok ? row : RG_PEER_NONE;
    a.remote[i] = ok ? m[1] : 0u;
    a.status[i] = (uint8_t)st; // after the row
    if (ok) atomicMin(&a.claim[row], i); // the minimum is the same whatever order the lanes arrive in
}

// "First finisher wins" (the reference's in-order loop) over the messages the finish kernel left pending: the
// lowest index that claimed a pending row finishes it and wipes it (hs.zeroize()), the others are rejected.
__global__ __launch_bounds__(kHsWG) void handshake_commit_kernel(HsFinishArgs a) {
    const uint32_t i = blockIdx.x * kHsWG + threadIdx.x;
    if (i >= a.n || a.status[i] != RG_PKT_PENDING) return;
    const uint32_t row = a.pend_idx[i];
    if (a.claim[row] == i) {
        uint4 *pr = a.pending + 8ull * row;
#pragma unroll
        for (int q = 0; q < 8; ++q) pr[q] = q == 6 ? make_uint4(RG_PEER_NONE, 0, 0, 0) : make_uint4(0, 0, 0, 0);
        a.status[i] = RG_PKT_OK; // written by the lane that decided it
    } else {
        uint4 *tk = a.tkeys + 4ull * i;
#pragma unroll
        for (int q = 0; q < 4; ++q) tk[q] = make_uint4(0, 0, 0, 0);
        a.pend_idx[i] = RG_PEER_NONE;
        a.remote[i] = 0u;
        a.status[i] = RG_PKT_REJECTED;
    }
}

} // namespace
} // namespace rg

using namespace rg::host;

namespace {
const dim3 kHsBlock(rg::kHsWG);

template <class T> const uint32_t *words(const T *p) { return reinterpret_cast<const uint32_t *>(p); }
template <class T> uint4 *quads(T *p) { return reinterpret_cast<uint4 *>(p); }
} // namespace

extern "C" int rg_x25519_batch_dev(rg_ctx *ctx, const uint8_t *scalars, const uint8_t *points, uint8_t *out,
                                   uint8_t *status, size_t n, void *stream) {
    rg::DeviceGuard dg_;
    const int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!scalars || !out || !status || n > 0xFFFFFFFFull) return bad("x25519", "bad args");
    if (misaligned(scalars, 4) || misaligned(points, 4) || misaligned(out, 4))
        return bad("x25519", "rows must be 4-byte aligned");
    rg::X25519Args a{};
    a.scalars = words(scalars);
    a.points = words(points);
    a.out = reinterpret_cast<uint32_t *>(out);
    a.status = status;
    a.n = (uint32_t)n;
    hipLaunchKernelGGL(rg::x25519_kernel, lanes(n, rg::kHsWG), kHsBlock, 0, (hipStream_t)stream, a);
    RG_HIP(hipGetLastError(), "x25519 launch");
    return RG_OK;
}

extern "C" int rg_handshake_init_batch_dev(rg_ctx *ctx, const rg_hs_static *own, const rg_hs_peer *peers,
                                           uint32_t npeers, const uint32_t *peer_table, uint32_t cap,
                                           const rg_pkt_desc *desc, const uint8_t *gate, size_t n, const uint8_t *buf,
                                           size_t buf_len, rg_hs_init_result *results, uint8_t *status, void *stream) {
    const char *const what = "handshake init";
    rg::DeviceGuard dg_;
    const int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!own || !peer_table || !desc || !buf || !results || !status || (npeers && !peers) || n > 0xFFFFFFFFull)
        return bad(what, "bad args");
    if (!pow2(cap)) return bad(what, "cap must be a power of two");
    if (misaligned(own, 16) || misaligned(peers, 16) || misaligned(desc, 16) || misaligned(results, 16) ||
        misaligned(peer_table, 4))
        return bad(what, "own, peers, desc and results must be 16-byte aligned, peer_table 4-byte aligned");
    rg::HsInitArgs a{};
    a.own = words(own);
    a.peers = words(peers);
    a.npeers = npeers;
    a.table = peer_table;
    a.cap = cap;
    a.desc = desc;
    a.gate = gate;
    a.buf = buf;
    a.buf_len = buf_len;
    a.results = quads(results);
    a.status = status;
    a.n = (uint32_t)n;
    hipLaunchKernelGGL(rg::handshake_init_kernel, lanes(n, rg::kHsWG), kHsBlock, 0, (hipStream_t)stream, a);
    RG_HIP(hipGetLastError(), "handshake init launch");
    return RG_OK;
}

extern "C" int rg_handshake_resp_batch_dev(rg_ctx *ctx, const rg_hs_peer *peers, uint32_t npeers,
                                           rg_hs_init_result *results, const uint8_t *gate, const uint8_t *esk,
                                           const uint32_t *session_ids, const uint8_t *cookies,
                                           const uint8_t *has_cookie, size_t n, uint8_t *responses,
                                           uint8_t *transport_keys, uint8_t *status, void *stream) {
    const char *const what = "handshake resp";
    rg::DeviceGuard dg_;
    const int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!results || !esk || !session_ids || !responses || !transport_keys || !status || (npeers && !peers) ||
        (cookies && !has_cookie) || n > 0xFFFFFFFFull)
        return bad(what, "bad args");
    if (misaligned(peers, 16) || misaligned(results, 16) || misaligned(responses, 16) || misaligned(transport_keys, 16) ||
        misaligned(esk, 4) || misaligned(session_ids, 4) || misaligned(cookies, 4))
        return bad(what, "peers, results, responses and transport_keys must be 16-byte aligned, esk, session_ids and "
                         "cookies 4-byte aligned");
    rg::HsRespArgs a{};
    a.peers = words(peers);
    a.npeers = npeers;
    a.results = quads(results);
    a.gate = gate;
    a.esk = words(esk);
    a.session_ids = session_ids;
    a.cookies = words(cookies);
    a.has_cookie = has_cookie;
    a.responses = quads(responses);
    a.tkeys = quads(transport_keys);
    a.status = status;
    a.n = (uint32_t)n;
    hipLaunchKernelGGL(rg::handshake_resp_kernel, lanes(n, rg::kHsWG), kHsBlock, 0, (hipStream_t)stream, a);
    RG_HIP(hipGetLastError(), "handshake resp launch");
    return RG_OK;
}

extern "C" int rg_handshake_initiate_batch_dev(rg_ctx *ctx, const rg_hs_static *own, const rg_hs_peer *peers,
                                               uint32_t npeers, const uint32_t *peer_idx, const uint8_t *gate,
                                               const uint8_t *esk, const uint8_t *timestamps,
                                               const uint32_t *session_ids, const uint8_t *cookies,
                                               const uint8_t *has_cookie, size_t n, uint8_t *messages,
                                               rg_hs_pending *pending, uint8_t *status, void *stream) {
    const char *const what = "handshake initiate";
    rg::DeviceGuard dg_;
    const int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!own || !peer_idx || !esk || !timestamps || !session_ids || !messages || !pending || !status ||
        (npeers && !peers) || (cookies && !has_cookie) || n > 0xFFFFFFFFull)
        return bad(what, "bad args");
    if (misaligned(own, 16) || misaligned(peers, 16) || misaligned(messages, 16) || misaligned(pending, 16) ||
        misaligned(peer_idx, 4) || misaligned(esk, 4) || misaligned(timestamps, 4) || misaligned(session_ids, 4) ||
        misaligned(cookies, 4))
        return bad(what, "own, peers, messages and pending must be 16-byte aligned, peer_idx, esk, timestamps, "
                         "session_ids and cookies 4-byte aligned");
    rg::HsInitiateArgs a{};
    a.own = words(own);
    a.peers = words(peers);
    a.npeers = npeers;
    a.peer_idx = peer_idx;
    a.gate = gate;
    a.esk = words(esk);
    a.ts = words(timestamps);
    a.session_ids = session_ids;
    a.cookies = words(cookies);
    a.has_cookie = has_cookie;
    a.messages = quads(messages);
    a.pending = quads(pending);
    a.status = status;
    a.n = (uint32_t)n;
    hipLaunchKernelGGL(rg::handshake_initiate_kernel, lanes(n, rg::kHsWG), kHsBlock, 0, (hipStream_t)stream, a);
    RG_HIP(hipGetLastError(), "handshake initiate launch");
    return RG_OK;
}

extern "C" int rg_handshake_finish_batch_dev(rg_ctx *ctx, const rg_hs_static *own, const rg_hs_peer *peers,
                                             uint32_t npeers, const rg_rx_entry *pend_table, uint32_t pend_cap,
                                             rg_hs_pending *pending, uint32_t npending, const rg_pkt_desc *desc,
                                             const uint8_t *gate, size_t n, const uint8_t *buf, size_t buf_len,
                                             uint8_t *transport_keys, uint32_t *pend_idx_out, uint32_t *remote_out,
                                             uint32_t *claim, uint8_t *status, void *stream) {
    const char *const what = "handshake finish";
    rg::DeviceGuard dg_;
    const int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!own || !pend_table || !pending || !desc || !buf || !transport_keys || !pend_idx_out || !remote_out ||
        !claim || !status || (npeers && !peers) || n > 0xFFFFFFFFull)
        return bad(what, "bad args");
    if (!pow2(pend_cap)) return bad(what, "pend_cap must be a power of two");
    if (misaligned(own, 16) || misaligned(peers, 16) || misaligned(pending, 16) || misaligned(desc, 16) ||
        misaligned(transport_keys, 16) || misaligned(pend_table, 4) || misaligned(pend_idx_out, 4) ||
        misaligned(remote_out, 4) || misaligned(claim, 4))
        return bad(what, "own, peers, pending, desc and transport_keys must be 16-byte aligned, pend_table, "
                         "pend_idx_out, remote_out and claim 4-byte aligned");
    rg::HsFinishArgs a{};
    a.own = words(own);
    a.peers = words(peers);
    a.npeers = npeers;
    a.table = pend_table;
    a.cap = pend_cap;
    a.pending = quads(pending);
    a.npending = npending;
    a.desc = desc;
    a.gate = gate;
    a.buf = buf;
    a.buf_len = buf_len;
    a.tkeys = quads(transport_keys);
    a.pend_idx = pend_idx_out;
    a.remote = remote_out;
    a.claim = claim;
    a.status = status;
    a.n = (uint32_t)n;
    hipStream_t s = (hipStream_t)stream;
    if (npending) RG_HIP(hipMemsetAsync(claim, 0xFF, (size_t)npending * sizeof(uint32_t), s), "handshake finish claim");
    hipLaunchKernelGGL(rg::handshake_finish_kernel, lanes(n, rg::kHsWG), kHsBlock, 0, s, a);
    RG_HIP(hipGetLastError(), "handshake finish launch");
    hipLaunchKernelGGL(rg::handshake_commit_kernel, lanes(n, rg::kHsWG), kHsBlock, 0, s, a);
    RG_HIP(hipGetLastError(), "handshake finish commit launch");
    return RG_OK;
}
