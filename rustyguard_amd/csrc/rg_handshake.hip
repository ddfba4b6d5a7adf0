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
// The cost is the X25519 ladder of rg_x25519.h: two per initiation consumed, three per response built, three
// per initiation built, two per response consumed, ~2800 field multiplications each; everything else (some
// fifty BLAKE2s compressions, a few ChaCha20 blocks) is noise beside it.  So the kernels are laid out for code size, not for the hash: the ladders of one kernel share
// one call site (a loop over the kernel's Diffie-Hellman steps, with the work that follows each step chosen
// by the loop count, which is public), and the HKDF steps share b2s_hkdf's.  Workgroups are one wave, so that
// a batch of a thousand messages still spreads over sixteen CUs.
//
// Constant time: no branch and no address depends on a private key, a shared secret, a chaining key or an
// AEAD key.  Branches follow the descriptor, the gate, the loop counts and the verdicts that the status array
// publishes anyway (a zero shared secret, a failed tag, an unknown static key); tag and key comparisons are
// OR-folds over all their words.  Nothing derived from a key is written to global memory except the rows
// the interface defines, and a row whose message fails is written as zeros.
//
// The entry points' host side is here too, on rg_host.h, like rg_cookie.hip's.
#include "rg_blake2s.h"
#include "rg_device.h"
#include "rg_host.h"
#include "rg_x25519.h"

namespace rg {
namespace {

constexpr int kHsWG = 64;           // one wave per workgroup
constexpr uint32_t kGoing = 0xFFu;  // no verdict yet (never stored)
constexpr uint32_t kInitLen = 148;  // HandshakeInit (rustyguard-types)

// HandshakeState::default(): BLAKE2s("Noise_IKpsk2_25519_ChaChaPoly_BLAKE2s") and
// BLAKE2s(that || "WireGuard v1 zx2c4 Jason@zx2c4.com"), as little-endian words
__device__ constexpr uint32_t kConstruction[8] = {0xAE6DE260u, 0xC0EF27F3u, 0xE235C32Eu, 0xD0D225A0u,
                                                  0x0642EB16u, 0xF57772F8u, 0x98D1382Du, 0x36CD788Bu};
__device__ constexpr uint32_t kIdentifier[8] = {0x61B31122u, 0x66C51A08u, 0xDB431269u, 0x32D58A45u,
                                                0x666C9C2Du, 0xB7E89322u, 0x659CE10Eu, 0xF39E07BAu};

__device__ __forceinline__ void load8(const uint32_t *p, uint32_t w[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = p[i];
}

// ChaCha20-Poly1305 with nonce 0 and aad = the 32-byte transcript hash over a payload of at most two
// 16-byte blocks (Encrypted<N>, prim.rs:330-366; N = 32, 12 or 0): the tag over ciphertext ct (zero past
// len bytes) and the keystream of block 1.  seal: ct holds the plaintext (zero past len bytes) and is
// encrypted in place first.
__device__ __forceinline__ void hs_aead(const uint32_t key[8], const uint32_t aad[8], uint32_t ct[8], uint32_t len,
                                        uint32_t stream[16], uint32_t tag[4], bool seal = false) {
    Key8 k;
#pragma unroll
    for (int i = 0; i < 8; ++i) k.k[i] = key[i];
    uint32_t otk[16];
    chacha_block(k, 0, 0, 0, 0, otk);
    chacha_block(k, 1, 0, 0, 0, stream);
    if (seal) {
#pragma unroll
        for (int i = 0; i < 8; ++i) ct[i] = (uint32_t)(4 * i) < len ? ct[i] ^ stream[i] : 0u;
    }
    const Mul r = make_mul(otk[0], otk[1], otk[2], otk[3]);
    Acc acc = {0, 0, 0, 0, 0};
    acc_block(acc, make_uint4(aad[0], aad[1], aad[2], aad[3]), r);
    acc_block(acc, make_uint4(aad[4], aad[5], aad[6], aad[7]), r);
    acc_block_pred(acc, make_uint4(ct[0], ct[1], ct[2], ct[3]), r, len > 0);
    acc_block_pred(acc, make_uint4(ct[4], ct[5], ct[6], ct[7]), r, len > 16);
    acc_block(acc, make_uint4(32u, 0u, len, 0u), r); // le64(aad_len) || le64(ct_len)
    acc_finish(acc, otk[4], otk[5], otk[6], otk[7], tag);
}

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

__global__ __launch_bounds__(kHsWG) void handshake_init_kernel(HsInitArgs a) {
    __shared__ uint32_t s_hash[8]; // the transcript hash after mix_hash(own public key): the same for every message
    if (threadIdx.x == 0) {
        uint32_t pk[12] = {}, h[8];
        load8(a.own + 8, pk);
        b2s_hash32(kIdentifier, pk, 8, h);
#pragma unroll
        for (int w = 0; w < 8; ++w) s_hash[w] = h[w];
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * kHsWG + threadIdx.x;
    if (i >= a.n) return;
    const rg_pkt_desc d = a.desc[i];
    uint32_t st = kGoing;
    if ((d.offset & 15u) != 0) st = RG_PKT_UNALIGNED;
    else if (d.offset > a.buf_len || d.len > a.buf_len - d.offset || d.len != kInitLen) st = RG_PKT_INVALID;
    else if ((a.gate && a.gate[i] != RG_PKT_OK) || d.key_idx == RG_KEY_SKIP) st = RG_PKT_REJECTED;

    uint32_t m[32] = {}; // the message's first 128 bytes: type, sender, ephemeral 2..10, static 10..22, timestamp 22..29
    uint32_t chain[8], hash[8], point[8], spk[8] = {}, ts[3] = {};
    uint32_t peer = RG_PEER_NONE;
    if (st == kGoing) {
        const uint4 *mp = reinterpret_cast<const uint4 *>(a.buf + d.offset);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const uint4 v = mp[q];
            m[4 * q] = v.x; m[4 * q + 1] = v.y; m[4 * q + 2] = v.z; m[4 * q + 3] = v.w;
        }
        if (m[0] != 1u) st = RG_PKT_INVALID; // Error::InvalidMessage
    }
    if (st == kGoing) {
        // -> e: mix_hash(ephemeral), mix_chain(ephemeral)
        uint32_t e[12] = {}, h0[8], none[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            e[w] = point[w] = m[2 + w];
            h0[w] = s_hash[w];
            chain[w] = kConstruction[w];
        }
        b2s_hash32(h0, e, 8, hash);
        b2s_hkdf(chain, e, 32, 0, none, none);
        uint32_t sk[8];
        load8(a.own, sk);
        // -> es, s (step 0: the ephemeral key, the encrypted static key) and -> ss, payload (step 1: the
        // decrypted static key, the encrypted timestamp)
#pragma unroll 1
        for (int step = 0; step < 2; ++step) {
            if (st != kGoing) continue; // a step that failed ends the message (no break: single-exit loop)
            uint32_t dh[8], key[8], none2[8];
            if (x25519_words(sk, point, dh) == 0) {
                st = RG_PKT_KEYEXCHANGE;
                continue;
            }
            b2s_hkdf(chain, dh, 32, 1, key, none2); // mix_key
            uint32_t f[12], ct[8], stream[16], tag[4];
#pragma unroll
            for (int w = 0; w < 12; ++w) f[w] = step ? (w < 7 ? m[22 + w] : 0u) : m[10 + w]; // ciphertext || tag
            const uint32_t len = step ? 12u : 32u;
#pragma unroll
            for (int w = 0; w < 8; ++w) ct[w] = (uint32_t)(4 * w) < len ? f[w] : 0u;
            hs_aead(key, hash, ct, len, stream, tag);
            uint32_t diff = 0; // the field's tag follows its 3 or 8 ciphertext words
#pragma unroll
            for (int w = 0; w < 4; ++w) diff |= tag[w] ^ (step ? f[3 + w] : f[8 + w]);
            if (diff != 0) {
                st = RG_PKT_DECRYPT_ERR;
                continue;
            }
            uint32_t nh[8];
            b2s_hash32(hash, f, step ? 7u : 12u, nh); // mix_hash(ciphertext || tag)
#pragma unroll
            for (int w = 0; w < 8; ++w) {
                hash[w] = nh[w];
                const uint32_t pt = ct[w] ^ stream[w];
                if (step == 0) spk[w] = point[w] = pt;
                else if (w < 3) ts[w] = pt;
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
    row[0] = ok ? make_uint4(chain[0], chain[1], chain[2], chain[3]) : make_uint4(0, 0, 0, 0);
    row[1] = ok ? make_uint4(chain[4], chain[5], chain[6], chain[7]) : make_uint4(0, 0, 0, 0);
    row[2] = ok ? make_uint4(hash[0], hash[1], hash[2], hash[3]) : make_uint4(0, 0, 0, 0);
    row[3] = ok ? make_uint4(hash[4], hash[5], hash[6], hash[7]) : make_uint4(0, 0, 0, 0);
    row[4] = ok ? make_uint4(m[2], m[3], m[4], m[5]) : make_uint4(0, 0, 0, 0);
    row[5] = ok ? make_uint4(m[6], m[7], m[8], m[9]) : make_uint4(0, 0, 0, 0);
    row[6] = ok ? make_uint4(ts[0], ts[1], ts[2], peer) : make_uint4(0, 0, 0, RG_PEER_NONE);
    row[7] = ok ? make_uint4(m[1], 0, 0, 0) : make_uint4(0, 0, 0, 0);
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

__global__ __launch_bounds__(kHsWG) void handshake_resp_kernel(HsRespArgs a) {
    const uint32_t i = blockIdx.x * kHsWG + threadIdx.x;
    if (i >= a.n) return;
    if (a.gate && a.gate[i] != RG_PKT_OK) { // nothing of the row is read or written
        a.status[i] = RG_PKT_REJECTED;
        return;
    }
    uint4 *row = a.results + 8ull * i;
    uint32_t chain[8], hash[8], eph[8], epk_r[8] = {}, w[24] = {}, send[8] = {};
    {
        const uint4 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3], r4 = row[4], r5 = row[5];
        chain[0] = r0.x; chain[1] = r0.y; chain[2] = r0.z; chain[3] = r0.w;
        chain[4] = r1.x; chain[5] = r1.y; chain[6] = r1.z; chain[7] = r1.w;
        hash[0] = r2.x; hash[1] = r2.y; hash[2] = r2.z; hash[3] = r2.w;
        hash[4] = r3.x; hash[5] = r3.y; hash[6] = r3.z; hash[7] = r3.w;
        eph[0] = r4.x; eph[1] = r4.y; eph[2] = r4.z; eph[3] = r4.w;
        eph[4] = r5.x; eph[5] = r5.y; eph[6] = r5.z; eph[7] = r5.w;
    }
    const uint32_t peer = row[6].w, sender = row[7].x;
    uint32_t st = peer < a.npeers ? kGoing : (uint32_t)RG_PKT_INVALID;
    if (st == kGoing) {
        const uint32_t *pr = a.peers + 24ull * peer; // public key, preshared key, mac1 key
        uint32_t esk[8], spk[8], none[8];
        load8(a.esk + 8ull * i, esk);
        load8(pr, spk);
        // <- e (step 0: the base point; mix_chain and mix_hash of our ephemeral public key), ee (step 1),
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
            b2s_hkdf(chain, out, 32, 0, none, none);
            if (step == 0) {
                uint32_t nh[8];
                b2s_hash32(hash, out, 8, nh);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    hash[q] = nh[q];
                    epk_r[q] = out[q];
                }
            }
        }
        if (st == kGoing) {
            // <- psk: mix_key_and_hash; payload: the empty AEAD under aad = hash
            uint32_t psk[8], t[12] = {}, key[8], nh[8], zero[8] = {}, stream[16], tag[4];
            load8(pr + 8, psk);
            b2s_hkdf(chain, psk, 32, 2, t, key);
            b2s_hash32(hash, t, 8, nh);
            hs_aead(key, nh, zero, 0, stream, tag);
            // HandshakeResp: type, sender = our session id, receiver = the initiation's sender, ephemeral, empty
            w[0] = 2u;
            w[1] = a.session_ids[i];
            w[2] = sender;
#pragma unroll
            for (int q = 0; q < 8; ++q) w[3 + q] = epk_r[q];
#pragma unroll
            for (int q = 0; q < 4; ++q) w[11 + q] = tag[q];
            // mac1 = BLAKE2s-128(mac1_key, bytes 0..60)
            uint32_t ks[8], mk[8], blk[16];
            load8(pr + 16, mk);
            b2s_key_state(mk, 32, false, ks);
#pragma unroll
            for (int q = 0; q < 16; ++q) blk[q] = q < 15 ? w[q] : 0u;
            b2s_compress(ks, blk, 64 + 60, true);
#pragma unroll
            for (int q = 0; q < 4; ++q) w[15 + q] = ks[q];
            // mac2 = BLAKE2s-128(cookie, bytes 0..76) when the peer gave us a cookie, else zero
            if (a.cookies && a.has_cookie[i] != 0) {
                uint32_t ck[8] = {};
#pragma unroll
                for (int q = 0; q < 4; ++q) ck[q] = a.cookies[4ull * i + q];
                b2s_key_state(ck, 16, false, ks);
#pragma unroll
                for (int q = 0; q < 16; ++q) blk[q] = w[q];
                b2s_compress(ks, blk, 128, false);
#pragma unroll
                for (int q = 0; q < 16; ++q) blk[q] = q < 3 ? w[16 + q] : 0u;
                b2s_compress(ks, blk, 64 + 76, true);
#pragma unroll
                for (int q = 0; q < 4; ++q) w[19 + q] = ks[q];
            }
            // split(false): send under HKDF's second output, receive under the new chain
            b2s_hkdf(chain, zero, 0, 1, send, none);
            st = RG_PKT_OK;
        }
    }
    const bool ok = st == RG_PKT_OK;
    uint4 *resp = a.responses + 6ull * i, *tk = a.tkeys + 4ull * i;
#pragma unroll
    for (int q = 0; q < 6; ++q)
        resp[q] = ok ? make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]) : make_uint4(0, 0, 0, 0);
    tk[0] = ok ? make_uint4(send[0], send[1], send[2], send[3]) : make_uint4(0, 0, 0, 0);
    tk[1] = ok ? make_uint4(send[4], send[5], send[6], send[7]) : make_uint4(0, 0, 0, 0);
    tk[2] = ok ? make_uint4(chain[0], chain[1], chain[2], chain[3]) : make_uint4(0, 0, 0, 0);
    tk[3] = ok ? make_uint4(chain[4], chain[5], chain[6], chain[7]) : make_uint4(0, 0, 0, 0);
    // HandshakeState::zeroize: the row's chaining key and hash are consumed, whatever the verdict
#pragma unroll
    for (int q = 0; q < 4; ++q) row[q] = make_uint4(0, 0, 0, 0);
    a.status[i] = (uint8_t)st;
}

// --------------------------------------------------------------- initiate
// BLAKE2s-128(key, the first NW words of w): mac1 under a 32-byte key, mac2 under a 16-byte cookie
// (HasMac, lib.rs:114-209), as handshake_resp_kernel computes them
template <int NW>
__device__ __forceinline__ void hs_mac(const uint32_t key[8], uint32_t key_len, const uint32_t *w, uint32_t out[4]) {
    uint32_t ks[8], blk[16];
    b2s_key_state(key, key_len, false, ks);
#pragma unroll
    for (int b = 0; 16 * b < NW; ++b) {
        const bool last = 16 * (b + 1) >= NW;
#pragma unroll
        for (int q = 0; q < 16; ++q) blk[q] = 16 * b + q < NW ? w[16 * b + q] : 0u;
        b2s_compress(ks, blk, 64 + (last ? 4 * NW : 64 * (b + 1)), last);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) out[q] = ks[q];
}

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
    uint32_t chain[8] = {}, hash[8] = {}, esk[8] = {}, w[40] = {};
    if (st == kGoing) {
        const uint32_t *pr = a.peers + 24ull * peer; // public key, preshared key, mac1 key
        uint32_t sk[8], pk[8], spk[12] = {}, ts[3];
        load8(a.esk + 8ull * i, esk);
        load8(a.own, sk);
        load8(a.own + 8, pk);
        load8(pr, spk);
#pragma unroll
        for (int q = 0; q < 3; ++q) ts[q] = a.ts[3ull * i + q];
        // HandshakeState::default() and mix_hash(the responder's static public key)
#pragma unroll
        for (int q = 0; q < 8; ++q) chain[q] = kConstruction[q];
        b2s_hash32(kIdentifier, spk, 8, hash);
        w[0] = 1u;
        w[1] = a.session_ids[i];
        // -> e (step 0: the base point; mix_hash and mix_chain of our ephemeral public key), es and s (step 1:
        // mix_key, the sealed static key), ss and the payload (step 2: mix_key, the sealed timestamp); every
        // step ends in mix_hash of what it put into the message
#pragma unroll 1
        for (int step = 0; step < 3; ++step) {
            uint32_t scalar[8], point[8], out[12] = {};
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                scalar[q] = step == 2 ? sk[q] : esk[q];
                point[q] = step == 0 ? (q == 0 ? 9u : 0u) : spk[q];
            }
            if (st != kGoing) continue; // a step that failed ends the row (no break: single-exit loop)
            if (x25519_words(scalar, point, out) == 0) { // never for the base point
                st = RG_PKT_KEYEXCHANGE;
                continue;
            }
            uint32_t key[8], none[8], nh[8];
            b2s_hkdf(chain, out, 32, step ? 1 : 0, key, none);
            if (step == 0) {
#pragma unroll
                for (int q = 0; q < 8; ++q) w[2 + q] = out[q];
            } else {
                uint32_t ct[8], stream[16], tag[4];
#pragma unroll
                for (int q = 0; q < 8; ++q) ct[q] = step == 1 ? pk[q] : (q < 3 ? ts[q] : 0u);
                hs_aead(key, hash, ct, step == 1 ? 32u : 12u, stream, tag, true);
#pragma unroll
                for (int q = 0; q < 12; ++q) // ciphertext || tag: 12 words of the static field, 7 of the timestamp
                    out[q] = step == 1 ? (q < 8 ? ct[q] : tag[q - 8]) : (q < 3 ? ct[q] : q < 7 ? tag[q - 3] : 0u);
                if (step == 1) {
#pragma unroll
                    for (int q = 0; q < 12; ++q) w[10 + q] = out[q];
                } else {
#pragma unroll
                    for (int q = 0; q < 7; ++q) w[22 + q] = out[q];
                }
            }
            b2s_hash32(hash, out, step == 0 ? 8u : step == 1 ? 12u : 7u, nh);
#pragma unroll
            for (int q = 0; q < 8; ++q) hash[q] = nh[q];
        }
        if (st == kGoing) {
            // mac1 = BLAKE2s-128(mac1_key, bytes 0..116); mac2 = BLAKE2s-128(cookie, bytes 0..132) when the peer
            // gave us a cookie, else zero
            uint32_t mk[8], m[4];
            load8(pr + 16, mk);
            hs_mac<29>(mk, 32, w, m);
#pragma unroll
            for (int q = 0; q < 4; ++q) w[29 + q] = m[q];
            if (a.cookies && a.has_cookie[i] != 0) {
                uint32_t ck[8] = {};
#pragma unroll
                for (int q = 0; q < 4; ++q) ck[q] = a.cookies[4ull * i + q];
                hs_mac<33>(ck, 16, w, m);
#pragma unroll
                for (int q = 0; q < 4; ++q) w[33 + q] = m[q];
            }
            st = RG_PKT_OK;
        }
    }
    const bool ok = st == RG_PKT_OK;
    uint4 *msg = a.messages + 10ull * i, *pend = a.pending + 8ull * i;
#pragma unroll
    for (int q = 0; q < 10; ++q)
        msg[q] = ok ? make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]) : make_uint4(0, 0, 0, 0);
    pend[0] = ok ? make_uint4(chain[0], chain[1], chain[2], chain[3]) : make_uint4(0, 0, 0, 0);
    pend[1] = ok ? make_uint4(chain[4], chain[5], chain[6], chain[7]) : make_uint4(0, 0, 0, 0);
    pend[2] = ok ? make_uint4(hash[0], hash[1], hash[2], hash[3]) : make_uint4(0, 0, 0, 0);
    pend[3] = ok ? make_uint4(hash[4], hash[5], hash[6], hash[7]) : make_uint4(0, 0, 0, 0);
    pend[4] = ok ? make_uint4(esk[0], esk[1], esk[2], esk[3]) : make_uint4(0, 0, 0, 0);
    pend[5] = ok ? make_uint4(esk[4], esk[5], esk[6], esk[7]) : make_uint4(0, 0, 0, 0);
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

constexpr uint32_t kRespLen = 92; // HandshakeResp (rustyguard-types)

__global__ __launch_bounds__(kHsWG) void handshake_finish_kernel(HsFinishArgs a) {
    const uint32_t i = blockIdx.x * kHsWG + threadIdx.x;
    if (i >= a.n) return;
    const rg_pkt_desc d = a.desc[i];
    uint32_t st = kGoing;
    if ((d.offset & 15u) != 0) st = RG_PKT_UNALIGNED;
    else if (d.offset > a.buf_len || d.len > a.buf_len - d.offset || d.len != kRespLen) st = RG_PKT_INVALID;
    else if ((a.gate && a.gate[i] != RG_PKT_OK) || d.key_idx == RG_KEY_SKIP) st = RG_PKT_REJECTED;

    uint32_t m[16] = {}; // the message's first 64 bytes: type, sender, receiver, ephemeral 3..11, empty 11..15
    uint32_t chain[8] = {}, hash[8] = {}, esk[8] = {}, recv[8] = {};
    uint32_t row = RG_PEER_NONE, peer = RG_PEER_NONE;
    if (st == kGoing) {
        const uint4 *mp = reinterpret_cast<const uint4 *>(a.buf + d.offset);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 v = mp[q];
            m[4 * q] = v.x; m[4 * q + 1] = v.y; m[4 * q + 2] = v.z; m[4 * q + 3] = v.w;
        }
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
        const uint4 r0 = pr[0], r1 = pr[1], r2 = pr[2], r3 = pr[3], r4 = pr[4], r5 = pr[5];
        chain[0] = r0.x; chain[1] = r0.y; chain[2] = r0.z; chain[3] = r0.w;
        chain[4] = r1.x; chain[5] = r1.y; chain[6] = r1.z; chain[7] = r1.w;
        hash[0] = r2.x; hash[1] = r2.y; hash[2] = r2.z; hash[3] = r2.w;
        hash[4] = r3.x; hash[5] = r3.y; hash[6] = r3.z; hash[7] = r3.w;
        esk[0] = r4.x; esk[1] = r4.y; esk[2] = r4.z; esk[3] = r4.w;
        esk[4] = r5.x; esk[5] = r5.y; esk[6] = r5.z; esk[7] = r5.w;
        uint32_t sk[8], e[12] = {}, none[8], nh[8];
        load8(a.own, sk);
#pragma unroll
        for (int q = 0; q < 8; ++q) e[q] = m[3 + q];
        b2s_hash32(hash, e, 8, nh); // <- e: mix_hash; its mix_chain is step 0 below
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
            b2s_hkdf(chain, mix, 32, 0, none, none);
        }
        if (st == kGoing) {
            // <- psk: mix_key_and_hash; the empty field's tag under aad = hash
            uint32_t psk[8], t[12] = {}, key[8], zero[8] = {}, stream[16], tag[4], diff = 0;
            load8(a.peers + 24ull * peer + 8, psk);
            b2s_hkdf(chain, psk, 32, 2, t, key);
            b2s_hash32(nh, t, 8, hash);
            hs_aead(key, hash, zero, 0, stream, tag);
#pragma unroll
            for (int q = 0; q < 4; ++q) diff |= tag[q] ^ m[11 + q];
            if (diff != 0) {
                st = RG_PKT_DECRYPT_ERR;
            } else {
                // split(true): send under the new chain, receive under HKDF's second output
                b2s_hkdf(chain, zero, 0, 1, recv, none);
                st = RG_PKT_PENDING; // the commit kernel decides between the messages that got this far
            }
        }
    }
    const bool ok = st == RG_PKT_PENDING;
    uint4 *tk = a.tkeys + 4ull * i;
    tk[0] = ok ? make_uint4(chain[0], chain[1], chain[2], chain[3]) : make_uint4(0, 0, 0, 0);
    tk[1] = ok ? make_uint4(chain[4], chain[5], chain[6], chain[7]) : make_uint4(0, 0, 0, 0);
    tk[2] = ok ? make_uint4(recv[0], recv[1], recv[2], recv[3]) : make_uint4(0, 0, 0, 0);
    tk[3] = ok ? make_uint4(recv[4], recv[5], recv[6], recv[7]) : make_uint4(0, 0, 0, 0);
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
uint32_t grid(size_t n) { return (uint32_t)((n + rg::kHsWG - 1) / rg::kHsWG); }
} // namespace

extern "C" int rg_x25519_batch_dev(rg_ctx *ctx, const uint8_t *scalars, const uint8_t *points, uint8_t *out,
                                   uint8_t *status, size_t n, void *stream) {
    rg::DeviceGuard dg_;
    const int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!scalars || !out || !status || n > 0xFFFFFFFFull) return set_err(RG_EINVAL, "x25519: bad args");
    if (misaligned(scalars, 4) || misaligned(points, 4) || misaligned(out, 4))
        return set_err(RG_EINVAL, "x25519: rows must be 4-byte aligned");
    rg::X25519Args a{};
    a.scalars = reinterpret_cast<const uint32_t *>(scalars);
    a.points = reinterpret_cast<const uint32_t *>(points);
    a.out = reinterpret_cast<uint32_t *>(out);
    a.status = status;
    a.n = (uint32_t)n;
    hipLaunchKernelGGL(rg::x25519_kernel, dim3(grid(n)), dim3(rg::kHsWG), 0, (hipStream_t)stream, a);
    RG_HIP(hipGetLastError(), "x25519 launch");
    return RG_OK;
}

extern "C" int rg_handshake_init_batch_dev(rg_ctx *ctx, const rg_hs_static *own, const rg_hs_peer *peers,
                                           uint32_t npeers, const uint32_t *peer_table, uint32_t cap,
                                           const rg_pkt_desc *desc, const uint8_t *gate, size_t n, const uint8_t *buf,
                                           size_t buf_len, rg_hs_init_result *results, uint8_t *status, void *stream) {
    rg::DeviceGuard dg_;
    const int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!own || !peer_table || !desc || !buf || !results || !status || (npeers && !peers) || n > 0xFFFFFFFFull)
        return set_err(RG_EINVAL, "handshake init: bad args");
    if (cap == 0 || (cap & (cap - 1)) != 0) return set_err(RG_EINVAL, "handshake init: cap must be a power of two");
    if (misaligned(own, 16) || misaligned(peers, 16) || misaligned(desc, 16) || misaligned(results, 16) ||
        misaligned(peer_table, 4))
        return set_err(RG_EINVAL, "handshake init: own, peers, desc and results must be 16-byte aligned, "
                                  "peer_table 4-byte aligned");
    rg::HsInitArgs a{};
    a.own = reinterpret_cast<const uint32_t *>(own);
    a.peers = reinterpret_cast<const uint32_t *>(peers);
    a.npeers = npeers;
    a.table = peer_table;
    a.cap = cap;
    a.desc = desc;
    a.gate = gate;
    a.buf = buf;
    a.buf_len = buf_len;
    a.results = reinterpret_cast<uint4 *>(results);
    a.status = status;
    a.n = (uint32_t)n;
    hipLaunchKernelGGL(rg::handshake_init_kernel, dim3(grid(n)), dim3(rg::kHsWG), 0, (hipStream_t)stream, a);
    RG_HIP(hipGetLastError(), "handshake init launch");
    return RG_OK;
}

extern "C" int rg_handshake_resp_batch_dev(rg_ctx *ctx, const rg_hs_peer *peers, uint32_t npeers,
                                           rg_hs_init_result *results, const uint8_t *gate, const uint8_t *esk,
                                           const uint32_t *session_ids, const uint8_t *cookies,
                                           const uint8_t *has_cookie, size_t n, uint8_t *responses,
                                           uint8_t *transport_keys, uint8_t *status, void *stream) {
    rg::DeviceGuard dg_;
    const int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!results || !esk || !session_ids || !responses || !transport_keys || !status || (npeers && !peers) ||
        (cookies && !has_cookie) || n > 0xFFFFFFFFull)
        return set_err(RG_EINVAL, "handshake resp: bad args");
    if (misaligned(peers, 16) || misaligned(results, 16) || misaligned(responses, 16) || misaligned(transport_keys, 16) ||
        misaligned(esk, 4) || misaligned(session_ids, 4) || misaligned(cookies, 4))
        return set_err(RG_EINVAL, "handshake resp: peers, results, responses and transport_keys must be 16-byte "
                                  "aligned, esk, session_ids and cookies 4-byte aligned");
    rg::HsRespArgs a{};
    a.peers = reinterpret_cast<const uint32_t *>(peers);
    a.npeers = npeers;
    a.results = reinterpret_cast<uint4 *>(results);
    a.gate = gate;
    a.esk = reinterpret_cast<const uint32_t *>(esk);
    a.session_ids = session_ids;
    a.cookies = reinterpret_cast<const uint32_t *>(cookies);
    a.has_cookie = has_cookie;
    a.responses = reinterpret_cast<uint4 *>(responses);
    a.tkeys = reinterpret_cast<uint4 *>(transport_keys);
    a.status = status;
    a.n = (uint32_t)n;
    hipLaunchKernelGGL(rg::handshake_resp_kernel, dim3(grid(n)), dim3(rg::kHsWG), 0, (hipStream_t)stream, a);
    RG_HIP(hipGetLastError(), "handshake resp launch");
    return RG_OK;
}

extern "C" int rg_handshake_initiate_batch_dev(rg_ctx *ctx, const rg_hs_static *own, const rg_hs_peer *peers,
                                               uint32_t npeers, const uint32_t *peer_idx, const uint8_t *gate,
                                               const uint8_t *esk, const uint8_t *timestamps,
                                               const uint32_t *session_ids, const uint8_t *cookies,
                                               const uint8_t *has_cookie, size_t n, uint8_t *messages,
                                               rg_hs_pending *pending, uint8_t *status, void *stream) {
    rg::DeviceGuard dg_;
    const int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!own || !peer_idx || !esk || !timestamps || !session_ids || !messages || !pending || !status ||
        (npeers && !peers) || (cookies && !has_cookie) || n > 0xFFFFFFFFull)
        return set_err(RG_EINVAL, "handshake initiate: bad args");
    if (misaligned(own, 16) || misaligned(peers, 16) || misaligned(messages, 16) || misaligned(pending, 16) ||
        misaligned(peer_idx, 4) || misaligned(esk, 4) || misaligned(timestamps, 4) || misaligned(session_ids, 4) ||
        misaligned(cookies, 4))
        return set_err(RG_EINVAL, "handshake initiate: own, peers, messages and pending must be 16-byte aligned, "
                                  "peer_idx, esk, timestamps, session_ids and cookies 4-byte aligned");
    rg::HsInitiateArgs a{};
    a.own = reinterpret_cast<const uint32_t *>(own);
    a.peers = reinterpret_cast<const uint32_t *>(peers);
    a.npeers = npeers;
    a.peer_idx = peer_idx;
    a.gate = gate;
    a.esk = reinterpret_cast<const uint32_t *>(esk);
    a.ts = reinterpret_cast<const uint32_t *>(timestamps);
    a.session_ids = session_ids;
    a.cookies = reinterpret_cast<const uint32_t *>(cookies);
    a.has_cookie = has_cookie;
    a.messages = reinterpret_cast<uint4 *>(messages);
    a.pending = reinterpret_cast<uint4 *>(pending);
    a.status = status;
    a.n = (uint32_t)n;
    hipLaunchKernelGGL(rg::handshake_initiate_kernel, dim3(grid(n)), dim3(rg::kHsWG), 0, (hipStream_t)stream, a);
    RG_HIP(hipGetLastError(), "handshake initiate launch");
    return RG_OK;
}

extern "C" int rg_handshake_finish_batch_dev(rg_ctx *ctx, const rg_hs_static *own, const rg_hs_peer *peers,
                                             uint32_t npeers, const rg_rx_entry *pend_table, uint32_t pend_cap,
                                             rg_hs_pending *pending, uint32_t npending, const rg_pkt_desc *desc,
                                             const uint8_t *gate, size_t n, const uint8_t *buf, size_t buf_len,
                                             uint8_t *transport_keys, uint32_t *pend_idx_out, uint32_t *remote_out,
                                             uint32_t *claim, uint8_t *status, void *stream) {
    rg::DeviceGuard dg_;
    const int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!own || !pend_table || !pending || !desc || !buf || !transport_keys || !pend_idx_out || !remote_out ||
        !claim || !status || (npeers && !peers) || n > 0xFFFFFFFFull)
        return set_err(RG_EINVAL, "handshake finish: bad args");
    if (pend_cap == 0 || (pend_cap & (pend_cap - 1)) != 0)
        return set_err(RG_EINVAL, "handshake finish: pend_cap must be a power of two");
    if (misaligned(own, 16) || misaligned(peers, 16) || misaligned(pending, 16) || misaligned(desc, 16) ||
        misaligned(transport_keys, 16) || misaligned(pend_table, 4) || misaligned(pend_idx_out, 4) ||
        misaligned(remote_out, 4) || misaligned(claim, 4))
        return set_err(RG_EINVAL, "handshake finish: own, peers, pending, desc and transport_keys must be 16-byte "
                                  "aligned, pend_table, pend_idx_out, remote_out and claim 4-byte aligned");
    rg::HsFinishArgs a{};
    a.own = reinterpret_cast<const uint32_t *>(own);
    a.peers = reinterpret_cast<const uint32_t *>(peers);
    a.npeers = npeers;
    a.table = pend_table;
    a.cap = pend_cap;
    a.pending = reinterpret_cast<uint4 *>(pending);
    a.npending = npending;
    a.desc = desc;
    a.gate = gate;
    a.buf = buf;
    a.buf_len = buf_len;
    a.tkeys = reinterpret_cast<uint4 *>(transport_keys);
    a.pend_idx = pend_idx_out;
    a.remote = remote_out;
    a.claim = claim;
    a.status = status;
    a.n = (uint32_t)n;
    hipStream_t s = (hipStream_t)stream;
    if (npending) RG_HIP(hipMemsetAsync(claim, 0xFF, (size_t)npending * sizeof(uint32_t), s), "handshake finish claim");
    hipLaunchKernelGGL(rg::handshake_finish_kernel, dim3(grid(n)), dim3(rg::kHsWG), 0, s, a);
    RG_HIP(hipGetLastError(), "handshake finish launch");
    hipLaunchKernelGGL(rg::handshake_commit_kernel, dim3(grid(n)), dim3(rg::kHsWG), 0, s, a);
    RG_HIP(hipGetLastError(), "handshake finish commit launch");
    return RG_OK;
}
