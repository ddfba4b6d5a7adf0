// rg_noise.h -- what the handshake-side kernels share (rg_handshake.hip, rg_cookie.hip, rg_peerstate.hip), one
// copy each, all inlined:
//
//   frame_verdict, kInitLen / kRespLen / kCookieLen   the preamble of every kernel that reads a handshake-side
//                                                     message out of a frame buffer
//   load8, load_words, store_or_zero                  rows of words in and out of uint4 arrays
//   Noise                                             HandshakeState (rustyguard-crypto/src/prim.rs:227-314) and
//                                                     Encrypted<N>::{encrypt,decrypt}_and_hash (prim.rs:316-366)
//   hs_aead, tag_diff                                 the ChaCha20-Poly1305 of the handshake's fields
//   hs_mac, hs_macs                                   mac1 and mac2 of a message being built (HasMac, lib.rs:114-209)
//   cookie_aead                                       the XChaCha20-Poly1305 of a CookieMessage, seal and open
//
// Constant time: no function here branches or indexes on a key, a shared secret, a chaining key or an AEAD key.
// Every length, count and flag a function takes is public (a message type, a step count, the presence of a
// cookie); tag comparisons are OR-folds over all their words, and the caller branches on the folded verdict
// alone, which the status array publishes anyway.
//
// Code size: the BLAKE2s compression is ~1100 instructions per call site.  Lengths, output counts and the
// `keyed` / `derive` flags are run-time values so that a step loop (one X25519 ladder call site per kernel) has
// one HKDF site and one mix_hash site for all its steps.
#pragma once
#include "rg_blake2s.h"
#include "rg_device.h"

namespace rg {

constexpr uint32_t kGoing = 0xFFu; // no verdict yet (never stored)
// HandshakeInit, HandshakeResp, CookieMessage (rustyguard-types)
constexpr uint32_t kInitLen = 148, kRespLen = 92, kCookieLen = 64;

// The verdict on a frame before any of it is read: kGoing, or the status to store.  gate is the row's gate byte,
// RG_PKT_OK for a call without a gate array; the frame's length must be len_a or len_b.
__device__ __forceinline__ uint32_t frame_verdict(const rg_pkt_desc &d, uint32_t gate, uint64_t buf_len, uint32_t len_a,
                                                  uint32_t len_b) {
    if ((d.offset & 15u) != 0) return RG_PKT_UNALIGNED;
    if (d.offset > buf_len || d.len > buf_len - d.offset || (d.len != len_a && d.len != len_b)) return RG_PKT_INVALID;
    if (gate != RG_PKT_OK || d.key_idx == RG_KEY_SKIP) return RG_PKT_REJECTED;
    return kGoing;
}
__device__ __forceinline__ uint32_t frame_verdict(const rg_pkt_desc &d, uint32_t gate, uint64_t buf_len, uint32_t len) {
    return frame_verdict(d, gate, buf_len, len, len);
}

// ------------------------------------------------------------------- rows
__device__ __forceinline__ void load8(const uint32_t *p, uint32_t w[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = p[i];
}

// NW words (a multiple of 4) from 16-byte aligned memory
template <int NW> __device__ __forceinline__ void load_words(const uint4 *p, uint32_t *w) {
#pragma unroll
    for (int q = 0; q < NW / 4; ++q) {
        const uint4 v = p[q];
        w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
}

// the words of a row that passed, zeros for one that failed: a select on the public verdict
__device__ __forceinline__ void store_or_zero(uint4 *dst, const uint32_t *w, int quads, bool ok) {
#pragma unroll
    for (int q = 0; q < quads; ++q)
        dst[q] = ok ? make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]) : make_uint4(0, 0, 0, 0);
}

__device__ __forceinline__ uint32_t tag_diff(const uint32_t tag[4], const uint32_t *w) {
    uint32_t diff = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) diff |= tag[q] ^ w[q];
    return diff;
}

// ------------------------------------------------------------ field AEAD
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

// ------------------------------------------------- Noise symmetric state
// HandshakeState::default(): BLAKE2s("Noise_IKpsk2_25519_ChaChaPoly_BLAKE2s") and
// BLAKE2s(that || "WireGuard v1 zx2c4 Jason@zx2c4.com"), as little-endian words
__device__ constexpr uint32_t kConstruction[8] = {0xAE6DE260u, 0xC0EF27F3u, 0xE235C32Eu, 0xD0D225A0u,
                                                  0x0642EB16u, 0xF57772F8u, 0x98D1382Du, 0x36CD788Bu};
__device__ constexpr uint32_t kIdentifier[8] = {0x61B31122u, 0x66C51A08u, 0xDB431269u, 0x32D58A45u,
                                                0x666C9C2Du, 0xB7E89322u, 0x659CE10Eu, 0xF39E07BAu};

// The members are the reference's methods of the same names.  Arrays handed to mix_hash, and the field arrays
// of the two *_and_hash members, are 12 words long and zero past the words that count.
// The state's words are two arrays of the kernel's own, `uint32_t chain[8], hash[8]; Noise ns{chain, hash};`:
// as members of one 16-word struct the optimiser left the whole chaining key in a stack slot (96 bytes of
// scratch in each of the four kernels), as arrays of their own they stay in registers as before.
struct Noise {
    uint32_t (&chain)[8], (&hash)[8];

    __device__ __forceinline__ void init() {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            chain[i] = kConstruction[i];
            hash[i] = kIdentifier[i];
        }
    }

    __device__ __forceinline__ void mix_hash(const uint32_t w[12], uint32_t nwords) {
        uint32_t nh[8];
        b2s_hash32(hash, w, nwords, nh);
#pragma unroll
        for (int i = 0; i < 8; ++i) hash[i] = nh[i];
    }

    // derive = false is mix_chain ("like mix-key, but discards the unused key": it is not computed, and
    // key_out is not written); a step loop whose first token has no key passes the public step count here
    __device__ __forceinline__ void mix_key(const uint32_t dh[8], uint32_t key_out[8], bool derive = true) {
        uint32_t none[8];
        b2s_hkdf(chain, dh, 32, derive ? 1 : 0, key_out, none);
    }

    __device__ __forceinline__ void mix_chain(const uint32_t dh[8]) {
        uint32_t none[8];
        b2s_hkdf(chain, dh, 32, 0, none, none);
    }

    __device__ __forceinline__ void mix_key_and_hash(const uint32_t psk[8], uint32_t key_out[8]) {
        uint32_t t[12] = {};
        b2s_hkdf(chain, psk, 32, 2, t, key_out);
        mix_hash(t, 8);
    }

    // chain becomes the first transport key (the initiator's send key), second_out the other one
    __device__ __forceinline__ void split(uint32_t second_out[8]) {
        uint32_t zero[8] = {}, none[8];
        b2s_hkdf(chain, zero, 0, 1, second_out, none);
    }

    // out = ciphertext || tag of the len-byte field pt (len = 32 or 12) under aad = hash, then mix_hash(out).
    // keyed = false is the Noise specification's EncryptAndHash before any key is set: the field (32 bytes,
    // the ephemeral public key) goes into the message as it is, and only the mix_hash remains.
    __device__ __forceinline__ void encrypt_and_hash(const uint32_t key[8], bool keyed, const uint32_t pt[8],
                                                     uint32_t len, uint32_t out[12]) {
        uint32_t ct[8], stream[16], tag[4] = {};
#pragma unroll
        for (int q = 0; q < 8; ++q) ct[q] = pt[q];
        if (keyed) hs_aead(key, hash, ct, len, stream, tag, true);
#pragma unroll
        for (int q = 0; q < 12; ++q)
            out[q] = len == 32 ? (q < 8 ? ct[q] : tag[q - 8]) : (q < 3 ? ct[q] : q < 7 ? tag[q - 3] : 0u);
        mix_hash(out, keyed ? len / 4 + 4 : len / 4);
    }

    // f = ciphertext || tag of a len-byte field (len = 32 or 12): false when the tag fails (an OR-fold over its
    // words; the state is then as it was), else pt = the plaintext, zero past len bytes, after mix_hash(f)
    __device__ __forceinline__ bool decrypt_and_hash(const uint32_t key[8], const uint32_t f[12], uint32_t len,
                                                     uint32_t pt[8]) {
        uint32_t ct[8], stream[16], tag[4];
#pragma unroll
        for (int q = 0; q < 8; ++q) ct[q] = (uint32_t)(4 * q) < len ? f[q] : 0u;
        hs_aead(key, hash, ct, len, stream, tag);
        if (tag_diff(tag, len == 32 ? f + 8 : f + 3) != 0) return false;
        mix_hash(f, len / 4 + 4);
#pragma unroll
        for (int q = 0; q < 8; ++q) pt[q] = ct[q] ^ stream[q];
        return true;
    }

    // the tag of the empty payload under aad = hash (EncryptedEmpty).  The mix_hash that follows it in the
    // reference feeds nothing that leaves the handshake and is not computed.
    __device__ __forceinline__ void empty_tag(const uint32_t key[8], uint32_t tag[4]) const {
        uint32_t zero[8] = {}, stream[16];
        hs_aead(key, hash, zero, 0, stream, tag);
    }
};

// ------------------------------------------------------------ mac1, mac2
// BLAKE2s-128(key, the first NW words of w): mac1 under a 32-byte key, mac2 under a 16-byte cookie
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

// The two macs that end a message of NW words: mac1 = BLAKE2s-128(mac1_key, w[0, NW - 8)) into w[NW - 8, NW - 4),
// and, when the peer gave us a cookie (cookie != nullptr: 4 words), mac2 = BLAKE2s-128(cookie, w[0, NW - 4)) into
// w[NW - 4, NW); without one mac2 stays as the caller left it, zero.
template <int NW> __device__ __forceinline__ void hs_macs(uint32_t *w, const uint32_t *mac1_key, const uint32_t *cookie) {
    uint32_t k[8], m[4];
    load8(mac1_key, k);
    hs_mac<NW - 8>(k, 32, w, m);
#pragma unroll
    for (int q = 0; q < 4; ++q) w[NW - 8 + q] = m[q];
    if (cookie) {
#pragma unroll
        for (int q = 0; q < 8; ++q) k[q] = q < 4 ? cookie[q] : 0u;
        hs_mac<NW - 4>(k, 16, w, m);
#pragma unroll
        for (int q = 0; q < 4; ++q) w[NW - 4 + q] = m[q];
    }
}

// ------------------------------------------------------------ cookie AEAD
// XChaCha20-Poly1305 of a CookieMessage (encrypt_cookie / decrypt_cookie): one 16-byte block `in` under
// cookie_key and the 24-byte nonce, aad = the 16-byte mac1 field.  Returns in ^ keystream; tag is over the
// ciphertext, which is that result for a seal and `in` for an open.
__device__ __forceinline__ uint4 cookie_aead(const Key8 &cookie_key, const uint32_t nonce[6], const uint4 &mac1,
                                             const uint4 &in, bool seal, uint32_t tag[4]) {
    const Key8 sub = hchacha20(cookie_key, nonce);
    uint32_t otk[16], stream[16];
    chacha_block(sub, 0, 0, nonce[4], nonce[5], otk); // one-time Poly1305 key
    chacha_block(sub, 1, 0, nonce[4], nonce[5], stream);
    const uint4 out = make_uint4(in.x ^ stream[0], in.y ^ stream[1], in.z ^ stream[2], in.w ^ stream[3]);
    const Mul r = make_mul(otk[0], otk[1], otk[2], otk[3]);
    Acc acc = {0, 0, 0, 0, 0};
    acc_block(acc, mac1, r);                             // AAD: 16 bytes, no padding
    acc_block(acc, seal ? out : in, r);                  // ciphertext: 16 bytes
    acc_block(acc, make_uint4(16u, 0u, 16u, 0u), r);     // le64(aad_len) || le64(ct_len)
    acc_finish(acc, otk[4], otk[5], otk[6], otk[7], tag);
    return out;
}

} // namespace rg
