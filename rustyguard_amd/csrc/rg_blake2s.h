// rg_blake2s.h -- keyed BLAKE2s-128 device functions shared by the handshake
// kernels (rg_mac.hip, rg_cookie.hip): Core::blake2s_mac (prim.rs:123-131,
// blake2s_simd with hash_length 16).
//
// BLAKE2s (RFC 7693) is 32-bit ARX like ChaCha20 -- 10 rounds of 8 G mixes
// over a 16-word state, rotations right by 16/12/8/7 -- so it runs on the
// same VALU idioms (byte rotations as v_perm_b32); the message schedule sigma
// is resolved at compile time (fully unrolled rounds, message words in VGPRs).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rg {

__device__ __forceinline__ uint32_t rotr(uint32_t v, int n) { return __builtin_rotateright32(v, n); }
__device__ __forceinline__ uint32_t rotr16(uint32_t v) { return __builtin_amdgcn_perm(v, v, 0x01000302u); }
__device__ __forceinline__ uint32_t rotr8(uint32_t v) { return __builtin_amdgcn_perm(v, v, 0x00030201u); }

constexpr uint32_t kIV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au,
                             0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
constexpr uint8_t kSigma[10][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};

#define B2S_G(a, b, c, d, x, y)                        \
    a = a + b + (x); d = rotr16(d ^ a);                 \
    c = c + d; b = rotr(b ^ c, 12);                     \
    a = a + b + (y); d = rotr8(d ^ a);                  \
    c = c + d; b = rotr(b ^ c, 7);

// RFC 7693 §3.2 compression F; t = bytes hashed so far including this block
__device__ __forceinline__ void b2s_compress(uint32_t h[8], const uint32_t m[16], uint32_t t, bool last) {
    uint32_t v0 = h[0], v1 = h[1], v2 = h[2], v3 = h[3], v4 = h[4], v5 = h[5], v6 = h[6], v7 = h[7];
    uint32_t v8 = kIV[0], v9 = kIV[1], v10 = kIV[2], v11 = kIV[3];
    uint32_t v12 = kIV[4] ^ t, v13 = kIV[5], v14 = last ? ~kIV[6] : kIV[6], v15 = kIV[7];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint8_t *s = kSigma[r];
        B2S_G(v0, v4, v8, v12, m[s[0]], m[s[1]]);
        B2S_G(v1, v5, v9, v13, m[s[2]], m[s[3]]);
        B2S_G(v2, v6, v10, v14, m[s[4]], m[s[5]]);
        B2S_G(v3, v7, v11, v15, m[s[6]], m[s[7]]);
        B2S_G(v0, v5, v10, v15, m[s[8]], m[s[9]]);
        B2S_G(v1, v6, v11, v12, m[s[10]], m[s[11]]);
        B2S_G(v2, v7, v8, v13, m[s[12]], m[s[13]]);
        B2S_G(v3, v4, v9, v14, m[s[14]], m[s[15]]);
    }
    h[0] ^= v0 ^ v8; h[1] ^= v1 ^ v9; h[2] ^= v2 ^ v10; h[3] ^= v3 ^ v11;
    h[4] ^= v4 ^ v12; h[5] ^= v5 ^ v13; h[6] ^= v6 ^ v14; h[7] ^= v7 ^ v15;
}
#undef B2S_G

// little-endian word at msg + byte, zero past len (byte loads: only for
// lengths or mac offsets that are not multiples of 4, which no handshake
// message has)
__device__ __forceinline__ uint32_t msg_word(const uint8_t *msg, uint32_t len, uint32_t byte) {
    uint32_t w = 0;
    for (uint32_t b = 0; b < 4; ++b)
        if (byte + b < len) w |= (uint32_t)msg[byte + b] << (8 * b);
    return w;
}

// the 16-byte piece p of a 16-byte aligned message, words past len zeroed
// (a partial last word keeps its low len % 4 bytes).  Only pieces starting
// below len are read; they end inside the frame, since the mac field follows.
__device__ __forceinline__ void msg_piece(const uint8_t *msg, uint32_t len, uint32_t p, uint32_t m[4]) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (16 * p < len) v = *reinterpret_cast<const uint4 *>(msg + 16 * p);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t byte = 16 * p + 4 * i;
        const uint32_t have = byte >= len ? 0u : min(len - byte, 4u);
        m[i] = have == 4 ? w[i] : w[i] & ((1u << (8 * have)) - 1u);
    }
}

// h after the key block (RFC 7693 §3.3: the zero-padded key is block 1 and,
// for a non-empty message, never the last block), so it depends on the key
// alone and is computed once per key (mac_key_state_kernel; once per workgroup
// in cookie_reply_kernel)
__device__ __forceinline__ void b2s_key_state(const uint32_t *key, uint32_t key_len, bool last, uint32_t h[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = kIV[i];
    h[0] ^= 0x01010000u ^ (key_len << 8) ^ 16u;
    uint32_t m[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] = (uint32_t)(4 * i) < key_len ? key[i] : 0u;
    b2s_compress(h, m, 64, last);
}

// keyed BLAKE2s with a 16-byte digest of msg[0, len), len > 0, from the key
// state; returns the digest's first 4 words
__device__ __forceinline__ uint4 b2s_mac16(const uint32_t ks[8], const uint8_t *msg, uint32_t len) {
    uint32_t h[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = ks[i];
    uint32_t t = 64;
    for (uint32_t off = 0; off < len; off += 64) {
        const uint32_t rem = len - off;
        const bool last = rem <= 64;
        uint32_t m[16];
#pragma unroll
        for (int p = 0; p < 4; ++p) msg_piece(msg + off, rem, p, m + 4 * p);
        t += last ? rem : 64;
        b2s_compress(h, m, t, last);
    }
    return make_uint4(h[0], h[1], h[2], h[3]);
}

// ------------------------------------------------ the handshake's hash, HMAC and HKDF (rg_handshake.hip)
// Core::blake2s_hash, hmac_blake2s and hkdf_blake2s (prim.rs:41-72, :116-157) on words, for the lengths the
// IKpsk2 transcript has.  Lengths and output counts are run-time values so that one call site serves
// several steps of the handshake (the compression function is ~1100 instructions per site); none of them
// depends on a secret.

// unkeyed BLAKE2s with a 32-byte digest: the parameter block alone
__device__ __forceinline__ void b2s_init32(uint32_t h[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = kIV[i];
    h[0] ^= 0x01010020u;
}

// out = BLAKE2s-256(a || b) for a 32-byte a and nbw <= 12 words of b (words of b past nbw must be zero):
// HandshakeState::mix_hash.  One block up to 64 bytes in all, else two.
__device__ __forceinline__ void b2s_hash32(const uint32_t a[8], const uint32_t b[12], uint32_t nbw, uint32_t out[8]) {
    uint32_t h[8], m[16];
    b2s_init32(h);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        m[i] = a[i];
        m[8 + i] = b[i];
    }
    const bool two = nbw > 8;
    b2s_compress(h, m, two ? 64u : 32u + 4u * nbw, !two);
    if (two) {
#pragma unroll
        for (int i = 0; i < 16; ++i) m[i] = i < 4 ? b[8 + i] : 0u;
        b2s_compress(h, m, 32u + 4u * nbw, true);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = h[i];
}

// out = HMAC-BLAKE2s(key, msg) for a 32-byte key and len <= 33 message bytes in m[9] (zero past len).  The
// two passes (ipad, opad) share their code; an empty message makes the pad block the hash's only block.
__device__ __forceinline__ void b2s_hmac(const uint32_t key[8], const uint32_t m[9], uint32_t len, uint32_t out[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = 0;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        const uint32_t pad = pass ? 0x5C5C5C5Cu : 0x36363636u;
        const uint32_t mlen = pass ? 32u : len;
        uint32_t h[8], blk[16];
        b2s_init32(h);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            blk[i] = key[i] ^ pad;
            blk[8 + i] = pad;
        }
        b2s_compress(h, blk, 64, mlen == 0);
        if (mlen != 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) blk[i] = i < 8 ? (pass ? out[i] : m[i]) : (i == 8 && !pass) ? m[8] : 0u;
            b2s_compress(h, blk, 64 + mlen, true);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) out[i] = h[i]; // the inner digest after pass 0, the MAC after pass 1
    }
}

// hkdf_blake2s (prim.rs:145-157): chain = T(1), o1 = T(2), o2 = T(3) of HKDF(chain, msg) for nout = 0, 1 or 2
// further outputs (mix_chain, mix_key, mix_key_and_hash; split with an empty msg).  msg: len = 0 or 32 bytes.
__device__ __forceinline__ void b2s_hkdf(uint32_t chain[8], const uint32_t msg[8], uint32_t len, uint32_t nout,
                                         uint32_t o1[8], uint32_t o2[8]) {
    uint32_t key[8], m[9], t[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        key[i] = chain[i];
        m[i] = len ? msg[i] : 0u;
    }
    m[8] = 0;
    uint32_t mlen = len;
#pragma unroll 1
    for (uint32_t step = 0; step <= nout + 1; ++step) { // step 0: the PRK; step i: T(i) = HMAC(PRK, T(i-1) || i)
        b2s_hmac(key, m, mlen, t);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (step == 0) key[i] = t[i];
            if (step == 1) chain[i] = t[i];
            if (step == 2) o1[i] = t[i];
            if (step == 3) o2[i] = t[i];
            m[i] = step == 0 ? 0u : t[i];
        }
        m[0] = step == 0 ? 1u : m[0];
        m[8] = step == 0 ? 0u : step + 1;
        mlen = step == 0 ? 1u : 33u;
    }
}

} // namespace rg
