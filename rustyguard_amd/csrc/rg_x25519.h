// rg_x25519.h -- arithmetic mod p = 2^255 - 19 and the X25519 function of RFC 7748 §5, written once for the
// host and the device: CryptoPrimatives::x25519 / x25519_pubkey (rustyguard-crypto/src/prim.rs:79-80,
// :159-177).  The device half runs in rg_handshake.hip, one lane per scalar multiplication; the host half
// exists so that every carry edge can be tested on a CPU under sanitizers (tests/x25519_host/driver.cpp).
//
// Layout: ten unsigned limbs of alternating 26 and 25 bits (radix 2^25.5), limb i at bit ceil(25.5 i).  The
// 32 x 32 -> 64 multiply-add (v_mad_u64_u32) takes a whole limb product, and 2^255 == 19 folds the upper
// half of a product back with one multiplication by 19 per limb.  Bounds, with "carried" meaning what
// fe_mul / fe_mul121665 return (limb 1 < 2^25 + 2^17, every other even limb < 2^26, odd limb < 2^25):
//   fe_add of two carried values      even limbs < 2^27,    odd limbs < 2^26 + 2^18
//   fe_sub of two carried values      even limbs < 3 2^26,  odd limbs < 3 2^25 + 2^17   (a + 2p - b, no borrow)
//   fe_mul takes either of those (or carried values) on both sides: 19 g_j < 19 * 3 * 2^26 < 2^32, every
//   term < 2^27.6 * 2^31.9, ten terms per column < 2^62.8: no column overflows a u64.
// The ladder only ever multiplies carried values, one sum or one difference of them, as the RFC's formulas
// are written, so no intermediate carry pass is needed.
//
// Constant time: no branch and no address depends on a limb or on a scalar bit.  The ladder's swap is a
// mask, the scalar is walked by shifting it through its top bit (no indexed access), the final zero test
// is an OR-fold.  Every limb loop has compile-time bounds and is fully unrolled, so a Fe lives in
// registers (ten VGPRs on the device), never in scratch memory.
//
// Only uint32_t / uint64_t arithmetic; no builtins.  Squaring is fe_mul(f, f): the first working layout
// (DESIGN.md §4.10 has the measured cost and what a dedicated squaring would save).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RG_HD __host__ __device__
#else
#define RG_HD
#endif
#define RG_X_FN RG_HD static inline __attribute__((always_inline))
// limb loops are unrolled in full, the bit loops stay loops (g++ needs neither to be told)
#if defined(__clang__)
#define RG_X_UNROLL _Pragma("unroll")
#define RG_X_LOOP _Pragma("unroll 1")
#else
#define RG_X_UNROLL
#define RG_X_LOOP
#endif

namespace rg {

struct Fe {
    uint32_t v[10];
};

constexpr uint32_t kFeM26 = 0x3FFFFFFu, kFeM25 = 0x1FFFFFFu;

RG_X_FN uint32_t fe_mask(int i) { return (i & 1) ? kFeM25 : kFeM26; }
RG_X_FN int fe_bits(int i) { return (i & 1) ? 25 : 26; }

RG_X_FN Fe fe_small(uint32_t x) { // x < 2^26
    Fe r;
    r.v[0] = x;
RG_X_UNROLL
    for (int i = 1; i < 10; ++i) r.v[i] = 0;
    return r;
}

// the integer of 8 little-endian words with bit 255 masked off; values in [p, 2^255) are accepted as they
// are (RFC 7748 §5: non-canonical u-coordinates are not rejected)
RG_X_FN Fe fe_from_words(const uint32_t w[8]) {
    Fe r;
    r.v[0] = w[0] & kFeM26;
    r.v[1] = ((w[0] >> 26) | (w[1] << 6)) & kFeM25;
    r.v[2] = ((w[1] >> 19) | (w[2] << 13)) & kFeM26;
    r.v[3] = ((w[2] >> 13) | (w[3] << 19)) & kFeM25;
    r.v[4] = w[3] >> 6;
    r.v[5] = w[4] & kFeM25;
    r.v[6] = ((w[4] >> 25) | (w[5] << 7)) & kFeM26;
    r.v[7] = ((w[5] >> 19) | (w[6] << 13)) & kFeM25;
    r.v[8] = ((w[6] >> 12) | (w[7] << 20)) & kFeM26;
    r.v[9] = (w[7] >> 6) & kFeM25;
    return r;
}

// the canonical value (in [0, p)) as 8 little-endian words.  Takes limbs up to 2^28.
RG_X_FN void fe_to_words(const Fe &f, uint32_t w[8]) {
    uint32_t v[10];
RG_X_UNROLL
    for (int i = 0; i < 10; ++i) v[i] = f.v[i];
    // two carry passes: every limb inside its width, except that limb 0 may keep up to 19 above 2^26
RG_X_UNROLL
    for (int pass = 0; pass < 2; ++pass) {
RG_X_UNROLL
        for (int i = 0; i < 9; ++i) {
            v[i + 1] += v[i] >> fe_bits(i);
            v[i] &= fe_mask(i);
        }
        v[0] += 19u * (v[9] >> 25);
        v[9] &= kFeM25;
    }
    // the value is below 2^255 + 19 < 2p: q = 1 exactly when it is >= p, i.e. when value + 19 reaches 2^255
    uint32_t q = (v[0] + 19u) >> 26;
RG_X_UNROLL
    for (int i = 1; i < 10; ++i) q = (v[i] + q) >> fe_bits(i);
    v[0] += 19u * q; // value - q p = value + 19 q - q 2^255: the carry out of limb 9 is that 2^255
RG_X_UNROLL
    for (int i = 0; i < 9; ++i) {
        v[i + 1] += v[i] >> fe_bits(i);
        v[i] &= fe_mask(i);
    }
    v[9] &= kFeM25;
    w[0] = v[0] | (v[1] << 26);
    w[1] = (v[1] >> 6) | (v[2] << 19);
    w[2] = (v[2] >> 13) | (v[3] << 13);
    w[3] = (v[3] >> 19) | (v[4] << 6);
    w[4] = v[5] | (v[6] << 25);
    w[5] = (v[6] >> 7) | (v[7] << 19);
    w[6] = (v[7] >> 13) | (v[8] << 12);
    w[7] = (v[8] >> 20) | (v[9] << 6);
}

RG_X_FN void fe_words_from_bytes(const uint8_t s[32], uint32_t w[8]) {
RG_X_UNROLL
    for (int i = 0; i < 8; ++i)
        w[i] = (uint32_t)s[4 * i] | ((uint32_t)s[4 * i + 1] << 8) | ((uint32_t)s[4 * i + 2] << 16) |
               ((uint32_t)s[4 * i + 3] << 24);
}

RG_X_FN void fe_words_to_bytes(const uint32_t w[8], uint8_t s[32]) {
RG_X_UNROLL
    for (int i = 0; i < 32; ++i) s[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

RG_X_FN Fe fe_from_bytes(const uint8_t s[32]) {
    uint32_t w[8];
    fe_words_from_bytes(s, w);
    return fe_from_words(w);
}

RG_X_FN void fe_to_bytes(const Fe &f, uint8_t s[32]) {
    uint32_t w[8];
    fe_to_words(f, w);
    fe_words_to_bytes(w, s);
}

RG_X_FN Fe fe_add(const Fe &a, const Fe &b) {
    Fe r;
RG_X_UNROLL
    for (int i = 0; i < 10; ++i) r.v[i] = a.v[i] + b.v[i];
    return r;
}

// a - b as a + 2p - b, limb by limb: b carried (every limb of b at most the matching limb of 2p)
RG_X_FN Fe fe_sub(const Fe &a, const Fe &b) {
    Fe r;
    r.v[0] = a.v[0] + 0x7FFFFDAu - b.v[0];
RG_X_UNROLL
    for (int i = 1; i < 10; ++i) r.v[i] = a.v[i] + ((i & 1) ? 0x3FFFFFEu : 0x7FFFFFEu) - b.v[i];
    return r;
}

// ten 64-bit columns -> carried limbs: one pass up the limbs, the carry out of limb 9 comes back into limb 0
// times 19 and limb 0's carry goes on into limb 1 (< 2^17)
RG_X_FN Fe fe_carry(uint64_t h[10]) {
    Fe r;
RG_X_UNROLL
    for (int i = 0; i < 9; ++i) {
        h[i + 1] += h[i] >> fe_bits(i);
        r.v[i] = (uint32_t)h[i] & fe_mask(i);
    }
    const uint64_t h0 = (uint64_t)r.v[0] + 19u * (h[9] >> 25);
    r.v[9] = (uint32_t)h[9] & kFeM25;
    r.v[0] = (uint32_t)h0 & kFeM26;
    r.v[1] += (uint32_t)(h0 >> 26);
    return r;
}

// f g mod p.  Limb weights are 2^ceil(25.5 i): the product of two odd limbs carries one bit more than
// its column's weight (factor 2), and columns 10..18 fold onto 0..8 with factor 19.
RG_X_FN Fe fe_mul(const Fe &f, const Fe &g) {
    uint32_t f2[10], g19[10];
RG_X_UNROLL
    for (int i = 0; i < 10; ++i) {
        f2[i] = (i & 1) ? 2u * f.v[i] : f.v[i];
        g19[i] = 19u * g.v[i];
    }
    uint64_t h[10];
RG_X_UNROLL
    for (int k = 0; k < 10; ++k) h[k] = 0;
RG_X_UNROLL
    for (int i = 0; i < 10; ++i) {
RG_X_UNROLL
        for (int j = 0; j < 10; ++j) {
            const int k = i + j;
            const uint32_t fi = ((i & 1) && (j & 1)) ? f2[i] : f.v[i];
            const uint32_t gj = k >= 10 ? g19[j] : g.v[j];
            h[k % 10] += (uint64_t)fi * gj;
        }
    }
    return fe_carry(h);
}

RG_X_FN Fe fe_sq(const Fe &f) { return fe_mul(f, f); }

// 121665 f = (A - 2) / 4 times f, the ladder's a24 step
RG_X_FN Fe fe_mul121665(const Fe &f) {
    uint64_t h[10];
RG_X_UNROLL
    for (int i = 0; i < 10; ++i) h[i] = (uint64_t)f.v[i] * 121665u;
    return fe_carry(h);
}

RG_X_FN Fe fe_sqn(Fe t, int n) {
RG_X_LOOP
    for (int i = 0; i < n; ++i) t = fe_sq(t);
    return t;
}

// z^(p-2) = z^(2^255 - 21) by the usual addition chain (254 squarings, 11 multiplications); 0 -> 0
RG_X_FN Fe fe_invert(const Fe &z) {
    const Fe z2 = fe_sq(z);
    const Fe z9 = fe_mul(fe_sqn(z2, 2), z);
    const Fe z11 = fe_mul(z9, z2);
    const Fe z2_5_0 = fe_mul(fe_sq(z11), z9);                  // 2^5 - 2^0
    const Fe z2_10_0 = fe_mul(fe_sqn(z2_5_0, 5), z2_5_0);      // 2^10 - 2^0
    const Fe z2_20_0 = fe_mul(fe_sqn(z2_10_0, 10), z2_10_0);   // 2^20 - 2^0
    const Fe z2_40_0 = fe_mul(fe_sqn(z2_20_0, 20), z2_20_0);   // 2^40 - 2^0
    const Fe z2_50_0 = fe_mul(fe_sqn(z2_40_0, 10), z2_10_0);   // 2^50 - 2^0
    const Fe z2_100_0 = fe_mul(fe_sqn(z2_50_0, 50), z2_50_0);  // 2^100 - 2^0
    const Fe z2_200_0 = fe_mul(fe_sqn(z2_100_0, 100), z2_100_0); // 2^200 - 2^0
    const Fe z2_250_0 = fe_mul(fe_sqn(z2_200_0, 50), z2_50_0); // 2^250 - 2^0
    return fe_mul(fe_sqn(z2_250_0, 5), z11);                   // 2^255 - 21
}

// swap a and b when bit is 1, by mask
RG_X_FN void fe_cswap(Fe &a, Fe &b, uint32_t bit) {
    const uint32_t m = 0u - bit;
RG_X_UNROLL
    for (int i = 0; i < 10; ++i) {
        const uint32_t t = m & (a.v[i] ^ b.v[i]);
        a.v[i] ^= t;
        b.v[i] ^= t;
    }
}

// X25519(k, u) of RFC 7748 §5 on little-endian words: the scalar is clamped here, u's bit 255 is masked.
// Returns the OR of the output words: 0 exactly when the result is all zero, X25519's only failure
// (RFC 7748 §6.1: u of small order), for which out is 8 zero words.
RG_X_FN uint32_t x25519_words(const uint32_t k[8], const uint32_t u[8], uint32_t out[8]) {
    // clamp (k[0] &= ~7, bit 255 cleared, bit 254 set), then move bit 254 to the top of the register
    uint32_t s[8];
RG_X_UNROLL
    for (int i = 0; i < 8; ++i) s[i] = k[i];
    s[0] &= ~7u;
    s[7] = (s[7] & 0x7FFFFFFFu) | 0x40000000u;
RG_X_UNROLL
    for (int i = 7; i > 0; --i) s[i] = (s[i] << 1) | (s[i - 1] >> 31);
    s[0] <<= 1;
    const Fe x1 = fe_from_words(u);
    Fe x2 = fe_small(1), z2 = fe_small(0), x3 = x1, z3 = fe_small(1);
    uint32_t swap = 0;
RG_X_LOOP
    for (int t = 254; t >= 0; --t) {
        const uint32_t kt = s[7] >> 31;
RG_X_UNROLL
        for (int i = 7; i > 0; --i) s[i] = (s[i] << 1) | (s[i - 1] >> 31);
        s[0] <<= 1;
        swap ^= kt;
        fe_cswap(x2, x3, swap);
        fe_cswap(z2, z3, swap);
        swap = kt;
        const Fe a = fe_add(x2, z2), b = fe_sub(x2, z2);
        const Fe aa = fe_sq(a), bb = fe_sq(b);
        const Fe e = fe_sub(aa, bb);
        const Fe c = fe_add(x3, z3), d = fe_sub(x3, z3);
        const Fe da = fe_mul(d, a), cb = fe_mul(c, b);
        x3 = fe_sq(fe_add(da, cb));
        z3 = fe_mul(x1, fe_sq(fe_sub(da, cb)));
        x2 = fe_mul(aa, bb);
        z2 = fe_mul(e, fe_add(aa, fe_mul121665(e)));
    }
    fe_cswap(x2, x3, swap);
    fe_cswap(z2, z3, swap);
    fe_to_words(fe_mul(x2, fe_invert(z2)), out);
    uint32_t nz = 0;
RG_X_UNROLL
    for (int i = 0; i < 8; ++i) nz |= out[i];
    return nz;
}

} // namespace rg
