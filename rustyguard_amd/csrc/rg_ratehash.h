// rg_ratehash.h -- the rate limiter's key and column (include/rg_aead.h, "device-resident handshake rate limiter"),
// written once for the kernels of rg_ratelimit.hip and for the host function rg_rate_column, so that the two cannot
// drift.  Plain integer code: nothing here reads memory.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RG_RATE_HD __host__ __device__ __forceinline__
#else
#define RG_RATE_HD inline
#endif

namespace rg {

// The key of a source address (rustyguard-core/src/lib.rs:509-512) from its first two 8-byte words as a
// little-endian load gives them: w0 = ip[0..8], w1 = ip[8..16].  ip[4..16] all zero is IPv4: the big-endian u32 of
// ip[0..4]; everything else is keyed by its /64: the big-endian u64 of ip[0..8].  The port is not part of it.
RG_RATE_HD uint64_t rate_key(uint64_t w0, uint64_t w1) {
    if ((w0 >> 32) == 0 && w1 == 0) return __builtin_bswap32((uint32_t)w0);
    return __builtin_bswap64(w0);
}

// the high 64 bits of the 128-bit product x * y
RG_RATE_HD uint64_t rate_mulhi(uint64_t x, uint64_t y) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(x, y);
#else
    return (uint64_t)(((unsigned __int128)x * y) >> 64);
#endif
}
// low 64 bits XOR high 64 bits of x * y
RG_RATE_HD uint64_t rate_fold(uint64_t x, uint64_t y) { return (x * y) ^ rate_mulhi(x, y); }

// the keyed 64-bit hash of one sketch row, seeded with (a, b)
RG_RATE_HD uint64_t rate_hash(uint64_t key, uint64_t a, uint64_t b) {
    return rate_fold(rate_fold(key ^ a, 0x9E3779B97F4A7C15ull) ^ b, 0xD6E8FEB86659FD93ull);
}

// the column of `key` in a row of `width` buckets: the hash's high word scaled into [0, width)
RG_RATE_HD uint32_t rate_column(uint64_t key, uint64_t a, uint64_t b, uint32_t width) {
    return (uint32_t)(((rate_hash(key, a, b) >> 32) * width) >> 32);
}

} // namespace rg
