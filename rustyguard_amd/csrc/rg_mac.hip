// rg_mac.hip -- batched handshake MAC checks: the
// HasMac::verify_mac1 / verify_mac2 filter of rustyguard-crypto/src/lib.rs:
// 114-209, i.e. keyed BLAKE2s-128 (Core::blake2s_mac, prim.rs:123-131,
// blake2s_simd with hash_length 16) over a handshake message up to its mac
// field, compared with that field.  One message per lane; with key index
// RG_KEY_SCAN every key is tried in order and the first match is kept, as in
// wg-proxy's peer scan (wg-proxy/src/main.rs:217-229).
//
// The keyed hash starts with the zero-padded key as its own block, so the
// state after it depends on the key alone: mac_key_state_kernel computes it
// once per key (one compression of three per 148-byte initiation saved), and
// messages are read as 16-byte vectors.  The BLAKE2s device functions are
// rg_blake2s.h's, shared with rg_cookie.hip.
#include "rg_blake2s.h"
#include "rg_device.h"
#include "rg_internal.h"

namespace rg {
namespace {

__global__ __launch_bounds__(64) void mac_key_state_kernel(const uint32_t *keys, uint32_t key_len, uint32_t nkeys,
                                                          uint32_t *state) {
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    if (k >= nkeys) return;
    uint32_t h[8];
    b2s_key_state(keys + (key_len / 4) * k, key_len, false, h);
    uint4 *o = reinterpret_cast<uint4 *>(state + 8 * k);
    o[0] = make_uint4(h[0], h[1], h[2], h[3]);
    o[1] = make_uint4(h[4], h[5], h[6], h[7]);
}

__global__ __launch_bounds__(256) void mac_verify_kernel(MacArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const rg_pkt_desc d = a.desc[i];
    uint32_t found = RG_KEY_SKIP;
    uint8_t st;
    if ((d.offset & 15u) != 0) st = RG_PKT_UNALIGNED;
    else if (d.len < 32 || d.offset > a.buf_len || d.len > a.buf_len - d.offset) st = RG_PKT_INVALID;
    else {
        const uint8_t *msg = a.buf + d.offset;
        const uint32_t covered = d.len - (a.which == 2 ? 16u : 32u);
        uint4 want;
        if ((covered & 3u) == 0) {
            const uint32_t *w = reinterpret_cast<const uint32_t *>(msg + covered);
            want = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            want = make_uint4(msg_word(msg, d.len, covered), msg_word(msg, d.len, covered + 4),
                              msg_word(msg, d.len, covered + 8), msg_word(msg, d.len, covered + 12));
        }
        const bool scan = d.key_idx == RG_KEY_SCAN;
        const uint32_t lo = scan ? 0u : d.key_idx, hi = scan ? a.nkeys : min(d.key_idx + 1, a.nkeys);
        for (uint32_t k = lo; k < hi; ++k) {
            uint32_t ks[8];
            if (covered > 0) {
                const uint4 *s = reinterpret_cast<const uint4 *>(a.key_state + 8 * k);
                const uint4 s0 = s[0], s1 = s[1];
                ks[0] = s0.x; ks[1] = s0.y; ks[2] = s0.z; ks[3] = s0.w;
                ks[4] = s1.x; ks[5] = s1.y; ks[6] = s1.z; ks[7] = s1.w;
            } else { // empty covered part: the key block is the last block
                b2s_key_state(a.keys + (a.key_len / 4) * k, a.key_len, true, ks);
            }
            const uint4 mac = covered > 0 ? b2s_mac16(ks, msg, covered) : make_uint4(ks[0], ks[1], ks[2], ks[3]);
            const uint32_t diff = (mac.x ^ want.x) | (mac.y ^ want.y) | (mac.z ^ want.z) | (mac.w ^ want.w);
            if (diff == 0 && found == RG_KEY_SKIP) found = k; // first match, every key still hashed
        }
        st = found != RG_KEY_SKIP ? RG_PKT_OK : RG_PKT_REJECTED; // CryptoError::Rejected (lib.rs:146-152)
    }
    a.status[i] = st;
    if (a.key_out) a.key_out[i] = found;
}

} // namespace

hipError_t launch_mac_verify(const MacArgs &a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(mac_key_state_kernel, dim3((a.nkeys + 63) / 64), dim3(64), 0, s, a.keys, a.key_len, a.nkeys,
                       a.key_state);
    hipLaunchKernelGGL(mac_verify_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace rg
