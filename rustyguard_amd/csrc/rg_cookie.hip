// rg_cookie.hip -- the handshake path of a server under load, batched and fused:
// HasMac::verify with overload = true (rustyguard-crypto/src/lib.rs:114-140)
// and, for every message whose mac2 fails, Sessions::write_cookie_message
// (rustyguard-core/src/lib.rs:517-540).  One message per lane:
//
//   mac1   = BLAKE2s-128(mac1_key, msg[..len-32])           2 / 1 compressions (148 / 92 bytes)
//   cookie = BLAKE2s-128(secret, addr[0..18])               1
//   mac2   = BLAKE2s-128(cookie, msg[..len-16])             1 + 3 / 1 + 2 (the 16-byte cookie is a key
//                                                           of its own: its key block is per lane)
//   reply  = XChaCha20-Poly1305(cookie_key, nonce, aad = mac1 field, pt = cookie):
//            HChaCha20, ChaCha20 blocks 0 (Poly1305 key) and 1 (keystream), three Poly1305 blocks
//
// The states after the mac1_key block and after the secret block depend on the
// call's keys alone: two lanes of each workgroup compute them (one compression
// each, side by side in one wave) and hand them to the other 254 through LDS.
// Nothing derived from the keys is written to global memory.  Under a flood
// nearly every lane writes a reply, so that path is straight-line per lane.
//
// The entry point's host side is here too (argument checks, device guard,
// launch), on rg_host.h like the host units: those are also linked against a
// CPU stand-in of the launchers (tests/sanitize) and so name no launcher of
// this file.
#include "rg_host.h"
#include "rg_noise.h"

namespace rg {
namespace {

struct CookieArgs {
    const uint32_t *keys;    // rg_cookie_keys as LE words: [0, 8) mac1_key, [8, 16) cookie_key, [16, 24) secret
    const rg_pkt_desc *desc; // [n]
    const uint8_t *addrs;    // [n][24]
    const uint8_t *overload; // [n] or nullptr
    const uint8_t *nonces;   // [n][24]
    const uint8_t *buf;
    uint64_t buf_len;
    uint8_t *replies; // [n][64]
    uint8_t *status;  // [n]
    uint32_t n;
};

// the 16-byte mac field at msg + at (a multiple of 4, not of 16: 116 / 132 and 60 / 76)
__device__ __forceinline__ uint4 mac_field(const uint8_t *msg, uint32_t at) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(msg + at);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ uint32_t mac_diff(const uint4 &a, const uint4 &b) {
    return (a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w);
}

__global__ __launch_bounds__(256) void cookie_reply_kernel(CookieArgs a) {
    __shared__ uint32_t s_ks[2][8]; // BLAKE2s states after the mac1_key block and after the secret block
    if (threadIdx.x < 2) {
        uint32_t h[8];
        b2s_key_state(a.keys + (threadIdx.x ? 16 : 0), 32, false, h);
#pragma unroll
        for (int w = 0; w < 8; ++w) s_ks[threadIdx.x][w] = h[w];
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const rg_pkt_desc d = a.desc[i];
    uint32_t st = frame_verdict(d, RG_PKT_OK, a.buf_len, kInitLen, kRespLen); // no gate
    if (st == kGoing) {
        const uint8_t *msg = a.buf + d.offset;
        const uint4 head = *reinterpret_cast<const uint4 *>(msg); // type, sender, ...
        if (head.x != (d.len == kInitLen ? 1u : 2u)) st = RG_PKT_INVALID; // Error::InvalidMessage
        else {
            uint32_t ks[8];
#pragma unroll
            for (int w = 0; w < 8; ++w) ks[w] = s_ks[0][w];
            const uint4 mac1 = mac_field(msg, d.len - 32);
            const bool overloaded = !a.overload || a.overload[i] != 0;
            if (mac_diff(b2s_mac16(ks, msg, d.len - 32), mac1) != 0) st = RG_PKT_REJECTED; // CryptoError::Rejected
            else if (!overloaded) st = RG_PKT_OK;
            else {
                // CookieState::new_cookie: the 18 address bytes are the last block under the secret
                const uint2 *ap = reinterpret_cast<const uint2 *>(a.addrs + 24ull * i);
                const uint2 a0 = ap[0], a1 = ap[1], a2 = ap[2];
                uint32_t m[16] = {a0.x, a0.y, a1.x, a1.y, a2.x & 0xFFFFu};
                uint32_t h[8];
#pragma unroll
                for (int w = 0; w < 8; ++w) h[w] = s_ks[1][w];
                b2s_compress(h, m, 64 + 18, true);
                const uint4 cookie = make_uint4(h[0], h[1], h[2], h[3]);
                b2s_key_state(h, 16, false, ks); // keyed by the cookie: the digest's first 16 bytes
                if (mac_diff(b2s_mac16(ks, msg, d.len - 16), mac_field(msg, d.len - 16)) == 0) st = RG_PKT_OK;
                else {
                    // write_cookie_message: encrypt_cookie(cookie, cookie_key, nonce, aad = mac1)
                    const uint2 *np = reinterpret_cast<const uint2 *>(a.nonces + 24ull * i);
                    const uint2 n0 = np[0], n1 = np[1], n2 = np[2];
                    const uint32_t nonce[6] = {n0.x, n0.y, n1.x, n1.y, n2.x, n2.y};
                    uint32_t tag[4];
                    const uint4 ct = cookie_aead(load_key(a.keys, 1), nonce, mac1, cookie, true, tag);
                    // CookieMessage {type = 3, receiver = the message's sender, nonce, cookie, tag}
                    uint4 *out = reinterpret_cast<uint4 *>(a.replies + 64ull * i);
                    out[0] = make_uint4(3u, head.y, n0.x, n0.y);
                    out[1] = make_uint4(n1.x, n1.y, n2.x, n2.y);
                    out[2] = ct;
                    out[3] = make_uint4(tag[0], tag[1], tag[2], tag[3]);
                    st = RG_PKT_COOKIE;
                }
            }
        }
    }
    a.status[i] = (uint8_t)st;
}

} // namespace
} // namespace rg

extern "C" int rg_cookie_reply_batch_dev(rg_ctx *ctx, const rg_cookie_keys *keys, const rg_pkt_desc *desc,
                                         const rg_src_addr *addrs, const uint8_t *overload, const uint8_t *nonces,
                                         size_t n, const uint8_t *buf, size_t buf_len, uint8_t *replies,
                                         uint8_t *status, void *stream) {
    using namespace rg::host;
    rg::DeviceGuard dg_;
    const int rc = check_ctx(ctx);
    if (rc) return rc;
    if (n == 0) return RG_OK;
    if (!keys || !desc || !addrs || !nonces || !buf || !replies || !status || n > 0xFFFFFFFFull)
        return bad("cookie reply", "bad args");
    if (misaligned(keys, 16) || misaligned(replies, 16))
        return bad("cookie reply", "keys and replies must be 16-byte aligned");
    if (misaligned(addrs, 8) || misaligned(nonces, 8))
        return bad("cookie reply", "addrs and nonces must be 8-byte aligned");
    rg::CookieArgs a{};
    a.keys = reinterpret_cast<const uint32_t *>(keys);
    a.desc = desc;
    a.addrs = reinterpret_cast<const uint8_t *>(addrs);
    a.overload = overload;
    a.nonces = nonces;
    a.buf = buf;
    a.buf_len = buf_len;
    a.replies = replies;
    a.status = status;
    a.n = (uint32_t)n;
    hipLaunchKernelGGL(rg::cookie_reply_kernel, lanes(n), kWg, 0, (hipStream_t)stream, a);
    RG_HIP(hipGetLastError(), "cookie reply launch");
    return RG_OK;
}
