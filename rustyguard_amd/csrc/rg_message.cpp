// rg_message.cpp -- the per-message CryptoPrimatives drop-in of include/rg_aead.h: one message of any
// nonce, AAD and length through the general kernel, on the context's own stream.
#include "rg_host.h"

using namespace rg::host;

// nonce: 12 bytes, or 24 for XChaCha20-Poly1305 (xchacha)
static int general_one(rg_ctx *ctx, bool dec, const uint8_t key[32], const uint8_t *nonce, const uint8_t *aad,
                       size_t aad_len, uint8_t *payload, size_t len, uint8_t tag[16], bool xchacha = false) {
    rg::DeviceGuard dg_;
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if (!key || !nonce || !tag || (aad_len && !aad) || (len && !payload))
        return set_err(RG_EINVAL, "aead: bad args");
    // chunk c takes block counter c + 1 and counter 0 is the Poly1305 key block: 2^32 - 1 chunks at the most
    // (RFC 8439 §2.8), or the last chunk's counter would wrap onto it
    if (len > 64ull * 0xFFFFFFFFull) return set_err(RG_EINVAL, "aead: message too long for a 32-bit block counter");
    std::lock_guard<std::mutex> g(ctx->mu);
    // one pinned image of the device arena: the inputs are packed into it on the host, moved by one
    // H2D copy, and the results come back by one D2H copy (pageable copies of each piece cost tens of
    // microseconds apiece)
    const size_t job_bytes = (sizeof(rg::GeneralJob) + 15) & ~15ull;
    const size_t aad_off = 0, pay_off = (aad_len + 15) & ~15ull, tag_off = pay_off + ((len + 15) & ~15ull);
    const size_t arena = job_bytes + tag_off + 16;
    RG_HIP(ctx->d_general.reserve(arena, ctx->gen_stream), "alloc arena");
    RG_HIP(ctx->h_general.reserve(arena), "alloc pinned arena");
    uint8_t *d = static_cast<uint8_t *>(ctx->d_general.p);
    uint8_t *h = static_cast<uint8_t *>(ctx->h_general.p);
    rg::GeneralJob job;
    memset(&job, 0, sizeof job);
    memcpy(job.key, key, 32);
    if (xchacha) { // HChaCha20 input nonce[0..16]; ChaCha20-Poly1305 nonce 0^4 || nonce[16..24]
        job.xchacha = 1;
        memcpy(job.hnonce, nonce, 16);
        memcpy(reinterpret_cast<uint8_t *>(job.nonce) + 4, nonce + 16, 8);
    } else {
        memcpy(job.nonce, nonce, 12);
    }
    job.decrypt = dec ? 1 : 0;
    job.aad_off = aad_off;
    job.aad_len = aad_len;
    job.payload_off = pay_off;
    job.payload_len = len;
    job.tag_off = tag_off;
    job.status = RG_PKT_PENDING; // fail closed: only the kernel's verdict accepts
    {
        const hipError_t e = ctx->ev_gen.ensure();
        if (e != hipSuccess) {
            memset(&job, 0, sizeof job);
            return set_err(RG_EDEVICE, "general event", e);
        }
    }
    memcpy(h, &job, sizeof job);
    // from here on the key sits in the pinned image (and, after the H2D copy, in the device arena):
    // wiped on every way out, errors included (the reference zeroizes keys on drop, prim.rs:227-231); the
    // waits are bounded, and a device that never completes keeps its arena (only the host image is wiped)
    struct Wipe {
        uint8_t *h, *d;
        size_t n;
        hipStream_t st;
        hipEvent_t ev;
        uint32_t ms;
        bool settled() { return hipEventRecord(ev, st) == hipSuccess && wait_event(ev, ms, "general wipe") == RG_OK; }
        ~Wipe() {
            const std::string keep = err_text(); // the call's own error stays the one reported
            if (settled()) { // nothing of this call is still reading the job
                (void)hipMemsetAsync(d, 0, n, st);
                (void)settled();
            }
            memset(h, 0, n);
            err_text() = keep;
        }
    } wipe{h, d, job_bytes, ctx->gen_stream, ctx->ev_gen.get(), ctx->wait_ms};
    memset(&job.key, 0, sizeof job.key); // the stack copy
    uint8_t *hb = h + job_bytes; // arena base as the kernel sees it; padding zeroed (pad16)
    memset(hb, 0, tag_off + 16);
    if (aad_len) memcpy(hb + aad_off, aad, aad_len);
    if (len) memcpy(hb + pay_off, payload, len);
    if (dec) memcpy(hb + tag_off, tag, 16);
    hipStream_t st = ctx->gen_stream;
    RG_HIP(hipMemcpyAsync(d, h, arena, hipMemcpyHostToDevice, st), "H2D arena");
    RG_HIP(rg::launch_general(reinterpret_cast<rg::GeneralJob *>(d), 1, d + job_bytes, st), "general launch");
    RG_HIP(hipMemcpyAsync(h, d, arena, hipMemcpyDeviceToHost, st), "D2H arena");
    RG_HIP(hipEventRecord(ctx->ev_gen.get(), st), "general event");
    RG_WAIT(ctx->ev_gen.get(), ctx->wait_ms, "general wait");
    const uint32_t status = reinterpret_cast<const rg::GeneralJob *>(h)->status;
    if (status != RG_PKT_OK && status != RG_PKT_DECRYPT_ERR)
        return set_err(RG_EDEVICE, "aead: the kernel left the message unfinished");
    if (dec && status != RG_PKT_OK) return RG_PKT_DECRYPT_ERR; // payload untouched
    if (len) memcpy(payload, hb + pay_off, len);
    if (!dec) memcpy(tag, hb + tag_off, 16);
    return RG_OK;
}

extern "C" {

int rg_chacha20poly1305_enc(rg_ctx *ctx, const uint8_t key[32], const uint8_t nonce[12], const uint8_t *aad,
                            size_t aad_len, uint8_t *payload, size_t len, uint8_t tag[16]) {
    return general_one(ctx, false, key, nonce, aad, aad_len, payload, len, tag);
}

int rg_chacha20poly1305_dec(rg_ctx *ctx, const uint8_t key[32], const uint8_t nonce[12], const uint8_t *aad,
                            size_t aad_len, uint8_t *payload, size_t len, const uint8_t tag[16]) {
    return general_one(ctx, true, key, nonce, aad, aad_len, payload, len, const_cast<uint8_t *>(tag));
}

int rg_xchacha20poly1305_enc(rg_ctx *ctx, const uint8_t key[32], const uint8_t nonce[24], const uint8_t *aad,
                             size_t aad_len, uint8_t *payload, size_t len, uint8_t tag[16]) {
    return general_one(ctx, false, key, nonce, aad, aad_len, payload, len, tag, true);
}

int rg_xchacha20poly1305_dec(rg_ctx *ctx, const uint8_t key[32], const uint8_t nonce[24], const uint8_t *aad,
                             size_t aad_len, uint8_t *payload, size_t len, const uint8_t tag[16]) {
    return general_one(ctx, true, key, nonce, aad, aad_len, payload, len, const_cast<uint8_t *>(tag), true);
}

} // extern "C"
