// rg_debug.cpp -- the test hooks of include/rg_aead_test.h and the four functions through which the other
// host units read them (rg_host.h, "test hooks").  With -DRG_TEST_HOOKS (librg_aead_test.so only) the hooks'
// state and the rg_debug_* calls are here; without it (the product library) the four functions are the
// constants below and nothing else is compiled.
#include "rg_host.h"

#if RG_TEST_HOOKS
#include <algorithm>
#include <atomic>

#include "../../include/rg_aead_test.h"

using namespace rg::host;

namespace {
std::atomic<int> g_fail_reserve{0};    // rg_debug_fail_reserve: the n-th following allocation fails
std::atomic<uint32_t> g_stale_done{0}; // rg_debug_plan_handoff: the counts the preset pass starts from (0: none)
std::atomic<uint32_t> g_stale_pool{0};
std::atomic<int> g_lose_completions{0}; // rg_debug_lose_completions
// the first bytes of the most recently wiped block, read back after its wipe (rg_debug_last_wipe)
std::mutex g_wipe_mu;
uint8_t *g_wipe_probe = nullptr; // pinned, 4 KiB, never freed
size_t g_wipe_bytes = 0;
uint64_t g_wipes = 0;
} // namespace

bool rg::host::injected_failure() {
    int v = g_fail_reserve.load();
    while (v > 0)
        if (g_fail_reserve.compare_exchange_weak(v, v - 1)) return v == 1;
    return false;
}

bool rg::host::completions_lost() { return g_lose_completions.load() != 0; }

void rg::host::stale_preset(uint32_t *done0, uint32_t *pool0) {
    *done0 = g_stale_done.load();
    *pool0 = g_stale_pool.load();
}

void rg::host::wipe_probe(void *blk, size_t n, hipStream_t s) {
    std::lock_guard<std::mutex> g(g_wipe_mu);
    if (!g_wipe_probe) (void)hipHostMalloc(reinterpret_cast<void **>(&g_wipe_probe), 4096, hipHostMallocDefault);
    g_wipe_bytes = std::min<size_t>(n, 4096);
    if (g_wipe_probe) (void)hipMemcpyAsync(g_wipe_probe, blk, g_wipe_bytes, hipMemcpyDeviceToHost, s);
    (void)hipStreamSynchronize(s);
    ++g_wipes;
}

static const SecretBuf *secret_of(rg_ctx *ctx, int which) {
    return which == 0 ? &ctx->d_general : which == 1 ? &ctx->d_keys : which == 2 ? &ctx->d_mac_keys : nullptr;
}

extern "C" {

int rg_debug_read_arena(rg_ctx *ctx, int which, void *dst, size_t bytes) {
    rg::DeviceGuard dg_;
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if (!dst) return set_err(RG_EINVAL, "debug_read_arena: null dst");
    const SecretBuf *b = secret_of(ctx, which);
    if (!b) return set_err(RG_EINVAL, "debug_read_arena: which must be 0, 1 or 2");
    std::lock_guard<std::mutex> g(ctx->mu);
    RG_HIP(hipDeviceSynchronize(), "debug_read_arena sync"); // test hook: the buffer's writers are done
    const size_t m = std::min(bytes, b->cap);
    if (m) RG_HIP(hipMemcpy(dst, b->p, m, hipMemcpyDeviceToHost), "debug_read_arena copy");
    return (int)std::min<size_t>(m, 0x7FFFFFFF);
}

void rg_debug_fail_reserve(int nth) { g_fail_reserve.store(nth > 0 ? nth : 0); }

void rg_debug_plan_handoff(int mode) {
    g_stale_done.store(mode == 1 ? 0x40000000u : 0u);
    g_stale_pool.store(mode == 2 ? 0x40000000u : 0u);
}

void rg_debug_lose_completions(int on) { g_lose_completions.store(on ? 1 : 0); }

int rg_debug_wait_selftest(uint32_t timeout_ms, uint32_t ready_after, uint32_t *polls_out, uint32_t *elapsed_ms_out) {
    uint32_t polls = 0;
    bool late = false;
    const auto t0 = std::chrono::steady_clock::now();
    const hipError_t r = wait_bounded(
        [&]() { return ++polls > ready_after ? hipSuccess : hipErrorNotReady; }, timeout_ms, &late);
    const auto el = std::chrono::steady_clock::now() - t0;
    if (polls_out) *polls_out = polls;
    if (elapsed_ms_out) *elapsed_ms_out = (uint32_t)std::chrono::duration_cast<std::chrono::milliseconds>(el).count();
    if (late) return set_err(RG_EDEVICE, "wait selftest: timed out");
    return r == hipSuccess ? RG_OK : set_err(RG_EDEVICE, "wait selftest: error");
}

int64_t rg_debug_last_wipe(void *dst, size_t bytes, uint64_t *wipes_out) {
    std::lock_guard<std::mutex> g(g_wipe_mu);
    if (wipes_out) *wipes_out = g_wipes;
    if (!g_wipe_probe || !dst) return 0;
    const size_t m = std::min(bytes, g_wipe_bytes);
    memcpy(dst, g_wipe_probe, m);
    return (int64_t)m;
}

int rg_debug_secret_state(rg_ctx *ctx, int which, uint32_t *retired_out, uint32_t *users_out) {
    if (!ctx) return set_err(RG_EINVAL, "null context");
    const SecretBuf *b = secret_of(ctx, which);
    if (!b) return set_err(RG_EINVAL, "debug_secret_state: which must be 0, 1 or 2");
    if (retired_out) *retired_out = (uint32_t)b->retired.size();
    if (users_out) *users_out = (uint32_t)b->users.size();
    return b->captured ? 1 : 0;
}

} // extern "C"

#else // the product library: no hook exists

bool rg::host::injected_failure() { return false; }
bool rg::host::completions_lost() { return false; }
void rg::host::stale_preset(uint32_t *, uint32_t *) {}
void rg::host::wipe_probe(void *, size_t, hipStream_t) {}

#endif
