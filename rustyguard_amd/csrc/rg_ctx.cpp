// rg_ctx.cpp -- the bottom layer of the C ABI of include/rg_aead.h: the thread's error text, the bounded
// waits, the buffer owners of rg_host.h, the device context with its setters and getters, and the pinned
// memory and NUMA helpers.
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <new>

#include "rg_host.h"

namespace rg {
namespace host {

namespace {
thread_local std::string g_err;
}

std::string &err_text() { return g_err; }

int set_err(int code, const char *what, hipError_t e) {
    char buf[256];
    if (e != hipSuccess)
        snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    else
        snprintf(buf, sizeof buf, "%s", what);
    g_err = buf;
    return code;
}

int wait_event(hipEvent_t e, uint32_t timeout_ms, const char *what) {
    if (!e) return RG_OK;
    bool late = false;
    const hipError_t r =
        wait_bounded([e]() { return completions_lost() ? hipErrorNotReady : hipEventQuery(e); }, timeout_ms, &late);
    if (late) {
        char buf[160];
        snprintf(buf, sizeof buf, "%s: timed out after %u ms (the device never reported the completion)", what,
                 timeout_ms);
        return set_err(RG_EDEVICE, buf);
    }
    if (r != hipSuccess) return set_err(RG_EDEVICE, what, r);
    return RG_OK;
}

bool capturing(hipStream_t s) {
    hipStreamCaptureStatus c = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &c) == hipSuccess && c != hipStreamCaptureStatusNone;
}

int fail_closed(int rc, uint8_t *status, size_t n) {
    if (rc < 0 && status) memset(status, RG_PKT_PENDING, n);
    return rc;
}

int check_workspace(const char *what, const void *table, const void *workspace, size_t workspace_len, uint64_t total) {
    char buf[160];
    if (((uintptr_t)table & 7u) || ((uintptr_t)workspace & 15u)) {
        snprintf(buf, sizeof buf, "%s: the table must be 8-byte and the workspace 16-byte aligned", what);
        return set_err(RG_EINVAL, buf);
    }
    if (total == 0 || workspace_len < total) {
        snprintf(buf, sizeof buf, "%s: workspace smaller than its workspace_size call asks for", what);
        return set_err(RG_EINVAL, buf);
    }
    return RG_OK;
}

// --------------------------------------------------------------- SecretBuf
SecretBuf::~SecretBuf() {
    if (p || !retired.empty()) {
        (void)release(nullptr);
        (void)hipStreamSynchronize(nullptr);
    }
    forget_users();
}

void SecretBuf::forget_users() {
    for (auto &u : users) (void)hipEventDestroy(u.second);
    users.clear();
}

hipError_t SecretBuf::use(hipStream_t s) {
    if (!p) return hipSuccess;
    if (capturing(s)) {
        captured = true;
        return hipSuccess;
    }
    for (auto &u : users)
        if (u.first == s) return hipEventRecord(u.second, s);
    // streams whose last recorded use has completed need no fence: dropped, so that a caller making a
    // new stream per call does not grow the list
    for (size_t k = 0; k < users.size();) {
        if (hipEventQuery(users[k].second) == hipSuccess) {
            (void)hipEventDestroy(users[k].second);
            users[k] = users.back();
            users.pop_back();
        } else {
            ++k;
        }
    }
    hipEvent_t e = nullptr;
    hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (r != hipSuccess) return r;
    users.emplace_back(s, e);
    return hipEventRecord(e, s);
}

hipError_t SecretBuf::wipe_free(void *blk, size_t n, hipStream_t s) {
    hipError_t r = hipSuccess;
    for (auto &u : users)
        if (r == hipSuccess) r = hipStreamWaitEvent(s, u.second, 0);
    if (r == hipSuccess) r = hipMemsetAsync(blk, 0, n, s);
    // a failed wait or wipe must not hand the keys back to the allocator: keep the block (freed by
    // a later release, or leaked rather than disclosed)
    if (r != hipSuccess) return r;
    wipe_probe(blk, n, s);
    return hipFreeAsync(blk, s);
}

hipError_t SecretBuf::release_current(hipStream_t s) {
    if (!p) return hipSuccess;
    hipError_t r = wipe_free(p, cap, s);
    if (r != hipSuccess) return r;
    p = nullptr;
    cap = 0;
    captured = false;
    if (retired.empty()) forget_users();
    return r;
}

hipError_t SecretBuf::release(hipStream_t s) {
    hipError_t r = hipSuccess;
    while (r == hipSuccess && !retired.empty()) {
        r = wipe_free(retired.back().first, retired.back().second, s);
        if (r == hipSuccess) retired.pop_back();
    }
    if (r == hipSuccess) r = release_current(s);
    if (r == hipSuccess) forget_users();
    return r;
}

hipError_t SecretBuf::reserve(size_t bytes, hipStream_t s) {
    if (bytes <= cap) return hipSuccess;
    if (capturing(s)) return hipErrorStreamCaptureUnsupported;
    if (captured) { // a graph reads this block: it stays until release()
        retired.emplace_back(p, cap);
        p = nullptr;
        cap = 0;
        captured = false;
    } else {
        hipError_t r = release_current(s);
        if (r != hipSuccess) return r;
    }
    if (injected_failure()) return hipErrorOutOfMemory;
    const size_t want = std::max<size_t>(bytes, 4096);
    hipError_t r = hipMallocAsync(&p, want, s);
    if (r == hipSuccess) cap = want;
    else p = nullptr;
    return r;
}

// ----------------------------------------------------------------- context
int check_ctx(rg_ctx *ctx) {
    if (!ctx) return set_err(RG_EINVAL, "null context");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return set_err(RG_EDEVICE, "hipSetDevice", e);
    return RG_OK;
}

int claim_stream(rg_ctx *ctx, hipStream_t st) {
    if (!ctx->dev_busy || ctx->dev_stream == st || capturing(st)) return RG_OK;
    const hipError_t q = hipEventQuery(ctx->dev_ev.get());
    if (q == hipSuccess) return RG_OK;
    if (q == hipErrorNotReady)
        return set_err(RG_EINVAL, "context busy: its last batch is still in flight on another stream (one context "
                                  "per concurrent stream; nothing enqueued)");
    return set_err(RG_EDEVICE, "context stream check", q);
}

// The event that marks a device batch's end: recorded by the transport kernel's own dispatch (RG_LAUNCH,
// no separate queue packet), or nullptr inside a stream capture (a graph is its owner's to order,
// include/rg_aead.h).  It is only queried, never used to read what the batch wrote: no system-scope fence
// (with one, the release wrote the L2s back after the kernel: +7 us on an eager config-2 seal; a separate
// fence-free hipEventRecord still cost +3 us, round 6).
hipEvent_t stream_event(rg_ctx *ctx, hipStream_t st) {
#if RG_NO_STREAM_MARK // diagnostic builds only (the A/B of the mark's cost)
    return nullptr;
#endif
    if (capturing(st)) return nullptr;
    (void)ctx->dev_ev.ensure(hipEventDisableTiming | hipEventDisableSystemFence);
    return ctx->dev_ev.get();
}

void mark_stream(rg_ctx *ctx, hipStream_t st) {
    ctx->dev_stream = st;
    ctx->dev_busy = true;
}

namespace {

// The host NUMA node closest to a GPU, -1 if unknown.  HIP's attribute first; this runtime answers it with
// hipErrorInvalidValue (round 6 box), and a failed query stays the thread's last error, which the next
// launch's hipGetLastError (and PyTorch's checks) then report -- so it is cleared, and the node is read
// from the device's PCI function in sysfs instead.
int gpu_numa_node(int device) {
    int node = -1;
    if (hipDeviceGetAttribute(&node, hipDeviceAttributeHostNumaId, device) == hipSuccess && node >= 0) return node;
    (void)hipGetLastError();
    char bus[32] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    for (char *p = bus; *p; ++p) *p = (char)((*p >= 'A' && *p <= 'F') ? *p - 'A' + 'a' : *p); // sysfs: lower case
    const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/numa_node";
    FILE *f = std::fopen(path.c_str(), "r");
    if (!f) return -1;
    if (std::fscanf(f, "%d", &node) != 1) node = -1;
    std::fclose(f);
    return node >= 0 ? node : -1;
}

} // namespace
} // namespace host
} // namespace rg

using namespace rg::host;
using rg::DeviceGuard;

extern "C" {

int rg_abi_version(void) { return RG_ABI_VERSION; }

const char *rg_last_error(void) { return err_text().c_str(); }

int rg_create(int device, rg_ctx **out) {
    if (!out) return set_err(RG_EINVAL, "null out");
    *out = nullptr;
    // Agent-scope completion signals: the round-5 host pipeline hung under them at 16 MiB slices while 8 MiB
    // completed (profiles/r5_e2e_rtenv.txt).  The reading that fits both: a wait spins on the signal for a
    // short active-wait window, then sleeps until the signal's interrupt; a slice that finishes inside the
    // window (8 MiB) is seen by the spin, a longer one (16 MiB) leaves the host asleep on an interrupt that
    // an agent-scope signal never raises.  Waits are bounded now, but the setting would turn every slice
    // past the window into a timeout: refused.
    {
        const char *v = getenv("ROC_SYSTEM_SCOPE_SIGNAL");
        if (v && v[0] == '0' && v[1] == '\0')
            return set_err(RG_EINVAL, "ROC_SYSTEM_SCOPE_SIGNAL=0 (agent-scope signals) hangs host waits; unset it");
    }
    int ndev = 0;
    RG_HIP(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
    if (device < 0 || device >= ndev) return set_err(RG_EINVAL, "no such HIP device");
    DeviceGuard dg_;
    RG_HIP(hipSetDevice(device), "hipSetDevice");
    rg_ctx *c = new (std::nothrow) rg_ctx();
    if (!c) return set_err(RG_ENOMEM, "alloc ctx");
    c->device = device;
    c->h_general.secret = true;
    {
        hipError_t e = hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, device);
        if (e == hipSuccess) c->numa_node = gpu_numa_node(device);
        if (e == hipSuccess) e = rg::prepare_tile_kernels();
        if (e == hipSuccess) e = rg::prepare_pipe_kernels(c->pipe_max_wg);
        if (e == hipSuccess) e = rg::prepare_flat_kernels();
        // the flattened kernel's store sink, allocated now: the automatic choice may first pick that
        // kernel inside a stream capture (HIP graph), where allocation is not permitted
        if (e == hipSuccess) e = c->d_junk.reserve(rg::flat_junk_bytes(c->cus));
        if (e == hipSuccess) e = c->plan_dev.ensure_ctl();
        for (auto &sl : c->slots)
            if (e == hipSuccess) e = sl.plan.ensure_ctl();
        if (e != hipSuccess) {
            rg_destroy(c); // every buffer allocated so far goes back (the owners' destructors)
            return set_err(RG_EDEVICE, "kernel setup", e);
        }
    }
    {
        hipError_t e = hipSuccess;
        for (hipStream_t *sp : {&c->hs_in, &c->hs_run, &c->hs_out, &c->gen_stream})
            if (e == hipSuccess) e = hipStreamCreateWithFlags(sp, hipStreamNonBlocking);
        for (auto &s : c->slots)
            for (Event *ep : {&s.ev_in, &s.ev_run, &s.ev_out})
                if (e == hipSuccess) e = ep->ensure();
        if (e != hipSuccess) {
            rg_destroy(c);
            return set_err(RG_EDEVICE, "hipStreamCreate", e);
        }
    }
    // the pools zeroed above (null-stream memsets) are zero before any launch on any of the caller's streams
    {
        const hipError_t e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) {
            rg_destroy(c);
            return set_err(RG_EDEVICE, "context setup", e);
        }
    }
    *out = c;
    return RG_OK;
}

// Only what has an order is spelled out; every buffer and event goes with its owner's destructor, while the
// context's device is still selected.
void rg_destroy(rg_ctx *ctx) {
    if (!ctx) return;
    DeviceGuard dg_;
    (void)hipSetDevice(ctx->device);
    for (hipStream_t sp : {ctx->hs_in, ctx->hs_run, ctx->hs_out, ctx->gen_stream})
        if (sp) (void)hipStreamSynchronize(sp);
    // key material: wiped behind its last readers, on the context's own stream
    hipStream_t ws = ctx->gen_stream; // null while rg_create has not made it (the legacy stream then)
    (void)ctx->d_keys.release(ws);
    (void)ctx->d_general.release(ws);
    (void)ctx->d_mac_keys.release(ws);
    (void)hipStreamSynchronize(ws);
    for (hipStream_t sp : {ctx->hs_in, ctx->hs_run, ctx->hs_out, ctx->gen_stream})
        if (sp) (void)hipStreamDestroy(sp);
    delete ctx;
}

int rg_set_lanes_per_packet(rg_ctx *ctx, int lanes) {
    if (!ctx) return set_err(RG_EINVAL, "null context");
    if (lanes != 0 && lanes != 1 && lanes != 2 && lanes != 4) return set_err(RG_EINVAL, "lanes must be 0,1,2,4");
    ctx->lanes = lanes;
    return RG_OK;
}

int rg_get_lanes_per_packet(rg_ctx *ctx, size_t n) {
    if (!ctx) return set_err(RG_EINVAL, "null context");
    if (ctx->lanes) return ctx->lanes;
    // fewest lanes per packet that still gives every SIMD one wave (n * K
    // lanes >= CUs * 256): a single wave of the pipelined kernel already keeps
    // a SIMD's VALU busy, so more segments only add combine work
    const size_t want = (size_t)(ctx->cus > 0 ? ctx->cus : 256) * 256;
    if (n >= want) return 1;
    if (2 * n >= want) return 2;
    return 4;
}

int rg_set_wg_per_cu(rg_ctx *ctx, int wg) {
    if (!ctx) return set_err(RG_EINVAL, "null context");
    if (wg < -1 || wg > 8) return set_err(RG_EINVAL, "wg_per_cu must be -1..8");
    ctx->wg_per_cu = wg;
    return RG_OK;
}

int rg_set_host_slice(rg_ctx *ctx, size_t bytes) {
    if (!ctx) return set_err(RG_EINVAL, "null context");
    if (bytes < (64u << 10) || bytes > (1ull << 30)) return set_err(RG_EINVAL, "host slice must be 64 KiB .. 1 GiB");
    ctx->host_slice = bytes;
    return RG_OK;
}

int rg_set_wait_timeout(rg_ctx *ctx, uint32_t ms) {
    if (!ctx) return set_err(RG_EINVAL, "null context");
    if (ms < 1 || ms > 3600000u) return set_err(RG_EINVAL, "wait timeout must be 1 .. 3600000 ms");
    ctx->wait_ms = ms;
    return RG_OK;
}

int rg_set_staged(rg_ctx *ctx, int g) {
    if (!ctx) return set_err(RG_EINVAL, "null context");
    if (g < -1 || g > 3)
        return set_err(RG_EINVAL, "kernel must be -1 (auto), 0 (pipelined lanes), 1/2 (tile windows) or 3 (flat)");
    ctx->staged_g = g;
    return RG_OK;
}

int rg_set_plan(rg_ctx *ctx, int on) {
    if (!ctx) return set_err(RG_EINVAL, "null context");
    if (on < 0 || on > 2) return set_err(RG_EINVAL, "plan must be 0 (off), 1 (on) or 2 (auto)");
    ctx->plan = on;
    return RG_OK;
}

int rg_set_segments(rg_ctx *ctx, int k) {
    if (!ctx) return set_err(RG_EINVAL, "null context");
    if (k != 0 && k != 1 && k != 2 && k != 4) return set_err(RG_EINVAL, "segments must be 0, 1, 2 or 4");
    ctx->segments = k;
    return RG_OK;
}

// Diagnostics exist only in diagnostic builds (-DRG_DIAG, tools/build_variant.sh): the product library
// accepts mode 0 and a null stamp buffer and refuses everything else, so no context of it can emit
// frames that are not sealed (the seal contract, prim.rs:179-188, always encrypts).
int rg_set_debug_buffer(rg_ctx *ctx, void *dev_ptr) {
    if (!ctx) return set_err(RG_EINVAL, "null context");
#if RG_DIAG
    ctx->dbg = static_cast<uint64_t *>(dev_ptr);
#else
    if (dev_ptr) return set_err(RG_EINVAL, "stamp buffers exist only in diagnostic builds (RG_DIAG)");
#endif
    return RG_OK;
}

int rg_set_debug_mode(rg_ctx *ctx, int mode) {
    if (!ctx) return set_err(RG_EINVAL, "null context");
#if RG_DIAG
    if (mode < 0 || mode > 8) return set_err(RG_EINVAL, "debug mode must be 0..8");
#else
    if (mode != 0) return set_err(RG_EINVAL, "debug modes exist only in diagnostic builds (RG_DIAG)");
#endif
    ctx->debug_mode = mode;
    return RG_OK;
}

// Kernel choice: batches that fill at most about one wave per SIMD go to the
// pipelined lane kernel (it saturates a SIMD with one wave and, with the
// planner, balances mixed sizes); larger batches go to the LDS-staged tile
// kernel, whose coalesced LDS-DMA windows win once two waves per SIMD are
// resident (measured).
int rg_get_kernel(rg_ctx *ctx, size_t n) {
    if (!ctx) return set_err(RG_EINVAL, "null context");
    if (ctx->staged_g >= 0) return ctx->staged_g;
    return n < (size_t)(ctx->cus > 0 ? ctx->cus : 256) * 512 ? 0 : 2;
}

int rg_last_kernel(rg_ctx *ctx) {
    if (!ctx) return set_err(RG_EINVAL, "null context");
    return ctx->last_kernel;
}

void *rg_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void rg_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}

int rg_numa_node(rg_ctx *ctx) {
    if (!ctx) return set_err(RG_EINVAL, "null context");
    return ctx->numa_node;
}

int rg_numa_bind(void *p, size_t bytes, int node) {
    if (!p || !bytes || node < 0 || node >= 1024) return set_err(RG_EINVAL, "numa_bind: bad args");
#ifdef SYS_mbind
    const uintptr_t pg = (uintptr_t)sysconf(_SC_PAGESIZE);
    const uintptr_t a = (uintptr_t)p & ~(pg - 1), b = ((uintptr_t)p + bytes + pg - 1) & ~(pg - 1);
    unsigned long mask[16] = {0};
    mask[node / 64] = 1ul << (node % 64);
    // MPOL_BIND, MPOL_MF_MOVE: pages already touched move to the node (pinned pages cannot: bind first)
    if (syscall(SYS_mbind, a, b - a, 2 /* MPOL_BIND */, mask, 1024ul, 2u /* MPOL_MF_MOVE */) != 0) {
        char what[96];
        snprintf(what, sizeof what, "numa_bind: mbind to node %d failed (errno %d)", node, errno);
        return set_err(RG_EINVAL, what);
    }
    return RG_OK;
#else
    return set_err(RG_EINVAL, "numa_bind: no mbind on this platform");
#endif
}

int rg_host_register(void *p, size_t bytes) {
    if (!p || !bytes) return set_err(RG_EINVAL, "host_register: bad args");
    RG_HIP(hipHostRegister(p, bytes, hipHostRegisterDefault), "hipHostRegister");
    return RG_OK;
}

int rg_host_unregister(void *p) {
    if (!p) return set_err(RG_EINVAL, "host_unregister: null");
    RG_HIP(hipHostUnregister(p), "hipHostUnregister");
    return RG_OK;
}

} // extern "C"
