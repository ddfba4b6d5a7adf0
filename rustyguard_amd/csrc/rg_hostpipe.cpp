// rg_hostpipe.cpp -- the host-frame calls of include/rg_aead.h: the three-slot H2D -> kernel -> D2H slice
// pipeline of one context, a group's runs (one NUMA-placed worker thread per context), the splitter and
// every *_multi call.
#include <sched.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <new>

#include "rg_host.h"

using namespace rg::host;
using rg::DeviceGuard;

namespace {

constexpr size_t kSlicePkts = 1u << 16;
constexpr uint64_t kOutOfRange = (UINT64_MAX / 2) & ~15ull;

bool in_arena(const rg_pkt_desc &d, bool open, size_t buf_len) {
    const uint64_t need = (uint64_t)d.len + (open ? 0 : 32);
    return d.offset <= buf_len && need <= buf_len - d.offset && d.len <= rg::kMaxPayload + 32;
}

// The key table of a host call, on the upload stream ahead of the slices' frames (a slice's kernel
// waits for its frames' upload, so for the keys too).  Every host call drains its slices before it
// returns (run_host), so no kernel still reads the old table when a regrow wipes it.
int upload_keys(rg_ctx *ctx, const uint8_t *keys, const uint32_t *receivers, uint32_t nkeys) {
    RG_HIP(ctx->d_keys.reserve((size_t)nkeys * 32, ctx->hs_in), "alloc keys");
    RG_HIP(hipMemcpyAsync(ctx->d_keys.p, keys, (size_t)nkeys * 32, hipMemcpyHostToDevice, ctx->hs_in), "H2D keys");
    if (receivers) {
        RG_HIP(ctx->d_recv.reserve((size_t)nkeys * 4), "alloc receivers");
        RG_HIP(hipMemcpy(ctx->d_recv.p, receivers, (size_t)nkeys * 4, hipMemcpyHostToDevice), "H2D receivers");
    }
    return RG_OK;
}

// Drain a finished slice: copy statuses / counters back to the caller.  A status still RG_PKT_PENDING
// after the slice completed is a packet no kernel finished: the call fails (include/rg_aead.h).
int finish_slot(Slot &s, uint32_t wait_ms, uint8_t *status, uint64_t *counters_out) {
    if (!s.busy) return RG_OK;
    RG_WAIT(s.ev_out.get(), wait_ms, "slice wait");
    if (s.orphan) {
        s.busy = s.orphan = false;
        return RG_OK;
    }
    const size_t m = s.i1 - s.i0;
    if (status) memcpy(status + s.i0, s.h_status.p, m);
    if (counters_out) memcpy(counters_out + s.i0, s.h_ctr_out.p, m * 8);
    s.busy = false;
    if (m && memchr(s.h_status.p, RG_PKT_PENDING, m)) {
        char what[128];
        snprintf(what, sizeof what, "slice [%zu, %zu): the kernel left packets unfinished (RG_PKT_PENDING)", s.i0,
                 s.i1);
        return set_err(RG_EDEVICE, what);
    }
    return RG_OK;
}

// Shared driver of the host entry points: packets [i, end) of the caller's arrays through one
// context's three-slot H2D -> kernel -> D2H pipeline, one slice per step().  A group (rg_group)
// drives one run per context (run_host_group).
struct HostRun {
    rg_ctx *ctx;
    bool open;
    uint32_t nkeys;
    const rg_pkt_desc *desc;
    const uint64_t *counters;
    size_t i, end;
    uint8_t *buf;
    size_t buf_len;
    uint8_t *status;
    uint64_t *counters_out;
    bool with_receivers;
    int which = 0;

    bool done() const { return i >= end; }
    // the slot the next step() reuses holds no slice in flight (or its download has completed): step()
    // will not block (hipEventQuery, no wait)
    bool ready() const {
        const Slot &s = ctx->slots[which];
        return !s.busy || hipEventQuery(s.ev_out.get()) == hipSuccess;
    }
    int step(uint64_t ticket = 0); // enqueue the next slice (after draining the slot it reuses)
    // every slot's slice back (the first error is the result; the other slots still drain)
    int drain() {
        int rc = RG_OK;
        for (auto &s : ctx->slots) {
            const int r = finish_slot(s, ctx->wait_ms, status, open ? counters_out : nullptr);
            if (rc == RG_OK) rc = r;
        }
        return rc;
    }
};

int HostRun::step(uint64_t ticket) {
    RG_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    // slice [i, j): bounded by packet count and by the byte span of its frames
    size_t j = i;
    uint64_t lo = UINT64_MAX, hi = 0;
    const size_t slice_bytes = ctx->host_slice;
    while (j < end && j - i < kSlicePkts) {
        const rg_pkt_desc &d = desc[j];
        if (in_arena(d, open, buf_len)) {
            const uint64_t e = d.offset + (uint64_t)d.len + (open ? 0 : 32);
            const uint64_t nlo = std::min<uint64_t>(lo, d.offset & ~15ull), nhi = std::max<uint64_t>(hi, e);
            if (j > i && nhi - nlo > slice_bytes) break;
            lo = nlo;
            hi = nhi;
        }
        ++j;
    }
    if (lo == UINT64_MAX) lo = hi = 0; // nothing in range: only statuses come back
    Slot &s = ctx->slots[which];
    int rc = finish_slot(s, ctx->wait_ms, status, counters_out);
    if (rc) return rc;
    const size_t m = j - i;
    const size_t span = hi - lo;
    RG_HIP(s.d_buf.reserve(span + 16), "alloc slice");
    RG_HIP(s.h_desc.reserve_mapped(m * sizeof(rg_pkt_desc)), "alloc h_desc");
    RG_HIP(s.h_status.reserve_mapped(m), "alloc h_status");
    // the slice's statuses start pending in host memory, whichever kernel runs (the previous slice's
    // verdicts must not stand for a packet the kernel never reaches)
    memset(s.h_status.p, RG_PKT_PENDING, m);
    rg_pkt_desc *hd = static_cast<rg_pkt_desc *>(s.h_desc.p);
    for (size_t k = 0; k < m; ++k) {
        hd[k] = desc[i + k];
        // frames outside the arena get an aligned out-of-range offset: the kernel flags them INVALID
        hd[k].offset = in_arena(desc[i + k], open, buf_len) ? desc[i + k].offset - lo : kOutOfRange;
    }
    if (!open) {
        RG_HIP(s.h_ctr.reserve_mapped(m * 8), "alloc h_ctr");
        memcpy(s.h_ctr.p, counters + i, m * 8);
    } else {
        RG_HIP(s.h_ctr_out.reserve_mapped(m * 8), "alloc h_ctr_out");
    }
    // the frames' upload on hs_in (after the previous use of this slot's buffers has been downloaded: the
    // host waited for ev_out above, so nothing of it is still in flight); descriptors, counters and
    // statuses stay in mapped host memory, which the kernel reads and writes over the link in place of
    // three small copies per slice (round 4, profiles/r4_e2e_mapped_ab.txt)
    hipStream_t sin = ctx->hs_in, srun = ctx->hs_run, sout = ctx->hs_out;
    if (span) RG_HIP(hipMemcpyAsync(s.d_buf.p, buf + lo, span, hipMemcpyHostToDevice, sin), "H2D frames");
    RG_HIP(hipEventRecord(s.ev_in.get(), sin), "slice event");
    // the kernel on hs_run, once the inputs are in
    RG_HIP(hipStreamWaitEvent(srun, s.ev_in.get(), 0), "slice wait");
    rg::SealArgs sa{};
    rg::OpenArgs oa{};
    auto shared = [&](auto &a) {
        a.keys = static_cast<const uint32_t *>(ctx->d_keys.p);
        a.desc = static_cast<const rg_pkt_desc *>(s.h_desc.d);
        a.buf = static_cast<uint8_t *>(s.d_buf.p);
        a.buf_len = span;
        a.status = static_cast<uint8_t *>(s.h_status.d);
        a.nkeys = nkeys;
        a.n = (uint32_t)m;
    };
    if (!open) {
        shared(sa);
        sa.receivers = with_receivers ? static_cast<const uint32_t *>(ctx->d_recv.p) : nullptr;
        sa.counters = static_cast<const uint64_t *>(s.h_ctr.d);
    } else {
        shared(oa);
        oa.counters_out = static_cast<uint64_t *>(s.h_ctr_out.d);
    }
    RG_HIP(launch_any(ctx, open ? nullptr : &sa, open ? &oa : nullptr, s.plan, srun), open ? "open launch" : "seal launch");
    RG_HIP(hipEventRecord(s.ev_run.get(), srun), "slice event");
    // downloads on hs_out, once the kernel is done
    RG_HIP(hipStreamWaitEvent(sout, s.ev_run.get(), 0), "slice wait");
    if (span) RG_HIP(hipMemcpyAsync(buf + lo, s.d_buf.p, span, hipMemcpyDeviceToHost, sout), "D2H frames");
    RG_HIP(hipEventRecord(s.ev_out.get(), sout), "slice event");
    s.i0 = i;
    s.i1 = j;
    s.ticket = ticket;
    s.busy = true;
    i = j;
    which = (which + 1) % rg_ctx::kHostSlots;
    return RG_OK;
}

// Runs to completion from one thread (one context, or several when a group cannot start a thread per
// context, or in builds with RG_GROUP_THREADS=0).  A run is stepped
// when the slot its next slice reuses is free, so that no context waits while another's download is in
// flight (round 4 stepped round-robin and blocked in each step on the slot it reused: VERDICT r4 item 5);
// only when every unfinished run's next slot is still busy does the thread block, on the slice issued
// first of all (the oldest download).  On an error every run still drains what it has in flight (its
// slots are reused by the next call).
int run_host(HostRun *runs, size_t nruns) {
    int rc = RG_OK;
    uint64_t ticket = 0;
    while (rc == RG_OK) {
        bool more = false, moved = false;
        for (HostRun *rp = runs; rp != runs + nruns; ++rp) {
            HostRun &r = *rp;
            if (r.done()) continue;
            more = true;
            if (!r.ready()) continue;
            rc = r.step(++ticket);
            if (rc) break;
            moved = true;
        }
        if (!more || rc != RG_OK) break;
        if (!moved) {
            Slot *oldest = nullptr;
            uint32_t wait_ms = kDefaultWaitMs;
            for (HostRun *rp = runs; rp != runs + nruns; ++rp) {
                HostRun &r = *rp;
                if (r.done()) continue;
                Slot &s = r.ctx->slots[r.which];
                if (s.busy && (!oldest || s.ticket < oldest->ticket)) {
                    oldest = &s;
                    wait_ms = r.ctx->wait_ms;
                }
            }
            if (oldest) rc = wait_event(oldest->ev_out.get(), wait_ms, "slice wait");
        }
    }
    for (HostRun *rp = runs; rp != runs + nruns; ++rp) {
        (void)hipSetDevice(rp->ctx->device);
        const int rc2 = rp->drain();
        if (rc == RG_OK) rc = rc2;
        for (auto &s : rp->ctx->slots) // still in flight after a failed wait: no longer this call's
            if (s.busy) s.orphan = true;
    }
    return rc;
}

// A group's runs, one worker thread per context (round 5).  From one thread, each slice costs ~50 us of
// HIP API calls: two copies, a launch, three event records and two stream waits
// (profiles/r5_e2e_chain.txt). At 8 MiB slices and ~45 GB/s per link, that feeds about four links.
// With a thread per context, the calls of different devices overlap, and each thread waits only for its
// own device. The caller's thread starts the workers and joins them. If a thread cannot be started, the
// caller's thread runs the remaining runs itself. The first failing run's error becomes the call's
// (rg_last_error is per thread).
// NUMA placement of a group's worker thread: on a two-socket host half the GPUs hang
// off the other socket, and a worker that drives a GPU from there crosses the socket link for every API
// call and for the slot buffers it touches.  The worker is pinned to the CPUs of its GPU's node that this
// process may use (none allowed there: left as it is), and its memory policy prefers that node, so the
// slice buffers it allocates and first-touches land there.  The caller's frames are the caller's: see
// rg_numa_bind / rg_host_register (include/rg_aead.h).
bool node_cpus(int node, cpu_set_t *out) {
    char path[96];
    snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    FILE *f = fopen(path, "r");
    if (!f) return false;
    char line[4096];
    const bool got = fgets(line, sizeof line, f) != nullptr;
    fclose(f);
    if (!got) return false;
    CPU_ZERO(out);
    for (char *p = line; *p && *p != '\n';) { // "0-15,128-143"
        char *end = nullptr;
        const long a = strtol(p, &end, 10);
        if (end == p) break;
        long b = a;
        if (*end == '-') {
            p = end + 1;
            b = strtol(p, &end, 10);
        }
        for (long c = a; c <= b && c < CPU_SETSIZE; ++c) CPU_SET((int)c, out);
        p = *end == ',' ? end + 1 : end;
    }
    return true;
}

int place_thread(int node) {
    if (node < 0) return -1;
    cpu_set_t want, allowed;
    if (!node_cpus(node, &want) || sched_getaffinity(0, sizeof allowed, &allowed) != 0) return -1;
    CPU_AND(&want, &want, &allowed);
    if (CPU_COUNT(&want) == 0) return -1; // none of the node's CPUs is ours
    if (sched_setaffinity(0, sizeof want, &want) != 0) return -1;
#ifdef SYS_set_mempolicy
    unsigned long mask[16] = {0};
    if (node < 1024) {
        mask[node / 64] = 1ul << (node % 64);
        (void)syscall(SYS_set_mempolicy, 1 /* MPOL_PREFERRED */, mask, 1024ul);
    }
#endif
    return CPU_COUNT(&want);
}

#ifndef RG_GROUP_THREADS
#define RG_GROUP_THREADS 1
#endif
int run_host_group(std::vector<HostRun> &runs) {
    if (!RG_GROUP_THREADS || runs.size() < 2) return run_host(runs.data(), runs.size());
    // Threads pay off once a context has a few slices to pipeline; a small batch (every part within two
    // slices) runs from the calling thread, without starting and joining a thread per context.
    bool big = false;
    for (const HostRun &r : runs) {
        uint64_t bytes = 0;
        for (size_t k = r.i; k < r.end && !big; ++k) {
            bytes += (uint64_t)r.desc[k].len + 32;
            big = bytes > 2 * (uint64_t)r.ctx->host_slice;
        }
        if (big) break;
    }
    if (!big) return run_host(runs.data(), runs.size());
    const size_t n = runs.size();
    std::vector<int> rcs;
    std::vector<std::string> errs;
    std::vector<std::thread> workers;
    try { // (no exception may cross the C ABI: without the bookkeeping, the calling thread runs them all)
        rcs.assign(n, RG_OK);
        errs.resize(n);
        workers.reserve(n);
    } catch (const std::exception &) {
        return run_host(runs.data(), n);
    }
    size_t started = 0;
    try {
        for (; started < n; ++started)
            workers.emplace_back([&runs, &rcs, &errs, started]() {
                place_thread(runs[started].ctx->numa_node); // the CPUs (and memory) next to this GPU
                rcs[started] = run_host(&runs[started], 1);
                if (rcs[started] != RG_OK) errs[started].swap(err_text()); // the worker's own message, moved out
            });
    } catch (const std::exception &) {
        // fewer threads than runs (std::system_error): the rest run here, stepped together as before
    }
    int rc_here = RG_OK;
    std::string err_here;
    if (started < n) {
        rc_here = run_host(&runs[started], n - started);
        if (rc_here != RG_OK) err_here.swap(err_text()); // (swaps: no string copy that could throw)
    }
    for (auto &t : workers) t.join();
    for (size_t k = 0; k < started; ++k)
        if (rcs[k] != RG_OK) {
            err_text().swap(errs[k]);
            return rcs[k];
        }
    if (rc_here != RG_OK) err_text().swap(err_here);
    return rc_here;
}

// A slice moves the byte span of its frames H2D and back D2H, so slices must cover disjoint spans: with
// the descriptors in offset order they do (frames do not overlap), in any other order a slice's span
// would take in other slices' frames and its D2H copy could put back stale bytes over their results.
// Batches not in offset order therefore run on a sorted copy of the descriptors (and counters), their
// statuses and counters scattered back to the caller's order afterwards.
struct HostOrder {
    bool identity = true;
    std::vector<rg_pkt_desc> desc;
    std::vector<uint64_t> ctr, ctr_out;
    std::vector<uint8_t> status;
    std::vector<uint32_t> perm; // sorted position k -> caller index
};

bool in_offset_order(const rg_pkt_desc *desc, size_t n) {
    for (size_t i = 1; i < n; ++i)
        if (desc[i].offset < desc[i - 1].offset) return false;
    return true;
}

// RunFn(desc, counters, status, counters_out): the pipeline over the (possibly permuted) arrays
template <class RunFn>
int run_ordered(const rg_pkt_desc *desc, const uint64_t *counters, size_t n, uint8_t *status, uint64_t *counters_out,
                RunFn &&run) {
    if (in_offset_order(desc, n)) return run(desc, counters, status, counters_out);
    HostOrder o;
    o.perm.resize(n);
    for (size_t i = 0; i < n; ++i) o.perm[i] = (uint32_t)i;
    std::stable_sort(o.perm.begin(), o.perm.end(),
                     [&](uint32_t a, uint32_t b) { return desc[a].offset < desc[b].offset; });
    o.desc.resize(n);
    o.status.resize(n);
    for (size_t k = 0; k < n; ++k) o.desc[k] = desc[o.perm[k]];
    if (counters) {
        o.ctr.resize(n);
        for (size_t k = 0; k < n; ++k) o.ctr[k] = counters[o.perm[k]];
    }
    if (counters_out) o.ctr_out.resize(n);
    const int rc = run(o.desc.data(), counters ? o.ctr.data() : nullptr, o.status.data(),
                       counters_out ? o.ctr_out.data() : nullptr);
    for (size_t k = 0; k < n; ++k) {
        status[o.perm[k]] = o.status[k];
        if (counters_out) counters_out[o.perm[k]] = o.ctr_out[k];
    }
    return rc;
}

int host_batch(rg_ctx *ctx, bool open, uint32_t nkeys, const rg_pkt_desc *desc, const uint64_t *counters, size_t n,
               uint8_t *buf, size_t buf_len, uint8_t *status, uint64_t *counters_out, bool with_receivers) {
    return run_ordered(desc, counters, n, status, counters_out,
                       [&](const rg_pkt_desc *d, const uint64_t *c, uint8_t *st, uint64_t *co) {
                           HostRun run{ctx, open, nkeys, d, c, 0, n, buf, buf_len, st, co, with_receivers};
                           return run_host(&run, 1);
                       });
}

// The end of every host call on a context: the key table's upload on hs_in has completed (a context of a
// group that ran no slice, or a call that failed before its first slice, never waited for it, and the
// caller may reuse a pinned key buffer as soon as the call returns: ADVICE r5), and a failed call leaves
// every status pending (include/rg_aead.h).
int settle_host(rg_ctx *ctx, int rc) {
    hipError_t e = ctx->ev_in_idle.ensure();
    if (e == hipSuccess) e = hipEventRecord(ctx->ev_in_idle.get(), ctx->hs_in);
    int r2 = e == hipSuccess ? wait_event(ctx->ev_in_idle.get(), ctx->wait_ms, "key upload")
                             : set_err(RG_EDEVICE, "key upload", e);
    return rc != RG_OK ? rc : r2;
}

// work of packet i for the split: its AEAD payload bytes plus one 64-byte one-time-key block
uint64_t split_work(const rg_pkt_desc &d, bool open) {
    const uint64_t P = open ? (d.len >= 32 ? d.len - 32 : 0) : d.len;
    return std::min<uint64_t>(P, rg::kMaxPayload) + 64;
}

void split_bounds(const rg_pkt_desc *desc, size_t n, bool open, int parts, size_t *bounds) {
    uint64_t total = 0;
    for (size_t i = 0; i < n; ++i) total += split_work(desc[i], open);
    bounds[0] = 0;
    size_t i = 0;
    uint64_t run = 0;
    for (int k = 1; k < parts; ++k) {
        // the first index whose running work before it reaches k / parts of the total
        const uint64_t target = (uint64_t)((long double)total * k / parts);
        while (i < n && run + split_work(desc[i], open) / 2 < target) run += split_work(desc[i++], open);
        bounds[k] = i;
    }
    bounds[parts] = n;
}

// every context of the group, locked in index order (a group's calls are serialised per context as
// a single context's are)
struct GroupLock {
    std::vector<std::unique_lock<std::mutex>> held;
    explicit GroupLock(rg_group *g) {
        for (rg_ctx *c : g->ctx) held.emplace_back(c->mu);
    }
};

int host_multi(rg_group *g, bool open, const uint8_t *keys, const uint32_t *receivers, uint32_t nkeys,
               const rg_pkt_desc *desc, const uint64_t *counters, size_t n, uint8_t *buf, size_t buf_len,
               uint8_t *status, uint64_t *counters_out) {
    DeviceGuard dg;
    GroupLock lk(g);
    const int parts = (int)g->ctx.size();
    int rc = RG_OK;
    int uploaded = 0; // contexts whose key upload was enqueued (each is settled below)
    for (; uploaded < parts && rc == RG_OK; ++uploaded) {
        const hipError_t e = hipSetDevice(g->ctx[uploaded]->device);
        rc = e != hipSuccess ? set_err(RG_EDEVICE, "hipSetDevice", e)
                             : upload_keys(g->ctx[uploaded], keys, receivers, nkeys);
    }
    // the split is over the batch in offset order, so the contexts' byte spans are disjoint too
    if (rc == RG_OK)
        rc = run_ordered(desc, counters, n, status, counters_out,
                         [&](const rg_pkt_desc *d, const uint64_t *c, uint8_t *st, uint64_t *co) {
                             std::vector<size_t> b(parts + 1);
                             split_bounds(d, n, open, parts, b.data());
                             std::vector<HostRun> runs;
                             for (int k = 0; k < parts; ++k)
                                 if (b[k] < b[k + 1])
                                     runs.push_back(HostRun{g->ctx[k], open, nkeys, d, c, b[k], b[k + 1], buf,
                                                            buf_len, st, co, receivers != nullptr});
                             return run_host_group(runs);
                         });
    for (int k = 0; k < uploaded; ++k) {
        (void)hipSetDevice(g->ctx[k]->device);
        rc = settle_host(g->ctx[k], rc);
    }
    return fail_closed(rc, status, n);
}

// Every shard's arguments are checked before any shard is enqueued (a call that failed on
// shard k after enqueuing shards 0..k-1 left the caller unable to tell which frames were sealed, and a
// retry would seal those again under new counters).  A launch that fails after the checks names its
// shard in rg_last_error; the shards before it are enqueued (include/rg_aead.h).
int dev_multi(rg_group *g, const rg_dev_shard *sh, bool open) {
    const char *op = open ? "open" : "seal";
    char what[384];
    if (!g || !sh) {
        snprintf(what, sizeof what, "%s_dev_multi: bad args", op);
        return set_err(RG_EINVAL, what);
    }
    for (size_t k = 0; k < g->ctx.size(); ++k) {
        const rg_dev_shard &x = sh[k];
        if (x.n == 0) continue;
        const bool bad = !g->ctx[k] || !x.keys || !x.desc || !x.buf || !x.status || x.nkeys == 0 ||
                         x.n > 0xFFFFFFFFull || (!open && !x.counters);
        if (bad) {
            snprintf(what, sizeof what, "%s_dev_multi: bad args in shard %zu (nothing enqueued)", op, k);
            return set_err(RG_EINVAL, what);
        }
    }
    DeviceGuard dg;
    for (size_t k = 0; k < g->ctx.size(); ++k) {
        const rg_dev_shard &x = sh[k];
        const int rc = open ? rg_open_batch_dev(g->ctx[k], x.keys, x.nkeys, x.desc, x.n, x.buf, x.buf_len, x.status,
                                                x.counters_out, x.stream)
                            : rg_seal_batch_dev(g->ctx[k], x.keys, x.receivers, x.nkeys, x.desc, x.counters, x.n, x.buf,
                                                x.buf_len, x.status, x.stream);
        if (rc == RG_OK) continue;
        const std::string inner = err_text();
        if (k == 0)
            snprintf(what, sizeof what, "%s_dev_multi: shard 0 failed (nothing enqueued): %s", op, inner.c_str());
        else
            snprintf(what, sizeof what, "%s_dev_multi: shard %zu failed (shards 0..%zu enqueued): %s", op, k, k - 1,
                     inner.c_str());
        return set_err(rc, what);
    }
    return RG_OK;
}

} // namespace

extern "C" {

int rg_seal_batch_host(rg_ctx *ctx, const uint8_t *keys, const uint32_t *receivers, uint32_t nkeys,
                       const rg_pkt_desc *desc, const uint64_t *counters, size_t n, uint8_t *buf, size_t buf_len,
                       uint8_t *status) {
    DeviceGuard dg_;
    int rc = check_ctx(ctx);
    if (rc) return fail_closed(rc, status, n);
    if (n == 0) return RG_OK;
    if (!keys || !desc || !counters || !buf || nkeys == 0)
        return fail_closed(set_err(RG_EINVAL, "seal_host: bad args"), status, n);
    std::lock_guard<std::mutex> g(ctx->mu);
    std::vector<uint8_t> tmp;
    if (!status) {
        tmp.resize(n);
        status = tmp.data();
    }
    rc = upload_keys(ctx, keys, receivers, nkeys);
    if (rc == RG_OK)
        rc = host_batch(ctx, false, nkeys, desc, counters, n, buf, buf_len, status, nullptr, receivers != nullptr);
    return fail_closed(settle_host(ctx, rc), status, n);
}

int rg_open_batch_host(rg_ctx *ctx, const uint8_t *keys, uint32_t nkeys, const rg_pkt_desc *desc, size_t n,
                       uint8_t *buf, size_t buf_len, uint8_t *status, uint64_t *counters_out) {
    DeviceGuard dg_;
    int rc = check_ctx(ctx);
    if (rc) return fail_closed(rc, status, n);
    if (n == 0) return RG_OK;
    if (!keys || !desc || !buf || !status || nkeys == 0)
        return fail_closed(set_err(RG_EINVAL, "open_host: bad args"), status, n);
    std::lock_guard<std::mutex> g(ctx->mu);
    std::vector<uint64_t> tmp;
    if (!counters_out) {
        tmp.resize(n);
        counters_out = tmp.data();
    }
    rc = upload_keys(ctx, keys, nullptr, nkeys);
    if (rc == RG_OK) rc = host_batch(ctx, true, nkeys, desc, nullptr, n, buf, buf_len, status, counters_out, false);
    return fail_closed(settle_host(ctx, rc), status, n);
}

int rg_group_create(const int *devices, int n, rg_group **out) {
    if (!out) return set_err(RG_EINVAL, "group: null out");
    *out = nullptr;
    if (!devices || n <= 0 || n > 64) return set_err(RG_EINVAL, "group: 1..64 devices");
    rg_group *g = new (std::nothrow) rg_group();
    if (!g) return set_err(RG_ENOMEM, "alloc group");
    DeviceGuard dg;
    for (int i = 0; i < n; ++i) {
        rg_ctx *c = nullptr;
        int rc = rg_create(devices[i], &c);
        if (rc) {
            rg_group_destroy(g);
            return rc;
        }
        g->ctx.push_back(c);
    }
    *out = g;
    return RG_OK;
}

void rg_group_destroy(rg_group *g) {
    if (!g) return;
    DeviceGuard dg;
    for (rg_ctx *c : g->ctx) rg_destroy(c);
    delete g;
}

int rg_group_size(const rg_group *g) { return g ? (int)g->ctx.size() : set_err(RG_EINVAL, "group: null"); }

rg_ctx *rg_group_ctx(rg_group *g, int i) {
    if (!g || i < 0 || i >= (int)g->ctx.size()) return nullptr;
    return g->ctx[i];
}

int rg_split_batch(const rg_pkt_desc *desc, size_t n, int open, int parts, size_t *bounds) {
    if (!bounds || parts <= 0 || (n && !desc)) return set_err(RG_EINVAL, "split: bad args");
    split_bounds(desc, n, open != 0, parts, bounds);
    return RG_OK;
}

int rg_seal_batch_host_multi(rg_group *g, const uint8_t *keys, const uint32_t *receivers, uint32_t nkeys,
                             const rg_pkt_desc *desc, const uint64_t *counters, size_t n, uint8_t *buf,
                             size_t buf_len, uint8_t *status) {
    if (!g || g->ctx.empty()) return fail_closed(set_err(RG_EINVAL, "seal_host_multi: null group"), status, n);
    if (n == 0) return RG_OK;
    if (!keys || !desc || !counters || !buf || nkeys == 0)
        return fail_closed(set_err(RG_EINVAL, "seal_host_multi: bad args"), status, n);
    std::vector<uint8_t> tmp;
    if (!status) {
        tmp.resize(n);
        status = tmp.data();
    }
    return host_multi(g, false, keys, receivers, nkeys, desc, counters, n, buf, buf_len, status, nullptr);
}

int rg_open_batch_host_multi(rg_group *g, const uint8_t *keys, uint32_t nkeys, const rg_pkt_desc *desc, size_t n,
                             uint8_t *buf, size_t buf_len, uint8_t *status, uint64_t *counters_out) {
    if (!g || g->ctx.empty()) return fail_closed(set_err(RG_EINVAL, "open_host_multi: null group"), status, n);
    if (n == 0) return RG_OK;
    if (!keys || !desc || !buf || !status || nkeys == 0)
        return fail_closed(set_err(RG_EINVAL, "open_host_multi: bad args"), status, n);
    std::vector<uint64_t> tmp;
    if (!counters_out) {
        tmp.resize(n);
        counters_out = tmp.data();
    }
    return host_multi(g, true, keys, nullptr, nkeys, desc, nullptr, n, buf, buf_len, status, counters_out);
}

int rg_seal_batch_dev_multi(rg_group *g, const rg_dev_shard *sh) { return dev_multi(g, sh, false); }

int rg_open_batch_dev_multi(rg_group *g, const rg_dev_shard *sh) { return dev_multi(g, sh, true); }

} // extern "C"
