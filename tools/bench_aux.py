#!/usr/bin/env python3
"""Throughput of the SURVEY 8(f) rows beside the transport AEAD (one MI355X):

  mac1   rg_mac_verify_batch_dev: 1 Mi handshake-initiation messages (148 B), mac1 checked under the
         message's own key, and under an 8-peer scan (RG_KEY_SCAN, wg-proxy)
  cookie rg_cookie_reply_batch_dev: 1 Mi initiations with a valid mac1 and no valid mac2, all overloaded, so
         every message takes the whole path (mac1, cookie, mac2, sealed CookieMessage); beside it, in the
         same run, rg_mac_verify_batch_dev (which = 1) on the same batch, and their ratio
  rx     rg_open_batch_dev_rx vs rg_open_batch_dev on config 4 frames (256 sessions): the cost of
         resolving every frame's session from its header on the device

  replay the device-frame receive on cfg2 (64 Ki x 1500 B, one session) and cfg4 (256 sessions x 4 Ki x 1500 B),
         same frames, three ways in one run: (a) rg_open_batch_dev_rx alone (the floor), (b) rg_recv_batch_dev +
         rg_recv_batch_dev_finish (host wall clock: the path waits on the host), (c) rg_recv_batch_dev_resident;
         fresh counters only, and 10 % replays of the previous batch.  Also written to
         profiles/replay_resident_bench.json

  send   the device-frame send on cfg2 and cfg4 geometry (cfg4: 256 sessions interleaved in hash order, not sorted),
         same plaintext, three ways in one run: (a) rg_seal_batch_dev with precomputed counters (the floor),
         (b) rg_send_batch_dev (host wall clock: the host hands out the counters), (c) rg_send_batch_dev_resident.
         Also written to profiles/send_resident_bench.json

  handshake  the batched IKpsk2 responder at 64 Ki and 1 Ki rows (256 distinct valid initiations, tiled):
         rg_x25519_batch_dev alone, rg_handshake_init_batch_dev, rg_handshake_resp_batch_dev and both as
         handshakes/s, by stream events, medians of seven with min-max; OpenSSL's X25519 through libcrypto on 1
         and 16 threads beside it when the library is there.  Also written to profiles/handshake_bench.json

  initiator  the batched IKpsk2 initiator at 64 Ki and 1 Ki rows: rg_handshake_initiate_batch_dev,
         rg_handshake_finish_batch_dev and both, and in the same run the responder calls and rg_x25519_batch_dev
         on the same handshakes, by stream events, medians of seven with min-max, with each call's time per
         X25519 ladder.  Also written to profiles/handshake_initiator_bench.json

  route  cryptokey routing on cfg2 and cfg4 geometry under a table of 256 prefixes of mixed length (/16 to /32,
         one peer each; cfg4: peer = session, cfg2: every peer on the one session), every packet an IPv4 packet
         of 1500 bytes: rg_send_batch_dev_routed against rg_send_batch_dev_resident with precomputed slots and
         padded descriptors on the same plaintext, and rg_recv_batch_dev_resident followed by
         rg_route_check_batch_dev against rg_recv_batch_dev_resident alone on the same frames; rg_route_batch_dev
         alone beside them.  Medians of seven with min-max, by stream events and by host wall clock.  Also
         written to profiles/route_bench.json

  peerstate  the device-resident peer handshake state at 64 Ki and 1 Ki rows: the responder chain (init -> ts ->
         cookies -> resp -> mac1) against init + resp alone, the initiator chain (cookies -> initiate -> mac1)
         against initiate alone, and rg_peer_ts_batch_dev, rg_peer_cookies_batch_dev, rg_peer_mac1_batch_dev and
         rg_peer_cookie_consume_batch_dev each alone, by stream events, medians of seven with min-max.  Also
         written to profiles/peerstate_bench.json

  session  the device-resident session table: rg_session_install_batch_dev of 1 Ki and 64 Ki finished handshakes
         into tables of 64 Ki and 1 Mi rows, half full; rg_session_expire_batch_dev of 10 % of the rows;
         rg_session_index_dev (the receiver-table rebuild every call pays) alone; and, for 1 Ki handshakes into
         the 64 Ki table, what a caller does today on the same rows: keys and ids to pinned host memory,
         rg_sessions_insert_peer per row, the mirror refresh of the next device call.  Medians of seven with
         min-max, by stream events and by host wall clock.  Also written to profiles/session_install_bench.json

  timers  the device-resident session timers: rg_timer_turn_dev over tables of 64 Ki and 1 Mi rows (four rows per
         peer) with about 1 % and about 50 % of the rows due, beside rg_session_expire_batch_dev on the same table;
         the keepalive send over the turn's padded list (n = npeers) beside the same send over the due rows alone;
         and rg_timer_arm_batch_dev, rg_timer_note_send_batch_dev and rg_timer_note_recv_batch_dev at 64 Ki
         packets.  Medians of seven with min-max, by stream events.  Also written to profiles/timers_bench.json

  pending  the device-resident pending handshakes at 16 Ki and 256 Ki peers with about 1 % and about 50 % of the
         rows due for a retry: rg_pending_turn_dev (alone and fed the timer turn's rekey list),
         rg_pending_install_batch_dev behind the chain and rg_pending_index_dev, beside rg_timer_turn_dev and the
         bare initiator chain (cookies -> initiate -> mac1, n = npeers) in the same run.  Medians of seven with
         min-max, by stream events.  Also written to profiles/pending_bench.json

  ratelimit  the device-resident handshake rate limiter on the default sketch: rg_rate_count_batch_dev at 1 Ki and
         64 Ki initiations from 1, 256 and 20 000 distinct source addresses, rg_cookie_reply_batch_dev on the same
         batch beside it (fed the count's flags, and all overloaded), and rg_rate_turn_dev with and without a
         reset.  Medians of seven with min-max, by stream events.  Also written to profiles/ratelimit_bench.json

  endpoint  the device-resident peer endpoints on cfg2, cfg4 and 1 Ki packets of one session: the resident receive
         + rg_timer_note_recv_batch_dev with and without rg_endpoint_note_recv_batch_dev, the resident send with and
         without rg_endpoint_gate_batch_dev, the note, the gate and the timer note each alone, by stream events,
         medians of seven with min-max; and by host wall clock the read-back and numpy last-per-peer a caller does
         today.  Also written to profiles/endpoint_bench.json

  demux  the device-resident inbound demultiplexer at 64 Ki and 1 Mi datagrams on an IMIX-like mix and an
         all-handshake flood: rg_demux_batch_dev, rg_demux_verdict_batch_dev and rg_timer_turn_dev over as many rows by
         stream events, medians of seven with min-max; by host wall clock the read-back, numpy split and upload they
         replace; and rg_handshake_init_batch_dev over a padded against a dense list.  Also written to
         profiles/demux_bench.json

Prints one JSON object.  Synthetic data (random messages: every MAC check does the full work and
rejects, which costs the same as accepting).  Legs named on the command line run alone (default: all)."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rustyguard_amd import aead, route, workloads  # noqa: E402
from rustyguard_amd.device import DeviceBatch  # noqa: E402
from rustyguard_amd.workloads import DESC_DTYPE  # noqa: E402


def timed(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def cookie_leg(eng, n=1 << 20):
    L = 148
    rng = np.random.default_rng(17)
    ck = rng.integers(0, 256, 96, dtype=np.uint8)  # rg_cookie_keys: mac1_key, cookie_key, secret
    mac1_key = ck[:32].tobytes()
    host = rng.integers(0, 256, (n, 160), dtype=np.uint8)
    host[:, 0:4] = (1, 0, 0, 0)  # HandshakeInit
    host[:, L - 16:L] = 0        # no mac2
    for row in host:             # a valid mac1: the reply path runs for every message
        row[L - 32:L - 16] = np.frombuffer(hashlib.blake2s(row[:L - 32].tobytes(), key=mac1_key, digest_size=16).digest(),
                                           np.uint8)
    desc = np.zeros(n, DESC_DTYPE)
    desc["offset"] = np.arange(n, dtype=np.uint64) * 160
    desc["len"] = L
    buf = torch.from_numpy(host.reshape(-1)).cuda()
    d = torch.from_numpy(desc.view(np.uint8).reshape(-1, 16)).cuda()
    keys = torch.from_numpy(ck).cuda()
    addrs = torch.from_numpy(rng.integers(0, 256, (n, 24), dtype=np.uint8)).cuda()
    nonces = torch.from_numpy(rng.integers(0, 256, (n, 24), dtype=np.uint8)).cuda()
    replies = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    st = torch.zeros(n, dtype=torch.uint8, device="cuda")
    st1 = torch.zeros(n, dtype=torch.uint8, device="cuda")
    mac1_keys = keys[:32].clone()
    # alternating repetitions, medians (the two calls are compared with each other)
    t_cookie, t_mac1 = [], []
    for _ in range(5):
        t_cookie.append(timed(lambda: eng.cookie_reply_dev(keys, d, addrs, None, nonces, buf, replies, st)))
        t_mac1.append(timed(lambda: eng.mac_verify_dev(mac1_keys, 1, d, buf, st1)))
    assert (st == aead.PKT_COOKIE).all().item() and (st1 == aead.PKT_OK).all().item()
    ms_c, ms_m = float(np.median(t_cookie)), float(np.median(t_mac1))
    return {"messages": n, "bytes_each": L, "cookie_reply_ms": round(ms_c, 4),
            "cookie_reply_mmsg_s": round(n / ms_c / 1e3, 1), "mac1_only_ms": round(ms_m, 4),
            "mac1_only_mmsg_s": round(n / ms_m / 1e3, 1), "cookie_over_mac1": round(ms_c / ms_m, 2),
            "note": "medians of 5 alternating repetitions of 20 launches; mac1-only = rg_mac_verify_batch_dev "
                    "(its key-state launch included) on the same batch; compressions per message 7 vs 2"}


def mac1_leg(eng):
    n, L = 1 << 20, 148
    rng = np.random.default_rng(5)
    keys = torch.from_numpy(rng.integers(0, 256, (8, 32), dtype=np.uint8)).cuda()
    desc = np.zeros(n, DESC_DTYPE)
    desc["offset"] = np.arange(n, dtype=np.uint64) * 160
    desc["len"] = L
    desc["key_idx"] = rng.integers(0, 8, n)
    buf = torch.randint(0, 256, (n * 160,), dtype=torch.uint8, device="cuda")
    d = torch.from_numpy(desc.view(np.uint8).reshape(-1, 16)).cuda()
    st = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ms_own = timed(lambda: eng.mac_verify_dev(keys, 1, d, buf, st))
    desc["key_idx"] = aead.KEY_SCAN
    ds = torch.from_numpy(desc.view(np.uint8).reshape(-1, 16)).cuda()
    ms_scan = timed(lambda: eng.mac_verify_dev(keys, 1, ds, buf, st))
    return {"messages": n, "bytes_each": L, "own_key_ms": round(ms_own, 4),
            "own_key_mmsg_s": round(n / ms_own / 1e3, 1), "scan8_ms": round(ms_scan, 4),
            "scan8_mmsg_s": round(n / ms_scan / 1e3, 1)}


def rx_leg(eng):
    w = workloads.build("cfg4")  # 256 sessions: a real table
    b = DeviceBatch(eng, w)
    b.fill()
    torch.cuda.synchronize()
    table = torch.from_numpy(aead.rx_table(w.receivers, np.arange(len(w.receivers), dtype=np.uint32))).cuda()

    def seal_open(rx):
        b.seal()
        if rx:
            eng.open_dev_rx(b.keys, table, b.desc_open, b.buf, b.status)
        else:
            eng.open_dev(b.keys, b.desc_open, b.buf, b.status)

    # alternating repetitions, medians: box-to-box and run-to-run noise on a 2 ms
    # step is larger than the ~50 us being measured
    t_open, t_rx = [], []
    for _ in range(7):
        t_open.append(timed(lambda: seal_open(False), 10))
        t_rx.append(timed(lambda: seal_open(True), 10))
    assert (b.status[: w.n] == 0).all().item()
    ms_open, ms_rx = float(np.median(t_open)), float(np.median(t_rx))
    return {"workload": "cfg4 (1 Mi packets, 256 sessions)", "seal_open_ms": round(ms_open, 4),
            "seal_open_rx_ms": round(ms_rx, 4), "resolve_overhead_us": round((ms_rx - ms_open) * 1e3, 2),
            "note": "medians of 7 alternating repetitions of 10 steps; the rx_resolve kernel itself is in the "
                    "rocprofv3 kernel stats"}


def sessions_leg(eng):
    # the device-resident session layer on config-2 geometry (64 Ki x 1504 B, one session): B seals
    # with rg_send_batch_dev (fresh counters every round), A receives with rg_recv_batch_dev; the host
    # half (rg_recv_batch_dev_finish: in-order anti-replay pass, flags, status write-back) is timed
    # on its own
    import time

    w = workloads.build("cfg2")
    b = DeviceBatch(eng, w)
    b.fill()
    rng = np.random.default_rng(9)
    k1, k2 = rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    sa, sb = aead.Sessions(eng, 4), aead.Sessions(eng, 4)
    slot_a = sa.insert(0x1111, 0x2222, k1, k2)
    slot_b = sb.insert(0x2222, 0x1111, k2, k1)
    slots = np.full(w.n, slot_b, np.uint32)
    t_send, t_gpu, t_fin = [], [], []
    for it in range(12):
        b.fill()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sb.send_batch_dev(slots, b.desc_seal, b.buf, b.status)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        sa.recv_batch_dev(b.desc_open, b.buf, b.status)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        st, sl, fl = sa.recv_batch_dev_finish(w.n)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        assert (st == 0).all() and (sl == slot_a).all()
        if it >= 2:
            t_send.append(t1 - t0)
            t_gpu.append(t2 - t1)
            t_fin.append(t3 - t2)
    med = lambda x: float(np.median(x)) * 1e3  # noqa: E731
    return {"workload": "cfg2 geometry, one session", "packets": w.n,
            "send_batch_dev_ms": round(med(t_send), 4), "recv_batch_dev_ms": round(med(t_gpu), 4),
            "recv_finish_ms": round(med(t_fin), 4),
            "recv_mpkt_s": round(w.n / (med(t_gpu) + med(t_fin)) / 1e3, 2),
            "note": "wall-clock medians of 10 rounds, each call followed by a device sync; finish is "
                    "the host's in-order anti-replay pass plus the status write-back"}


def replay_leg(eng):
    import ctypes
    import time

    def shape(cfg):
        w = workloads.build(cfg)
        n, nk = w.n, len(w.receivers)
        b = DeviceBatch(eng, w)
        off = w.desc["offset"].astype(np.int64)
        stride = int(off[1] - off[0])
        assert (np.diff(off) == stride).all() and w.buf_bytes >= n * stride
        rows = lambda t: t[: n * stride].view(n, stride)  # noqa: E731
        # batch 1 (the workload's counters) and batch 2 (the same sessions, 2^24 further on)
        b.fill()
        b.seal()
        batch1 = b.buf.clone()
        b.fill()
        eng.seal_dev(b.keys, b.receivers, b.desc_seal, b.counters + (1 << 24), b.buf, b.status)
        fresh = b.buf.clone()
        mixed = fresh.clone()
        rows(mixed)[::10] = rows(batch1)[::10]  # 10 % replays of the previous batch
        torch.cuda.synchronize()
        table = torch.from_numpy(aead.rx_table(w.receivers, np.arange(nk, dtype=np.uint32))).cuda()
        ws = eng.replay_workspace(n, nk)
        win = torch.zeros(nk * 33, dtype=torch.int64, device="cuda")
        eng.recv_batch_dev_resident(b.keys, table, win, b.desc_open, batch1.clone(), b.status, workspace=ws)
        torch.cuda.synchronize()
        assert (b.status[:n] == 0).all().item()
        win1 = win.clone()  # the windows after batch 1
        tab = aead.Sessions(eng, nk)
        slots = [tab.insert(int(w.receivers[s]), 0x70000000 + s, bytes(32), w.keys.reshape(-1, 32)[s].tobytes())
                 for s in range(nk)]
        host1 = win1.cpu().numpy().view(np.uint8).reshape(nk, 264)
        ptrs = [eng.library.rg_sessions_replay(tab._h, sl) for sl in slots]

        def restore(frames):
            b.buf.copy_(frames)
            win.copy_(win1)
            for s, p in enumerate(ptrs):
                ctypes.memmove(p, host1[s].ctypes.data, 264)
            torch.cuda.synchronize()

        def gpu_ms(fn):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            z.record()
            torch.cuda.synchronize()
            return a.elapsed_time(z)

        def wall_ms(fn):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def floor():
            eng.open_dev_rx(b.keys, table, b.desc_open, b.buf, b.status)

        def parent():
            tab.recv_batch_dev(b.desc_open, b.buf, b.status)
            tab.recv_batch_dev_finish(n)

        def resident():
            eng.recv_batch_dev_resident(b.keys, table, win, b.desc_open, b.buf, b.status, workspace=ws)

        out = {"packets": n, "sessions": nk}
        for mix, frames in (("fresh", fresh), ("replay10", mixed)):
            t = {"a_open_rx_gpu_ms": [], "b_parent_wall_ms": [], "c_resident_gpu_ms": [], "c_resident_wall_ms": []}
            want = None
            for rep in range(9):
                restore(frames)
                t["a_open_rx_gpu_ms"].append(gpu_ms(floor))
                restore(frames)
                t["b_parent_wall_ms"].append(wall_ms(parent))
                st_b = b.status[:n].clone()
                restore(frames)
                t["c_resident_gpu_ms"].append(gpu_ms(resident))
                assert torch.equal(b.status[:n], st_b), "resident and parent paths disagree"
                restore(frames)
                t["c_resident_wall_ms"].append(wall_ms(resident))
                want = int((st_b == 3).sum().item())
            r = {k: {"median": round(float(np.median(v[2:])), 4), "min": round(min(v[2:]), 4),
                     "max": round(max(v[2:]), 4)} for k, v in t.items()}
            r["rejected"] = want
            r["c_over_a"] = round(r["c_resident_gpu_ms"]["median"] / r["a_open_rx_gpu_ms"]["median"], 3)
            r["b_over_c"] = round(r["b_parent_wall_ms"]["median"] / r["c_resident_wall_ms"]["median"], 3)
            out[mix] = r
        return out

    res = {"cfg2": shape("cfg2"), "cfg4": shape("cfg4"),
           "note": "9 alternating repetitions per mix, the first two dropped; frames, device windows and the session "
                   "table's windows restored outside the timed region; (a) and (c) by stream events, (b) and (c) "
                   "also by host wall clock around the calls and a device sync"}
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                        "replay_resident_bench.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return res


def send_leg(eng):
    import time

    T = 10**12

    def shape(cfg):
        w = workloads.build(cfg)
        n, nk = w.n, len(w.receivers)
        b = DeviceBatch(eng, w)
        b.fill()
        plain = b.buf.clone()
        host_slots = np.ascontiguousarray(w.desc["key_idx"], np.uint32)  # cfg4: interleaved, not sorted
        slots = torch.from_numpy(host_slots.view(np.int32).copy()).cuda()
        tab = aead.Sessions(eng, nk)
        tab.set_time(T)
        keys = w.keys.reshape(-1, 32)
        assert [tab.insert(0x70000000 + s, int(w.receivers[s]), keys[s].tobytes(), bytes(32)) for s in range(nk)] == \
            list(range(nk))
        tab.set_time(T + 5)
        state0 = torch.from_numpy(np.tile(np.array([0, T, T], np.uint64), nk).view(np.int64)).cuda()
        state = state0.clone()
        now = torch.from_numpy(np.array([T + 5], np.uint64).view(np.int64)).cuda()
        ws = eng.send_workspace(n, nk)
        status_c = torch.zeros(n, dtype=torch.uint8, device="cuda")

        def restore():
            b.buf.copy_(plain)
            state.copy_(state0)
            for s in range(nk):
                tab.set_send_counter(s, 0)
            torch.cuda.synchronize()

        def gpu_ms(fn):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            z.record()
            torch.cuda.synchronize()
            return a.elapsed_time(z)

        def wall_ms(fn):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def floor():
            b.seal()

        def parent():
            tab.send_batch_dev(host_slots, b.desc_seal, b.buf, b.status)

        def resident():
            eng.send_batch_dev_resident(b.keys, b.receivers, state, slots, b.desc_seal, b.buf, status_c, now_ns=now,
                                        workspace=ws)

        t = {"a_seal_gpu_ms": [], "b_parent_wall_ms": [], "c_resident_gpu_ms": [], "c_resident_wall_ms": []}
        for rep in range(9):
            restore()
            t["a_seal_gpu_ms"].append(gpu_ms(floor))
            restore()
            t["b_parent_wall_ms"].append(wall_ms(parent))
            frames_b = b.buf.clone()
            restore()
            t["c_resident_gpu_ms"].append(gpu_ms(resident))
            assert torch.equal(status_c, b.status[:n]) and (status_c == 0).all().item(), "statuses disagree"
            assert torch.equal(b.buf, frames_b), "resident and parent paths sealed different frames"
            del frames_b
            restore()
            t["c_resident_wall_ms"].append(wall_ms(resident))
        r = {k: {"median": round(float(np.median(v[2:])), 4), "min": round(min(v[2:]), 4), "max": round(max(v[2:]), 4)}
             for k, v in t.items()}
        r["c_over_a"] = round(r["c_resident_gpu_ms"]["median"] / r["a_seal_gpu_ms"]["median"], 3)
        r["b_over_c"] = round(r["b_parent_wall_ms"]["median"] / r["c_resident_wall_ms"]["median"], 3)
        return {"packets": n, "sessions": nk, **r}

    res = {"cfg2": shape("cfg2"), "cfg4": shape("cfg4"),
           "note": "9 alternating repetitions, the first two dropped; frames, device state rows and the session "
                   "table's counters restored outside the timed region; (a) and (c) by stream events, (b) and (c) "
                   "also by host wall clock around the call and a device sync; (b) and (c) sealed identical "
                   "frames and statuses in every repetition"}
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                        "send_resident_bench.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return res


def route_leg(eng):
    import time

    T = 10**12
    NP = 256
    LENS = (16, 20, 24, 28, 32)

    def prefix(p):
        """peer p's one prefix, in a /16 of its own: (network as bytes, length)"""
        plen = LENS[p % len(LENS)]
        host = {16: (0, 0), 20: (64, 0), 24: (77, 0), 28: (77, 16), 32: (77, 5)}[plen]
        return bytes([10, p, *host]), plen

    def shape(cfg):
        w = workloads.build(cfg)
        n, nk = w.n, len(w.receivers)
        b = DeviceBatch(eng, w)
        off = w.desc["offset"].astype(np.int64)
        stride = int(off[1] - off[0])
        L, P = int(w.inner_len[0]), int(w.desc["len"][0])
        assert (np.diff(off) == stride).all() and w.buf_bytes >= n * stride and (w.inner_len == L).all()
        assert (w.desc["len"] == P).all() and P == (L + 15) // 16 * 16
        rows = lambda t: t[: n * stride].view(n, stride)  # noqa: E731
        table = torch.from_numpy(route.build_table([(prefix(p), p) for p in range(NP)]).view(np.int32)).cuda()
        slot = np.ascontiguousarray(w.desc["key_idx"], np.uint32)
        # cfg4: peer = session; cfg2: the packets go round the 256 peers, which all share the one session
        peer = slot if nk == NP else (np.arange(n) % NP).astype(np.uint32)
        peer_slot = np.arange(NP, dtype=np.uint32) if nk == NP else np.zeros(NP, np.uint32)
        slot_peer = np.arange(nk, dtype=np.uint32)  # the receiving side: key row k is peer k
        addr = np.array([list(prefix(p)[0]) for p in range(NP)], np.uint8)
        hdr = np.zeros((n, 20), np.uint8)
        hdr[:, 0], hdr[:, 2], hdr[:, 3], hdr[:, 8], hdr[:, 9] = 0x45, L >> 8, L & 255, 64, 17
        hdr[:, 12:16] = addr[slot_peer[slot]]  # a source of the session's own peer
        hdr[:, 16:20] = addr[peer]
        b.fill()
        rows(b.buf)[:, 16:36] = torch.from_numpy(hdr).cuda()
        rows(b.buf)[:, 16 + L:16 + P] = 0  # the padding as the route leaves it: both sends seal the same bytes
        plain = b.buf.clone()
        slots = torch.from_numpy(slot.view(np.int32).copy()).cuda()
        d_peer_slot = torch.from_numpy(peer_slot.view(np.int32).copy()).cuda()
        d_slot_peer = torch.from_numpy(slot_peer.view(np.int32).copy()).cuda()
        unpadded = w.desc.copy()
        unpadded["len"] = w.inner_len
        desc_in = torch.from_numpy(unpadded.view(np.uint8).reshape(-1, 16)).cuda()
        state0 = torch.from_numpy(np.tile(np.array([0, T, T], np.uint64), nk).view(np.int64)).cuda()
        state = state0.clone()
        now = torch.from_numpy(np.array([T + 5], np.uint64).view(np.int64)).cuda()
        ws_send, ws_route, ws_recv = eng.send_workspace(n, nk), route.route_workspace(eng, n, nk), eng.replay_workspace(n, nk)
        st_a = torch.zeros(n, dtype=torch.uint8, device="cuda")
        st_c = torch.zeros(n, dtype=torch.uint8, device="cuda")
        r_slots = torch.zeros(n, dtype=torch.int32, device="cuda")
        r_desc = torch.zeros((n, 16), dtype=torch.uint8, device="cuda")
        rx = torch.from_numpy(aead.rx_table(w.receivers, np.arange(nk, dtype=np.uint32))).cuda()
        win = torch.zeros(nk * 33, dtype=torch.int64, device="cuda")
        key = torch.zeros(n, dtype=torch.int32, device="cuda")
        inner = torch.zeros(n, dtype=torch.int32, device="cuda")

        def gpu_ms(fn):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            z.record()
            torch.cuda.synchronize()
            return a.elapsed_time(z)

        def wall_ms(fn):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def restore_send():
            b.buf.copy_(plain)
            state.copy_(state0)
            torch.cuda.synchronize()

        def resident():
            eng.send_batch_dev_resident(b.keys, b.receivers, state, slots, b.desc_seal, b.buf, st_a, now_ns=now,
                                        workspace=ws_send)

        def routed():
            route.send_batch_dev_routed(eng, b.keys, b.receivers, state, table, d_peer_slot, desc_in, b.buf, st_c,
                                        now_ns=now, workspace=ws_route)

        def route_only():
            route.route_batch_dev(eng, table, d_peer_slot, desc_in, b.buf, r_slots, r_desc, st_c)

        t = {k: [] for k in ("send_a_resident_gpu_ms", "send_a_resident_wall_ms", "send_c_routed_gpu_ms",
                             "send_c_routed_wall_ms", "route_alone_gpu_ms", "recv_a_resident_gpu_ms",
                             "recv_a_resident_wall_ms", "recv_c_checked_gpu_ms", "recv_c_checked_wall_ms",
                             "check_alone_gpu_ms")}
        frames = None
        for rep in range(9):
            restore_send()
            t["send_a_resident_gpu_ms"].append(gpu_ms(resident))
            frames_a = b.buf.clone()
            restore_send()
            t["send_c_routed_gpu_ms"].append(gpu_ms(routed))
            assert (st_a == 0).all().item() and (st_c == 0).all().item(), "a send verdict is not OK"
            assert torch.equal(b.buf, frames_a), "routed and resident sends sealed different frames"
            frames = frames_a
            restore_send()
            t["send_a_resident_wall_ms"].append(wall_ms(resident))
            restore_send()
            t["send_c_routed_wall_ms"].append(wall_ms(routed))
            restore_send()
            t["route_alone_gpu_ms"].append(gpu_ms(route_only))
            assert torch.equal(r_slots, slots)

        def restore_recv():
            b.buf.copy_(frames)
            win.zero_()
            torch.cuda.synchronize()

        def recv():
            eng.recv_batch_dev_resident(b.keys, rx, win, b.desc_open, b.buf, st_a, None, key, workspace=ws_recv)

        def check():
            route.route_check_batch_dev(eng, table, d_slot_peer, b.desc_open, key, b.buf, st_a, inner)

        def checked():
            recv()
            check()

        for rep in range(9):
            restore_recv()
            t["recv_a_resident_gpu_ms"].append(gpu_ms(recv))
            assert (st_a == 0).all().item(), "a receive verdict is not OK"
            t["check_alone_gpu_ms"].append(gpu_ms(check))
            assert (st_a == 0).all().item() and (inner == L).all().item(), "the check turned a packet away"
            restore_recv()
            t["recv_c_checked_gpu_ms"].append(gpu_ms(checked))
            restore_recv()
            t["recv_a_resident_wall_ms"].append(wall_ms(recv))
            restore_recv()
            t["recv_c_checked_wall_ms"].append(wall_ms(checked))
        r = {k: {"median": round(float(np.median(v[2:])), 4), "min": round(min(v[2:]), 4), "max": round(max(v[2:]), 4)}
             for k, v in t.items()}
        for side in ("send", "recv"):
            a_, c_ = (k for k in t if k.startswith(side) and k.endswith("gpu_ms"))
            r[f"{side}_c_over_a_gpu"] = round(r[c_]["median"] / r[a_]["median"], 3)
            a_, c_ = (k for k in t if k.startswith(side) and k.endswith("wall_ms"))
            r[f"{side}_c_over_a_wall"] = round(r[c_]["median"] / r[a_]["median"], 3)
        return {"packets": n, "sessions": nk, "prefixes": NP, "table_words": int(table.numel()), **r}

    res = {"cfg2": shape("cfg2"), "cfg4": shape("cfg4"),
           "note": "9 alternating repetitions, the first two dropped (medians of seven, min-max); plaintext, state rows "
                   "and windows restored outside the timed region; every figure by stream events (gpu_ms) or by host "
                   "wall clock around the call and a device sync (wall_ms); (a) the unrouted resident call, (c) the "
                   "routed send / the receive followed by the check, on the same frames in the same run; both sends "
                   "sealed identical frames and every verdict was OK in every repetition"}
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "route_bench.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return res


def _openssl_x25519(seconds=1.0):
    """OpenSSL's X25519 through libcrypto (ctypes releases the GIL, so threads run side by side): derivations
    per second on 1 and 16 threads, or None when the library is not there."""
    import ctypes
    import ctypes.util
    import threading
    import time

    name = ctypes.util.find_library("crypto")
    if not name:
        return None
    try:
        C = ctypes.CDLL(name)
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        C.EVP_PKEY_new_raw_private_key.restype = vp
        C.EVP_PKEY_new_raw_private_key.argtypes = [ctypes.c_int, vp, ctypes.c_char_p, sz]
        C.EVP_PKEY_new_raw_public_key.restype = vp
        C.EVP_PKEY_new_raw_public_key.argtypes = [ctypes.c_int, vp, ctypes.c_char_p, sz]
        C.EVP_PKEY_CTX_new.restype = vp
        C.EVP_PKEY_CTX_new.argtypes = [vp, vp]
        C.EVP_PKEY_derive_init.argtypes = [vp]
        C.EVP_PKEY_derive_set_peer.argtypes = [vp, vp]
        C.EVP_PKEY_derive.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(sz)]
        C.EVP_PKEY_CTX_free.argtypes = [vp]
        C.EVP_PKEY_free.argtypes = [vp]
    except (OSError, AttributeError):
        return None
    NID_X25519 = 1034

    def worker(count, stop):
        sk = C.EVP_PKEY_new_raw_private_key(NID_X25519, None, os.urandom(32), 32)
        pk = C.EVP_PKEY_new_raw_public_key(NID_X25519, None, bytes([9]) + bytes(31), 32)
        out, n = ctypes.create_string_buffer(32), 0
        while not stop.is_set():
            ctx = C.EVP_PKEY_CTX_new(sk, None)
            ln = sz(32)
            ok = C.EVP_PKEY_derive_init(ctx) == 1 and C.EVP_PKEY_derive_set_peer(ctx, pk) == 1 and \
                C.EVP_PKEY_derive(ctx, out, ctypes.byref(ln)) == 1
            C.EVP_PKEY_CTX_free(ctx)
            if not ok:
                count.append(-1)
                return
            n += 1
        C.EVP_PKEY_free(sk)
        C.EVP_PKEY_free(pk)
        count.append(n)

    res = {}
    for nt in (1, 16):
        count, stop = [], threading.Event()
        th = [threading.Thread(target=worker, args=(count, stop)) for _ in range(nt)]
        t0 = time.perf_counter()
        for t in th:
            t.start()
        time.sleep(seconds)
        stop.set()
        for t in th:
            t.join()
        if min(count) < 0:
            return None
        res[f"threads_{nt}_per_s"] = round(sum(count) / (time.perf_counter() - t0))
    return res


def handshake_leg(eng):
    """rg_x25519_batch_dev, rg_handshake_init_batch_dev and rg_handshake_resp_batch_dev at 64 Ki and 1 Ki rows
    (256 distinct valid initiations, tiled: the kernels' timing does not depend on the data), by stream events,
    medians of seven repetitions with min-max; OpenSSL's X25519 on the CPU beside it, in the same run.  Also
    written to profiles/handshake_bench.json."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import handshake_cases as hc  # the Python model makes the valid messages

    r = hc.Responder(41, npeers=8, neph=256)
    base = np.zeros((256, 160), np.uint8)
    for i in range(256):
        msg, _ = hc.make_initiation(r.sk_i[i % 8], r.pk_r, r.esk_i[i], hc.tai64n(1_800_000_000, i), i)
        base[i, :148] = np.frombuffer(msg, np.uint8)
    peers = hc.peer_rows(r.peers)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d_own, d_peers, d_table = dev(r.own), dev(peers), dev(aead.peer_table(peers))
    rng = np.random.default_rng(43)

    def ev_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def stats(ts, n, per=1):
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        return {"ms_median": round(med, 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4),
                "per_s_median": round(n * per / med * 1e3)}

    out = {}
    for n in (1 << 16, 1 << 10):
        buf = dev(np.tile(base, (n // 256, 1)).reshape(-1))
        desc = np.zeros(n, DESC_DTYPE)
        desc["offset"] = np.arange(n, dtype=np.uint64) * 160
        desc["len"] = 148
        d_desc = dev(desc.view(np.uint8).reshape(-1, 16))
        scal, pts = dev(rng.integers(0, 256, (n, 32), dtype=np.uint8)), dev(rng.integers(0, 256, (n, 32), dtype=np.uint8))
        xo = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
        st = torch.zeros(n, dtype=torch.uint8, device="cuda")
        res = torch.zeros((n, 128), dtype=torch.uint8, device="cuda")
        keep = torch.zeros((n, 128), dtype=torch.uint8, device="cuda")
        esk = dev(rng.integers(0, 256, (n, 32), dtype=np.uint8))
        sids = dev(np.arange(n, dtype=np.uint32))
        resp = torch.zeros((n, 96), dtype=torch.uint8, device="cuda")
        keys = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
        st2 = torch.zeros(n, dtype=torch.uint8, device="cuda")
        x = lambda: eng.x25519_dev(scal, pts, xo, st)  # noqa: E731
        ini = lambda: eng.handshake_init_dev(d_own, d_peers, d_table, d_desc, None, buf, res, st)  # noqa: E731
        rsp = lambda: eng.handshake_resp_dev(d_peers, res, None, esk, sids, None, None, resp, keys, st2)  # noqa: E731
        x(), ini()
        torch.cuda.synchronize()
        assert (st == aead.PKT_OK).all().item()
        keep.copy_(res)
        rsp()
        torch.cuda.synchronize()
        assert (st2 == aead.PKT_OK).all().item()
        t = {"x25519": [], "init": [], "resp": [], "both": []}
        for _ in range(7):
            t["x25519"].append(ev_ms(x))
            t["init"].append(ev_ms(ini))
            res.copy_(keep)  # the response call consumes its rows: give them back outside the timed window
            torch.cuda.synchronize()
            t["resp"].append(ev_ms(rsp))
            t["both"].append(ev_ms(lambda: (ini(), rsp())))
        out[f"rows_{n}"] = {"x25519": stats(t["x25519"], n), "init": stats(t["init"], n), "resp": stats(t["resp"], n),
                            "handshakes": stats(t["both"], n),
                            "ladders_per_s_in_handshakes": stats(t["both"], n, 5)["per_s_median"]}
    cpu = _openssl_x25519()
    out["cpu_openssl_x25519"] = cpu if cpu else "no CPU baseline"
    out["note"] = ("stream events around one call each, medians of 7 repetitions (one warm-up call before); rows are "
                   "256 distinct valid initiations over 8 peers, tiled; a handshake = the init call + the response "
                   "call = 5 X25519 ladders; CPU baseline: EVP_PKEY_derive in a loop per thread, same run")
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "handshake_bench.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


def initiator_leg(eng):
    """rg_handshake_initiate_batch_dev and rg_handshake_finish_batch_dev at 64 Ki and 1 Ki rows, and in the same
    run rg_handshake_init_batch_dev, rg_handshake_resp_batch_dev and rg_x25519_batch_dev on the same handshakes:
    stream events, medians of seven repetitions with min-max, and the time per X25519 ladder of each call
    (initiate / 3, finish / 2, init / 2, response / 3).  Written to profiles/handshake_initiator_bench.json."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import handshake_cases as hc  # the Python model makes the keys

    rng = np.random.default_rng(47)
    rb = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    sk_a, sk_b = rb(32), rb(32)
    pk_a, pk_b = hc.pubkey(sk_a), hc.pubkey(sk_b)
    psk = rb(32)
    others = [hc.pubkey(rb(32)) for _ in range(7)]
    peers_a = [(pk, rb(32), hc.mac1_key(pk)) for pk in others[:3]] + [(pk_b, psk, hc.mac1_key(pk_b))] + \
              [(pk, rb(32), hc.mac1_key(pk)) for pk in others[3:]]  # the responder is row 3 of 8
    peers_b = hc.peer_rows([(pk_a, psk, hc.mac1_key(pk_a))])
    a_own, a_peers = dev(np.frombuffer(sk_a + pk_a, np.uint8)), dev(hc.peer_rows(peers_a))
    b_own, b_peers, b_table = dev(np.frombuffer(sk_b + pk_b, np.uint8)), dev(peers_b), dev(aead.peer_table(peers_b))

    def ev_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def stats(ts, n, ladders):
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        return {"ms_median": round(med, 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4),
                "per_s_median": round(n / med * 1e3), "ladders": ladders,
                "us_per_ladder_row_median": round(med / ladders / n * 1e3, 5),
                "ms_per_ladder_median": round(med / ladders, 4), "ms_per_ladder_min": round(ts[0] / ladders, 4),
                "ms_per_ladder_max": round(ts[-1] / ladders, 4)}

    z = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype, device="cuda")  # noqa: E731
    out = {}
    for n in (1 << 16, 1 << 10):
        sids = np.arange(n, dtype=np.uint32) + 0x100
        pidx, esk_a, esk_b = dev(np.full(n, 3, np.uint32)), dev(rng.integers(0, 256, (n, 32), dtype=np.uint8)), \
            dev(rng.integers(0, 256, (n, 32), dtype=np.uint8))
        ts = dev(np.tile(np.frombuffer(hc.tai64n(1_800_000_000, 7), np.uint8), (n, 1)))
        d_sid_a, d_sid_b, a_table = dev(sids), dev(sids + 0x4000_0000), dev(aead.pending_table(sids))
        desc_i, desc_r = np.zeros(n, DESC_DTYPE), np.zeros(n, DESC_DTYPE)
        desc_i["offset"], desc_i["len"] = np.arange(n, dtype=np.uint64) * 160, 148
        desc_r["offset"], desc_r["len"] = np.arange(n, dtype=np.uint64) * 96, 92
        d_desc_i, d_desc_r = dev(desc_i.view(np.uint8).reshape(-1, 16)), dev(desc_r.view(np.uint8).reshape(-1, 16))
        msgs, pending = z(n, 160), z(n, 128)
        res, keep_r, resp, keys_b, keys_a = z(n, 128), z(n, 128), z(n, 96), z(n, 64), z(n, 64)
        st = [z(n) for _ in range(4)]
        pix, rem, claim = z(n, dtype=torch.int32), z(n, dtype=torch.int32), z(n, dtype=torch.int32)
        xo, xs, pts = z(n, 32), z(n), dev(rng.integers(0, 256, (n, 32), dtype=np.uint8))
        ini = lambda: eng.handshake_initiate_dev(a_own, a_peers, pidx, None, esk_a, ts, d_sid_a, None, None, msgs,  # noqa: E731
                                                 pending, st[0])
        cons = lambda: eng.handshake_init_dev(b_own, b_peers, b_table, d_desc_i, None, msgs, res, st[1])  # noqa: E731
        rsp = lambda: eng.handshake_resp_dev(b_peers, res, None, esk_b, d_sid_b, None, None, resp, keys_b, st[2])  # noqa: E731
        fin = lambda: eng.handshake_finish_dev(a_own, a_peers, a_table, pending, d_desc_r, None, resp, keys_a, pix,  # noqa: E731
                                               rem, claim, st[3])
        x = lambda: eng.x25519_dev(esk_a, pts, xo, xs)  # noqa: E731
        ini(), cons()
        keep_r.copy_(res)
        rsp(), fin(), x()
        torch.cuda.synchronize()
        assert all((s == aead.PKT_OK).all().item() for s in st)
        assert torch.equal(keys_a[:, :32], keys_b[:, 32:]) and torch.equal(keys_a[:, 32:], keys_b[:, :32])
        t = {k: [] for k in ("initiate", "finish", "both", "init", "resp", "x25519")}
        for _ in range(7):
            t["initiate"].append(ev_ms(ini))
            t["finish"].append(ev_ms(fin))  # the rows the initiate call has just written again
            t["both"].append(ev_ms(lambda: (ini(), fin())))
            t["init"].append(ev_ms(cons))
            res.copy_(keep_r)  # the response call consumes its rows: give them back outside the timed window
            torch.cuda.synchronize()
            t["resp"].append(ev_ms(rsp))
            t["x25519"].append(ev_ms(x))
        assert (st[3] == aead.PKT_OK).all().item()  # every timed finish did the whole work
        out[f"rows_{n}"] = {"initiate": stats(t["initiate"], n, 3), "finish": stats(t["finish"], n, 2),
                            "initiate_and_finish": stats(t["both"], n, 5), "init": stats(t["init"], n, 2),
                            "resp": stats(t["resp"], n, 3), "x25519": stats(t["x25519"], n, 1)}
    out["note"] = ("stream events around one call each (finish = memset + finish kernel + commit kernel), medians of 7 "
                   "repetitions after one warm-up round; one initiator with 8 peer rows, every row towards the same "
                   "responder, fresh ephemeral keys per row; the responder calls run on these handshakes' own "
                   "messages in the same run; ms_per_ladder = the call's time / its X25519 ladders per row")
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                        "handshake_initiator_bench.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


def peerstate_leg(eng):
    """The device-resident peer handshake state at 64 Ki and 1 Ki rows, by stream events, medians of seven with
    min-max, all in one run: the responder chain (init -> ts -> cookies -> resp -> mac1) against init + resp alone
    on the same messages, the initiator chain (cookies -> initiate -> mac1) against initiate alone, and each new
    call alone (ts with all rows on one peer and with every row on a peer of its own).  Every row carries the same
    timestamp, which passes (equal to latest), so every call does its whole work in every repetition.  Written to
    profiles/peerstate_bench.json."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tests"))
    import handshake_cases as hc  # the Python model makes the valid messages
    import peerstate_cases as pc

    r = hc.Responder(53, npeers=8, neph=256)
    rng = np.random.default_rng(59)
    rb = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    z = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype, device="cuda")  # noqa: E731
    stamp = hc.tai64n(1_800_000_000, 7)
    base = np.zeros((256, 160), np.uint8)
    for i in range(256):
        base[i, :148] = np.frombuffer(hc.make_initiation(r.sk_i[i % 8], r.pk_r, r.esk_i[i], stamp, i)[0], np.uint8)
    peers = hc.peer_rows(r.peers)
    d_own, d_peers, d_table = dev(r.own), dev(peers), dev(aead.peer_table(peers))
    # the initiator of the second chain: 8 peer rows, dealt round robin
    sk_a = rb(32)
    a_own = dev(np.frombuffer(sk_a + hc.pubkey(sk_a), np.uint8))
    # 256 valid cookie messages over the 8 peers, each under its peer's recorded mac1
    ckeys = [pc.cookie_key(p[0]) for p in r.peers]
    state8 = [pc.state_row(mac1=rb(16)) for _ in range(8)]
    ids = np.arange(256, dtype=np.uint32) + 0x7000_0000
    cmsg = np.frombuffer(b"".join(pc.cookie_message(int(ids[i]), rb(24), ckeys[i % 8], state8[i % 8][32:48], rb(16))
                                  for i in range(256)), np.uint8).reshape(256, 64)
    d_ckeys = dev(np.frombuffer(b"".join(ckeys), np.uint8))
    d_sess = dev(aead.rx_table(ids, (np.arange(256) % 8).astype(np.uint32)))

    def ev_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def stats(ts, n):
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        return {"ms_median": round(med, 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4),
                "per_s_median": round(n / med * 1e3)}

    out = {}
    for n in (1 << 16, 1 << 10):
        buf = dev(np.tile(base, (n // 256, 1)).reshape(-1))
        desc = np.zeros(n, DESC_DTYPE)
        desc["offset"], desc["len"] = np.arange(n, dtype=np.uint64) * 160, 148
        d_desc = dev(desc.view(np.uint8).reshape(-1, 16))
        cdesc = np.zeros(n, DESC_DTYPE)
        cdesc["offset"], cdesc["len"] = np.arange(n, dtype=np.uint64) * 64, 64
        d_cdesc, d_cbuf = dev(cdesc.view(np.uint8).reshape(-1, 16)), dev(np.tile(cmsg, (n // 256, 1)).reshape(-1))
        state, claim = dev(pc.rows_array(state8, 64)), z(8, dtype=torch.int32)
        res, st, st2, po = z(n, 128), z(n), z(n), z(n, dtype=torch.int32)
        esk, sids = dev(rng.integers(0, 256, (n, 32), dtype=np.uint8)), dev(np.arange(n, dtype=np.uint32))
        resp, keys, cookies, has = z(n, 96), z(n, 64), z(n, 16), z(n)
        ws = eng.peer_ts_workspace(n, 8)
        ini = lambda: eng.handshake_init_dev(d_own, d_peers, d_table, d_desc, None, buf, res, st)  # noqa: E731
        rsp0 = lambda: eng.handshake_resp_dev(d_peers, res, None, esk, sids, None, None, resp, keys, st2)  # noqa: E731
        tsc = lambda: eng.peer_ts_dev(state, res, st, po, workspace=ws)  # noqa: E731
        gat = lambda: eng.peer_cookies_dev(state, po, cookies, has)  # noqa: E731
        rsp = lambda: eng.handshake_resp_dev(d_peers, res, st, esk, sids, cookies, has, resp, keys, st2)  # noqa: E731
        rec = lambda: eng.peer_mac1_dev(state, po, st2, resp, 96, 60, claim)  # noqa: E731
        chain = lambda: (ini(), tsc(), gat(), rsp(), rec())  # noqa: E731
        # the initiator's side
        pidx, tss = dev((np.arange(n) % 8).astype(np.uint32)), dev(np.tile(np.frombuffer(stamp, np.uint8), (n, 1)))
        msgs, pending, st3 = z(n, 160), z(n, 128), z(n)
        gat_i = lambda: eng.peer_cookies_dev(state, pidx, cookies, has)  # noqa: E731
        init0 = lambda: eng.handshake_initiate_dev(a_own, d_peers, pidx, None, esk, tss, sids, None, None, msgs,  # noqa: E731
                                                   pending, st3)
        init = lambda: eng.handshake_initiate_dev(a_own, d_peers, pidx, None, esk, tss, sids, cookies, has, msgs,  # noqa: E731
                                                  pending, st3)
        rec_i = lambda: eng.peer_mac1_dev(state, pidx, st3, msgs, 160, 116, claim)  # noqa: E731
        chain_i = lambda: (gat_i(), init(), rec_i())  # noqa: E731
        # each call alone; ts on crafted rows: one peer, and a peer per row
        one = dev(pc.rows_array([pc.result_row(stamp, 0)], 128)).repeat(n, 1)
        many = one.clone()
        many[:, 108:112] = dev(np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4))
        st_ok, po2, state_n, ws_n = z(n), z(n, dtype=torch.int32), z(n, 64), eng.peer_ts_workspace(n, n)
        ts_one = lambda: eng.peer_ts_dev(state, one, st_ok, po2, workspace=ws)  # noqa: E731
        ts_many = lambda: eng.peer_ts_dev(state_n, many, st_ok, po2, workspace=ws_n)  # noqa: E731
        got_ck, st4 = z(n, 16), z(n)
        state_c = dev(pc.rows_array(state8, 64))  # a table of its own: the chains' mac1 calls rewrite the AAD
        con = lambda: eng.peer_cookie_consume_dev(state_c, d_ckeys, d_sess, d_cdesc, None, d_cbuf, got_ck, claim, st4)  # noqa: E731
        chain(), chain_i(), ts_one(), ts_many()
        torch.cuda.synchronize()
        assert (st == aead.PKT_OK).all().item() and (st2 == aead.PKT_OK).all().item() and (st3 == aead.PKT_OK).all().item()
        assert (st_ok == aead.PKT_OK).all().item() and torch.equal(po2.cpu(), torch.arange(n, dtype=torch.int32))
        con()
        torch.cuda.synchronize()
        assert (st4 == aead.PKT_OK).all().item()
        t = {k: [] for k in ("init_resp", "responder_chain", "initiate", "initiator_chain", "ts_one_peer",
                             "ts_peer_per_row", "ts_8_peers_in_chain", "cookies", "mac1_resp", "mac1_init", "consume")}
        for _ in range(7):
            t["init_resp"].append(ev_ms(lambda: (ini(), rsp0())))
            t["responder_chain"].append(ev_ms(chain))
            t["initiate"].append(ev_ms(init0))
            t["initiator_chain"].append(ev_ms(chain_i))
            ini()
            torch.cuda.synchronize()
            t["ts_8_peers_in_chain"].append(ev_ms(tsc))
            t["ts_one_peer"].append(ev_ms(ts_one))
            t["ts_peer_per_row"].append(ev_ms(ts_many))
            t["cookies"].append(ev_ms(gat_i))
            t["mac1_resp"].append(ev_ms(rec))
            t["mac1_init"].append(ev_ms(rec_i))
            t["consume"].append(ev_ms(con))
        assert (st2 == aead.PKT_OK).all().item() and (st4 == aead.PKT_OK).all().item()
        row = {k: stats(v, n) for k, v in t.items()}
        row["responder_chain_extra_ms"] = round(row["responder_chain"]["ms_median"] - row["init_resp"]["ms_median"], 4)
        row["initiator_chain_extra_ms"] = round(row["initiator_chain"]["ms_median"] - row["initiate"]["ms_median"], 4)
        out[f"rows_{n}"] = row
    out["note"] = ("stream events around each sequence of calls, medians of 7 repetitions after one warm-up round; rows "
                   "are 256 distinct valid initiations over 8 peers, tiled, all with one timestamp (equal passes: no "
                   "row is turned down); responder_chain = init + ts + cookies + resp + mac1, init_resp = init + resp; "
                   "initiator_chain = cookies + initiate + mac1; ts = prep + the radix passes the peer count needs "
                   "(none for one peer, 1 for 8, 2 for 1 Ki and for 64 Ki) + reduce + carry + verdict + advance; "
                   "consume = memset + open + commit over 8 peers; mac1 = memset + claim + commit")
    with open(os.path.join(root, "profiles", "peerstate_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


def session_leg(eng):
    """The device-resident session table, medians of seven with min-max by stream events and by host wall clock (a
    device sync behind the call), all in one run.  Tables of 64 Ki and 1 Mi rows with every other row live; 1 Ki
    and 64 Ki handshakes with fresh ids over 256 peers (into the 64 Ki table only 32 Ki rows are free: the rest
    is RG_PKT_FULL, which is part of what is timed).  The table is put back from a saved copy between
    repetitions, outside the timed region.  The host path is timed for 1 Ki handshakes into the 64 Ki table
    alone: rg_sessions_insert_peer searches the table for a free row from the start, which takes minutes to fill
    half of a 1 Mi table.  Written to profiles/session_install_bench.json."""
    import ctypes
    import time

    from rustyguard_amd import session

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(61)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    words = lambda a: dev(np.asarray(a, np.uint32).view(np.int32))  # noqa: E731
    npeers = 256

    def measure(fn, reset):
        ev, wall = [], []
        for _ in range(8):  # the first is the warm-up
            reset()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(a.elapsed_time(b))
        st = lambda ts: {"ms_median": round(sorted(ts)[len(ts) // 2], 4), "ms_min": round(min(ts), 4),  # noqa: E731
                         "ms_max": round(max(ts), 4)}
        return {"gpu": st(ev[1:]), "wall": st(wall[1:])}

    out = {}
    for nkeys in (1 << 16, 1 << 20):
        T = session.SessionTables(eng, nkeys, npeers)
        live = np.arange(nkeys) % 2 == 0
        T.slot_peer[:] = words(np.where(live, np.arange(nkeys) % npeers, 0xFFFFFFFF))
        T.local_ids[:] = words(np.where(live, np.arange(nkeys) + 0x4000_0000, 0))
        T.send_keys[:] = dev(rng.integers(0, 256, (nkeys, 32), dtype=np.uint8))
        started = np.zeros((nkeys, 3), np.uint64)
        started[:, 1] = np.where(np.arange(nkeys) % 10 == 0, 5, 10**12)  # every fifth live row is old: 10 % of the rows
        T.send_state[:] = dev(started.view(np.uint8).reshape(nkeys, 24))
        session.index_dev(eng, T)
        saved = {name: getattr(T, name).clone() for name in session.ARRAYS}

        def reset():
            for name in session.ARRAYS:
                getattr(T, name).copy_(saved[name])

        d_now = dev(np.array([10**12], np.int64))
        expired = torch.zeros(nkeys, dtype=torch.uint8, device="cuda")
        row = {}
        for n in (1 << 10, 1 << 16):
            lids, rids = words(np.arange(n) + 0x7000_0000), words(np.arange(n) + 0x0100_0000)
            peers, key_rows = words(np.arange(n) % npeers), dev(rng.integers(0, 256, (n, 64), dtype=np.uint8))
            keys, st = key_rows.clone(), torch.zeros(n, dtype=torch.uint8, device="cuda")
            rows_out = torch.zeros(n, dtype=torch.int32, device="cuda")
            ws = session.session_workspace(eng, n, nkeys, npeers)

            def reset_n():
                reset()
                keys.copy_(key_rows)

            row[f"install_{n}"] = measure(lambda: session.install_batch_dev(eng, T, None, lids, rids, peers, keys, st,
                                                                            rows_out, now_ns=d_now, workspace=ws), reset_n)
            want_ok = min(n, nkeys // 2)
            assert int((st == aead.PKT_OK).sum()) == want_ok and int((st == session.PKT_FULL).sum()) == n - want_ok
        ws = session.session_workspace(eng, 0, nkeys, npeers)
        row["expire_10_percent"] = measure(lambda: session.expire_batch_dev(eng, T, d_now, None, expired, workspace=ws), reset)
        assert int(expired.sum()) == (nkeys + 9) // 10
        row["rebuild"] = measure(lambda: session.index_dev(eng, T), reset)
        out[f"table_{nkeys}"] = row

    # what a caller does today: 1 Ki handshakes into a half-full host table of 64 Ki rows
    n, nkeys = 1 << 10, 1 << 16
    L = eng.library
    S = aead.Sessions(eng, nkeys)
    zero = (ctypes.c_uint8 * 32)()
    for r in range(nkeys // 2):
        L.rg_sessions_insert_peer(S._h, 0x4000_0000 + r, r, zero, zero, r % npeers)
    d_keys, d_ids = dev(rng.integers(0, 256, (n, 64), dtype=np.uint8)), words(np.arange(3 * n))
    h_keys = torch.zeros((n, 64), dtype=torch.uint8).pin_memory()
    h_ids = torch.zeros(3 * n, dtype=torch.int32).pin_memory()
    fdesc = dev(np.array([(0, 32, 0)], DESC_DTYPE).view(np.uint8).reshape(-1, 16))
    fbuf, fst = torch.zeros(64, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.uint8, device="cuda")
    slots = []

    def host_path():
        h_keys.copy_(d_keys, non_blocking=True)
        h_ids.copy_(d_ids, non_blocking=True)
        torch.cuda.synchronize()
        base, ids = h_keys.data_ptr(), h_ids.numpy().view(np.uint32)
        slots[:] = [L.rg_sessions_insert_peer(S._h, 0x7000_0000 + i, int(ids[n + i]), ctypes.c_void_p(base + 64 * i),
                                              ctypes.c_void_p(base + 64 * i + 32), i % npeers) for i in range(n)]
        S.send_batch_dev([slots[0]], fdesc, fbuf, fst)  # the next device call uploads the mirrors

    def host_reset():
        for r in slots:
            L.rg_sessions_remove(S._h, r)
        slots.clear()

    out["host_path_1024_into_65536"] = measure(host_path, host_reset)
    assert min(slots) >= 0
    out["note"] = ("medians of 7 repetitions after one warm-up; gpu = stream events around the call, wall = host clock "
                   "with a device sync behind it; tables half full (every other row live), handshakes with fresh ids "
                   "over 256 peers; install = 4 memsets + prep + judge + carry + rank + free_count + carry + free_compact "
                   "+ commit + peer_commit + the rebuild; expire = the expiry kernel + the rebuild; rebuild = memset + "
                   "index kernel; host_path = keys and ids to pinned memory, rg_sessions_insert_peer per row from "
                   "Python through ctypes, and a one-packet rg_send_batch_dev, whose mirror refresh uploads the table")
    with open(os.path.join(root, "profiles", "session_install_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


def timers_leg(eng):
    """The device-resident session timers by stream events, medians of seven with min-max, all in one run.  Every
    row of the table is live, four rows per peer, the peer's current row its last; a due row is pending, silent
    and carries a fired rekey entry on a session past REKEY_AFTER_TIME.  The timers and the send state are put back
    from a saved copy between repetitions, outside the timed region.  Written to profiles/timers_bench.json."""
    from rustyguard_amd import session, timers

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(71)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    words = lambda a: dev(np.asarray(a, np.uint32).view(np.int32))  # noqa: E731
    now = 10**12
    d_now = dev(np.array([now], np.int64))

    def measure(fn, reset):
        ev = []
        for _ in range(8):  # the first is the warm-up
            reset()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ev.append(a.elapsed_time(b))
        ts = sorted(ev[1:])
        return {"ms_median": round(ts[len(ts) // 2], 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4)}

    out = {}
    for nkeys in (1 << 16, 1 << 20):
        npeers = nkeys // 4
        T = session.SessionTables(eng, nkeys, npeers)
        r = np.arange(nkeys)
        T.slot_peer[:] = words(r % npeers)
        T.peer_slot[:] = words(np.arange(npeers) + nkeys - npeers)
        T.send_keys[:] = dev(rng.integers(0, 256, (nkeys, 32), dtype=np.uint8))
        T.receivers[:] = words(r + 0x0100_0000)
        T.local_ids[:] = words(r + 0x4000_0000)  # distinct ids: the rebuild behind the expiry probes a few entries
        session.index_dev(eng, T)
        tm = timers.timer_rows(eng, nkeys)
        ka, rk = (torch.zeros(npeers, dtype=torch.int32, device="cuda") for _ in range(2))
        gate, counts = torch.zeros(npeers, dtype=torch.uint8, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
        expired = torch.zeros(nkeys, dtype=torch.uint8, device="cuda")
        ws_t, ws_x = timers.timer_workspace(eng, nkeys, npeers), session.session_workspace(eng, 0, nkeys, npeers)
        desc = dev(np.array([(32 * k, 0, 0) for k in range(npeers)], DESC_DTYPE).view(np.uint8).reshape(-1, 16))
        buf, st = torch.zeros(32 * npeers, dtype=torch.uint8, device="cuda"), torch.zeros(npeers, dtype=torch.uint8, device="cuda")
        ws_s = eng.send_workspace(npeers, nkeys)
        row = {"npeers": npeers}
        for label, share in (("1_percent", 0.01), ("50_percent", 0.5)):
            due = rng.random(nkeys) < share
            state = np.zeros((nkeys, 3), np.uint64)
            state[:, 0] = 3
            state[:, 1] = np.where(due, now - 120 * 10**9 - 9, now - 9)
            state[:, 2] = np.where(due, now - 10 * 10**9 - 9, now - 9)
            rows_tm = np.zeros((nkeys, 2), np.uint64)
            rows_tm[:, 0] = np.where(due, now - 1, now + 120 * 10**9)
            rows_tm[:, 1] = due
            saved_state, saved_tm = dev(state.view(np.uint8).reshape(nkeys, 24)), dev(rows_tm.view(np.uint8).reshape(nkeys, 16))

            def reset():
                T.send_state.copy_(saved_state)
                tm.copy_(saved_tm)

            turn = lambda: timers.turn_dev(eng, T, tm, d_now, ka, rk, gate, counts, workspace=ws_t)  # noqa: E731
            res = {"turn": measure(turn, reset)}
            nka, nrk = (int(x) for x in counts.cpu().numpy().view(np.uint32))
            peers_due = int(np.bincount(r[due] % npeers, minlength=npeers).astype(bool).sum())
            assert nka == nrk == peers_due, (nka, nrk, peers_due)
            res["rows_due"], res["keepalives"], res["rekeys"] = int(due.sum()), nka, nrk
            res["expire_none_due"] = measure(lambda: session.expire_batch_dev(eng, T, d_now, None, expired, workspace=ws_x),
                                             reset)
            assert int(expired.sum()) == 0
            reset()
            turn()
            slots = ka.clone()  # the padded list: nka rows, then RG_KEY_SKIP
            send = lambda m: eng.send_batch_dev_resident(T.send_keys, T.receivers, T.send_state, slots[:m], desc[:m],  # noqa: E731
                                                         buf, st[:m], now_ns=d_now, workspace=ws_s)
            res["keepalive_send_padded"] = measure(lambda: send(npeers), reset)
            assert int((st == aead.PKT_OK).sum()) == nka
            res["keepalive_send_due_only"] = measure(lambda: send(nka), reset)
            assert int((st[:nka] == aead.PKT_OK).sum()) == nka
            res["padded_send_over_turn"] = round(res["keepalive_send_padded"]["ms_median"] / res["turn"]["ms_median"], 2)
            row[label] = res
        if nkeys == 1 << 16:
            n = 1 << 16
            hit = words(rng.integers(0, nkeys, n))
            ok, one = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.ones(n, dtype=torch.uint8, device="cuda")
            row["arm_65536"] = measure(lambda: timers.arm_batch_dev(eng, tm, hit, ok, d_now, 120 * 10**9), reset)
            row["note_send_65536"] = measure(lambda: timers.note_send_batch_dev(eng, tm, hit, ok, one, d_now), reset)
            row["note_recv_65536"] = measure(lambda: timers.note_recv_batch_dev(eng, tm, T.send_state, hit, ok, d_now), reset)
        out[f"table_{nkeys}"] = row
    out["note"] = ("stream events around one call each, medians of 7 repetitions after one warm-up; every row live, four "
                   "rows per peer; turn = clear + row + count + carry + compact kernels; expire = the expiry kernel + the "
                   "receiver-table rebuild, no row leaving; keepalive sends of 32-byte frames, padded = n = npeers with "
                   "RG_KEY_SKIP behind the due rows, due_only = n = the turn's count; the note and arm calls hit random "
                   "rows of the 64 Ki table with every packet eligible")
    with open(os.path.join(root, "profiles", "timers_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


def pending_leg(eng):
    """The device-resident pending handshakes by stream events, medians of seven with min-max, all in one run, at
    16 Ki and 256 Ki peers with about 1 % and about 50 % of the rows due for a retry.  Every row of the pending table
    is live; a due row was last sent REKEY_TIMEOUT and 9 ns ago.  Beside rg_pending_turn_dev, the install of the
    chain's rows (n = npeers, the turn's gate) and the table rebuild alone: rg_timer_turn_dev over a transport table
    of four rows per peer with the same share due, and the bare initiator chain (cookies -> initiate -> mac1,
    n = npeers) over the turn's list.  Tables and batch are put back from saved copies between repetitions, outside
    the timed region.  Written to profiles/pending_bench.json."""
    from rustyguard_amd import pending, session, timers

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(73)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    words = lambda a: dev(np.asarray(a, np.uint32).view(np.int32))  # noqa: E731
    z = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype, device="cuda")  # noqa: E731
    now = 10**12
    d_now = dev(np.array([now], np.int64))
    sk_a = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    a_own = dev(np.frombuffer(sk_a + bytes(32), np.uint8))  # the initiate reads the private half and its own public key

    def measure(fn, reset):
        ev = []
        for _ in range(8):  # the first is the warm-up
            reset()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ev.append(a.elapsed_time(b))
        ts = sorted(ev[1:])
        return {"ms_median": round(ts[len(ts) // 2], 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4)}

    out = {}
    for npeers in (1 << 14, 1 << 18):
        nkeys = 4 * npeers
        P = pending.PendingTables(eng, npeers)
        rows = rng.integers(0, 256, (npeers, 128), dtype=np.uint8)
        rows.view(np.uint32).reshape(npeers, 32)[:, pending.PEER_WORD] = np.arange(npeers)
        rows.view(np.uint32).reshape(npeers, 32)[:, pending.SENDER_WORD] = np.arange(npeers) + 0x4000_0000
        saved_rows = dev(rows)
        a_peers, state = dev(rng.integers(0, 256, (npeers, 96), dtype=np.uint8)), z(npeers, 64)
        init, gate, expired, counts = z(npeers, dtype=torch.int32), z(npeers), z(npeers), z(2, dtype=torch.int32)
        ws = pending.pending_workspace(eng, npeers, npeers, npeers)
        esk, sids = dev(rng.integers(0, 256, (npeers, 32), dtype=np.uint8)), words(np.arange(npeers) + 0x5000_0000)
        tss = dev(np.tile(np.frombuffer(bytes(12), np.uint8), (npeers, 1)))
        cookies, has, claim = z(npeers, 16), z(npeers), z(npeers, dtype=torch.int32)
        msgs, batch, st_i, st_p = z(npeers, 160), z(npeers, 128), z(npeers), z(npeers)
        installed = z(npeers, dtype=torch.int32)
        # the transport table beside it: the timers leg's, four rows per peer
        T, tm = session.SessionTables(eng, nkeys, npeers), timers.timer_rows(eng, nkeys)
        r = np.arange(nkeys)
        T.slot_peer[:] = words(r % npeers)
        T.peer_slot[:] = words(np.arange(npeers) + nkeys - npeers)
        ka, rk, rk_gate, rk_counts = z(npeers, dtype=torch.int32), z(npeers, dtype=torch.int32), z(npeers), z(2, dtype=torch.int32)
        ws_t = timers.timer_workspace(eng, nkeys, npeers)
        row = {"nkeys_of_the_timer_turn": nkeys}
        for label, share in (("1_percent", 0.01), ("50_percent", 0.5)):
            due = rng.random(npeers) < share
            tmr = np.zeros((npeers, 2), np.uint64)
            tmr[:, 0] = tmr[:, 1] = np.where(due, now - 5 * 10**9 - 9, now - 1)
            saved_tm = dev(tmr.view(np.uint8).reshape(npeers, 16))
            due_k = rng.random(nkeys) < share
            state_k = np.zeros((nkeys, 3), np.uint64)
            state_k[:, 0] = 3
            state_k[:, 1] = np.where(due_k, now - 120 * 10**9 - 9, now - 9)
            state_k[:, 2] = np.where(due_k, now - 10 * 10**9 - 9, now - 9)
            tm_k = np.zeros((nkeys, 2), np.uint64)
            tm_k[:, 0] = np.where(due_k, now - 1, now + 120 * 10**9)
            tm_k[:, 1] = due_k
            saved_state_k, saved_tm_k = dev(state_k.view(np.uint8).reshape(nkeys, 24)), dev(tm_k.view(np.uint8).reshape(nkeys, 16))
            saved_batch = batch.clone()

            def reset():
                P.pending.copy_(saved_rows)
                P.timers.copy_(saved_tm)
                batch.copy_(saved_batch)
                T.send_state.copy_(saved_state_k)
                tm.copy_(saved_tm_k)

            turn = lambda: pending.turn_dev(eng, P, d_now, init, gate, counts, expired_out=expired, workspace=ws)  # noqa: E731
            res = {"pending_turn": measure(turn, reset)}
            k, nexp = (int(x) for x in counts.cpu().numpy().view(np.uint32))
            assert k == int(due.sum()) and nexp == 0, (k, nexp, int(due.sum()))
            res["rows_due"] = k
            # the same turn fed the timer turn's rekey list as requests: every row is live, so none is added
            res["timer_turn"] = measure(lambda: timers.turn_dev(eng, T, tm, d_now, ka, rk, rk_gate, rk_counts, workspace=ws_t),
                                        reset)
            res["rekeys_listed"] = int(rk_counts.cpu().numpy().view(np.uint32)[1])
            res["pending_turn_with_requests"] = measure(
                lambda: pending.turn_dev(eng, P, d_now, init, gate, counts, start_peers=rk, start_status=rk_gate,
                                         start_match=aead.PKT_OK, expired_out=expired, workspace=ws), reset)
            assert int(counts.cpu().numpy().view(np.uint32)[0]) == k
            chain = lambda: (eng.peer_cookies_dev(state, init, cookies, has),  # noqa: E731
                             eng.handshake_initiate_dev(a_own, a_peers, init, gate, esk, tss, sids, cookies, has, msgs,
                                                        batch, st_i),
                             eng.peer_mac1_dev(state, init, st_i, msgs, 160, 116, claim))
            res["initiator_chain"] = measure(chain, lambda: None)
            assert int((st_i == aead.PKT_OK).sum()) == k
            saved_batch = batch.clone()  # the chain's rows: what the install consumes
            res["pending_install"] = measure(
                lambda: pending.install_dev(eng, P, batch, st_i, d_now, st_p, installed, workspace=ws), reset)
            assert int((st_p == aead.PKT_OK).sum()) == k and int((installed != -1).sum()) == k
            res["pending_index"] = measure(lambda: pending.index_dev(eng, P), reset)
            row[label] = res
        out[f"peers_{npeers}"] = row
    out["note"] = ("stream events around one call each, medians of 7 repetitions after one warm-up; every pending row "
                   "live, a due row last sent 5 s + 9 ns ago; pending_turn = clear + row + count + carry + rank + index "
                   "kernels (with requests: + the request kernel, m = npeers); pending_install = clear + claim + commit "
                   "+ wipe + index kernels, n = npeers behind the chain's statuses; pending_index = fill + index; "
                   "timer_turn over four transport rows per peer with the same share due; initiator_chain = cookies -> "
                   "initiate -> mac1 with n = npeers over the pending turn's list and gate")
    with open(os.path.join(root, "profiles", "pending_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


def ratelimit_leg(eng):
    """The device-resident handshake rate limiter by stream events, medians of seven with min-max, all in one run, on
    the default sketch (5437 x 5): rg_rate_count_batch_dev at 1 Ki and 64 Ki valid initiations from 1, 256 and 20 000
    distinct source addresses (dealt round-robin), from an empty sketch each time; rg_cookie_reply_batch_dev on the
    same batch beside it, fed the count's flags and all overloaded; the count of the same 320 Ki items with two, one
    and no radix pass (where its time goes); and rg_rate_turn_dev with and without a reset.  The sketch is put back between repetitions, outside the timed region.  Written to
    profiles/ratelimit_bench.json."""
    from rustyguard_amd import ratelimit

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(97)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    z = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype, device="cuda")  # noqa: E731
    L = 148

    def measure(fn, reset):
        ev = []
        for _ in range(8):  # the first is the warm-up
            reset()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ev.append(a.elapsed_time(b))
        ts = sorted(ev[1:])
        return {"ms_median": round(ts[len(ts) // 2], 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4)}

    T = ratelimit.RateTables(eng)
    seeds = dev(rng.integers(0, 256, (T.depth, 16), dtype=np.uint8))
    new_seeds = dev(rng.integers(0, 256, (T.depth, 16), dtype=np.uint8))
    ck = rng.integers(0, 256, 96, dtype=np.uint8)
    keys, mac1_key = dev(ck), ck[:32].tobytes()

    def empty():
        T.buckets.zero_()
        T.seeds.copy_(seeds)

    out = {"width": T.width, "depth": T.depth, "limit": ratelimit.RATE_LIMIT}
    for n in (1 << 10, 1 << 16):
        host = rng.integers(0, 256, (n, 160), dtype=np.uint8)
        host[:, 0:4] = (1, 0, 0, 0)  # HandshakeInit
        host[:, L - 16:L] = 0        # no mac2
        for row in host:             # a valid mac1: an overloaded message takes the filter's whole path
            row[L - 32:L - 16] = np.frombuffer(
                hashlib.blake2s(row[:L - 32].tobytes(), key=mac1_key, digest_size=16).digest(), np.uint8)
        desc = np.zeros(n, DESC_DTYPE)
        desc["offset"], desc["len"] = np.arange(n, dtype=np.uint64) * 160, L
        buf, d = dev(host.reshape(-1)), dev(desc.view(np.uint8).reshape(-1, 16))
        nonces = dev(rng.integers(0, 256, (n, 24), dtype=np.uint8))
        replies, st, flags, counts = z(n, 64), z(n), z(n), z(n, dtype=torch.int32)
        ws = ratelimit.rate_workspace(eng, n)
        row = {}
        for sources in (1, 256, 20000):
            pool = np.zeros((sources, 24), np.uint8)
            pool[:, 0] = 10
            pool[:, 1:4] = (np.arange(sources)[:, None] >> (16, 8, 0)) & 255  # 10.x.y.z
            addrs = dev(pool[np.arange(n) % sources])
            count = lambda: ratelimit.count_dev(eng, T, d, addrs, buf, flags, counts, workspace=ws)  # noqa: E731
            res = {"rate_count": measure(count, empty)}
            over = int(flags.sum())
            true_over = sum(max(0, (n - s + sources - 1) // sources - ratelimit.RATE_LIMIT) for s in range(min(sources, n)))
            assert over >= true_over  # a count-min estimate is never below the true count
            res["messages_over_the_limit"], res["by_their_true_counts"] = over, true_over
            res["cookie_reply_with_the_flags"] = measure(
                lambda: eng.cookie_reply_dev(keys, d, addrs, flags, nonces, buf, replies, st), lambda: None)
            assert int((st == aead.PKT_COOKIE).sum()) == over and int((st == aead.PKT_OK).sum()) == n - over
            res["cookie_reply_all_overloaded"] = measure(
                lambda: eng.cookie_reply_dev(keys, d, addrs, None, nonces, buf, replies, st), lambda: None)
            row[f"sources_{sources}"] = res
        out[f"messages_{n}"] = row
    # Where the count's time goes: the same 320 Ki items (64 Ki messages x 5, the last batch above) grouped with
    # two radix passes (the default sketch), one (51 x 5 = 255 buckets) and none (one bucket: 320 Ki messages on a
    # 1 x 1 sketch, descriptors and addresses repeated); the kernels around the passes are the same in all three.
    n, split = 1 << 16, {}
    for label, width, depth, reps in (("two_radix_passes_5437x5", T.width, T.depth, 1), ("one_radix_pass_51x5", 51, 5, 1),
                                      ("no_radix_pass_1x1", 1, 1, 5)):
        S = ratelimit.RateTables(eng, width, depth)
        S.seeds.copy_(seeds[:depth])
        m = n * reps
        d_m, addrs_m, flags_m = d.repeat(reps, 1), addrs.repeat(reps, 1), z(m)
        ws_m = ratelimit.rate_workspace(eng, m, width, depth)
        assert m * depth == n * T.depth
        split[label] = measure(lambda: ratelimit.count_dev(eng, S, d_m, addrs_m, buf, flags_m, workspace=ws_m),
                               lambda: S.buckets.zero_())
    out["where_the_time_goes_320Ki_items"] = split
    d_now, reset_out = dev(np.array([10**12], np.int64)), z(1, dtype=torch.int32)
    turn = lambda: ratelimit.turn_dev(eng, T, d_now, new_seeds, reset_out)  # noqa: E731
    out["rate_turn_with_reset"] = measure(turn, lambda: T.last_reset_ns.zero_())
    assert int(reset_out[0]) == 1
    out["rate_turn_without_reset"] = measure(turn, lambda: None)
    assert int(reset_out[0]) == 0
    out["note"] = ("stream events around one call each, medians of 7 repetitions after one warm-up; rate_count = key + "
                   "2 x (hist + scan + scatter) + reduce + carry + verdict + finish kernels over n * depth items from an "
                   "empty sketch; the sources are dealt round-robin; cookie_reply = rg_cookie_reply_batch_dev on the "
                   "same batch (valid mac1, no mac2) with overload = the count's flags and with overload = NULL; "
                   "rate_turn = decide + wipe kernels")
    with open(os.path.join(root, "profiles", "ratelimit_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


def endpoint_leg(eng):
    """The device-resident peer endpoints on the replay and send legs' two workloads (cfg2: 64 Ki x 1500 B on one
    session; cfg4: 256 sessions x 4 Ki x 1500 B interleaved) and on 1 Ki packets of one session (the launch floor),
    peer = session, all in one run: (a) the resident receive + rg_timer_note_recv_batch_dev, (b) the same with
    rg_endpoint_note_recv_batch_dev, (c) the resident send, (d) rg_endpoint_gate_batch_dev + the resident send, (e)
    the note, the gate and rg_timer_note_recv_batch_dev each alone on the same batch -- by stream events, medians of
    seven with min-max -- and, by host wall clock, what a caller does today behind the same receive: status and
    key_idx_out to pinned memory, a stream synchronise and a vectorised numpy last-per-peer.  Written to
    profiles/endpoint_bench.json."""
    import time

    from rustyguard_amd import endpoint, timers

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(83)
    T0 = 10**12
    d_now = torch.from_numpy(np.array([T0], np.int64)).cuda()

    def shape(w):
        n, nk = w.n, len(w.receivers)
        b = DeviceBatch(eng, w)
        b.fill()
        plain = b.buf.clone()
        b.seal()
        sealed = b.buf.clone()
        table = torch.from_numpy(aead.rx_table(w.receivers, np.arange(nk, dtype=np.uint32))).cuda()
        ws_r, ws_s = eng.replay_workspace(n, nk), eng.send_workspace(n, nk)
        win = torch.zeros(nk * 33, dtype=torch.int64, device="cuda")
        state = torch.zeros(nk * 3, dtype=torch.int64, device="cuda")
        tm = timers.timer_rows(eng, nk)
        host_slot_peer = np.arange(nk, dtype=np.uint32)  # peer = session
        slot_peer = torch.from_numpy(host_slot_peer.view(np.int32).copy()).cuda()
        E = endpoint.EndpointTable(eng, nk)
        host_src = np.zeros((n, 24), np.uint8)
        host_src[:, :18] = rng.integers(0, 256, (n, 18), dtype=np.uint8)
        src = torch.from_numpy(host_src).cuda()
        key_idx = torch.zeros(n, dtype=torch.int32, device="cuda")
        slots = torch.from_numpy(np.ascontiguousarray(w.desc["key_idx"], np.uint32).view(np.int32).copy()).cuda()
        slots_out, dst = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros((n, 24), dtype=torch.uint8, device="cuda")
        st_send = torch.zeros(n, dtype=torch.uint8, device="cuda")
        pin_st, pin_k = torch.empty(n, dtype=torch.uint8).pin_memory(), torch.empty(n, dtype=torch.int32).pin_memory()
        host_ep = np.zeros((nk, 24), np.uint8)

        def recv():
            eng.recv_batch_dev_resident(b.keys, table, win, b.desc_open, b.buf, b.status, key_idx_out=key_idx,
                                        workspace=ws_r)

        def timer_note():
            timers.note_recv_batch_dev(eng, tm, state, key_idx, b.status, d_now)

        def ep_note():
            E.note_recv_batch_dev(slot_peer, key_idx, b.status[:n], src)

        def gate():
            E.gate_batch_dev(slot_peer, slots, slots_out, dst)

        def send(sl):
            eng.send_batch_dev_resident(b.keys, b.receivers, state, sl, b.desc_seal, b.buf, st_send, workspace=ws_s)

        def today():
            recv()
            pin_st.copy_(b.status[:n], non_blocking=True)
            pin_k.copy_(key_idx, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            idx = np.nonzero(pin_st.numpy() == 0)[0]
            last = np.full(nk, -1, np.int64)
            last[host_slot_peer[pin_k.numpy().view(np.uint32)[idx]]] = idx  # repeated peers: the last index stays
            moved = last >= 0
            host_ep[moved] = host_src[last[moved]]

        def restore_recv():
            b.buf.copy_(sealed)
            win.zero_()
            tm.zero_()
            torch.cuda.synchronize()

        def restore_send():
            b.buf.copy_(plain)
            state.zero_()
            torch.cuda.synchronize()

        def gpu_ms(fn):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            z.record()
            torch.cuda.synchronize()
            return a.elapsed_time(z)

        def wall_ms(fn):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        legs = (("a_recv_timer_note_gpu_ms", restore_recv, gpu_ms, lambda: (recv(), timer_note())),
                ("b_recv_timer_note_endpoint_note_gpu_ms", restore_recv, gpu_ms, lambda: (recv(), timer_note(), ep_note())),
                ("c_send_gpu_ms", restore_send, gpu_ms, lambda: send(slots)),
                ("d_gate_send_gpu_ms", restore_send, gpu_ms, lambda: (gate(), send(slots_out))),
                ("e_endpoint_note_alone_gpu_ms", lambda: None, gpu_ms, ep_note),
                ("e_endpoint_gate_alone_gpu_ms", lambda: None, gpu_ms, gate),
                ("e_timer_note_alone_gpu_ms", lambda: None, gpu_ms, timer_note),
                ("caller_today_recv_readback_numpy_wall_ms", restore_recv, wall_ms, today),
                ("resident_recv_notes_wall_ms", restore_recv, wall_ms, lambda: (recv(), timer_note(), ep_note())))
        t = {name: [] for name, *_ in legs}
        for rep in range(9):
            for name, restore, clock, fn in legs:
                restore()
                t[name].append(clock(fn))
                if name.startswith("b_"):
                    assert (b.status[:n] == 0).all().item() and not E.claim.any().item()
                if name.startswith("d_"):
                    assert (st_send == 0).all().item() and torch.equal(slots_out, slots)
        r = {k: {"median": round(float(np.median(v[2:])), 4), "min": round(min(v[2:]), 4), "max": round(max(v[2:]), 4)}
             for k, v in t.items()}
        # the device table and the caller's host map hold the same addresses
        rows = E.endpoints.cpu().numpy()
        assert np.array_equal(rows[:, :18], host_ep[:, :18]) and (rows[:, 18] == 1).all()
        return {"packets": n, "sessions": nk, **r}

    res = {"cfg2": shape(workloads.build("cfg2")), "cfg4": shape(workloads.build("cfg4")),
           "one_session_1024": shape(workloads.uniform(1024, name="1ki")),
           "note": "9 alternating repetitions, the first two dropped; frames, windows, timers and send state restored "
                   "outside the timed region; peer = session, every packet authentic; *_gpu_ms by stream events around "
                   "the calls named, *_wall_ms by host wall clock around the calls and a device sync; the (e) calls run "
                   "on the key_idx_out and status the receive before them left; caller_today = the same receive, then "
                   "status and key_idx_out to pinned memory, a stream synchronise and a numpy last-per-peer into a "
                   "host address map"}
    with open(os.path.join(root, "profiles", "endpoint_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return res


def demux_leg(eng):
    """The device-resident inbound demultiplexer at 64 Ki and 1 Mi datagrams, one 256-byte slot of buf each, on an
    IMIX-like mix (1 % handshake, 0.1 % cookie, the rest data) and an all-handshake flood (initiations and responses
    in turn): rg_demux_batch_dev with every list as long as the batch, the same with lists only as long as what
    arrives (what the pad pass costs), rg_demux_verdict_batch_dev, rg_timer_turn_dev over a table of as many peers
    (one compact of the same shape) by stream events, medians of seven with min-max; and by host wall clock what the
    two calls replace: the type words gathered and read back, a numpy split and the upload of the three lists with
    their addresses, alone and with a resident receive enqueued in front.  Then rg_handshake_init_batch_dev over a
    flood's init_desc and rg_handshake_finish_batch_dev over its resp_desc (inert rows interleaved) against the same
    calls on the dense lists.  Written to profiles/demux_bench.json."""
    import time

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import handshake_cases as hc  # the Python model makes the valid initiations

    from rustyguard_amd import demux, session, timers

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(83)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    words = lambda a: dev(np.asarray(a, np.uint32).view(np.int32))  # noqa: E731
    SLOT = 256
    LEN = {1: 148, 2: 92, 3: 64, 4: 96}

    def measure(fn, clock="gpu", reset=None):
        ev = []
        for _ in range(8):  # the first is the warm-up
            if reset:
                reset()  # outside the timed window
            torch.cuda.synchronize()
            if clock == "gpu":
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                ev.append(a.elapsed_time(b))
            else:
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ev.append((time.perf_counter() - t0) * 1e3)
        ts = sorted(ev[1:])
        return {"ms_median": round(ts[len(ts) // 2], 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4)}

    def batch(n, mix):
        i = np.arange(n)
        if mix == "imix":
            u = rng.random(n)
            types = np.where(u < 0.005, 1, np.where(u < 0.01, 2, np.where(u < 0.011, 3, 4)))
        else:
            types = 1 + i % 2
        desc = np.zeros(n, DESC_DTYPE)
        desc["offset"] = i.astype(np.uint64) * SLOT
        desc["len"] = np.array([0, 148, 92, 64, 96], np.uint32)[types]
        buf = torch.zeros(n * SLOT, dtype=torch.uint8, device="cuda")
        buf.view(torch.int32)[::SLOT // 4] = dev(types.astype(np.int32))
        return types, desc, buf

    # the receive that runs in front of the wall-clock pair: cfg2, 64 Ki x 1500 B on one session
    w = workloads.build("cfg2")
    nk = len(w.receivers)
    b = DeviceBatch(eng, w)
    b.fill()
    b.seal()
    sealed = b.buf.clone()
    rx = dev(aead.rx_table(w.receivers, np.arange(nk, dtype=np.uint32)))
    ws_r, win = eng.replay_workspace(w.n, nk), torch.zeros(nk * 33, dtype=torch.int64, device="cuda")

    def recv():
        eng.recv_batch_dev_resident(b.keys, rx, win, b.desc_open, b.buf, b.status, workspace=ws_r)

    def restore_recv():
        b.buf.copy_(sealed)
        win.zero_()

    out = {}
    for n in (1 << 16, 1 << 20):
        row = {}
        addrs = rng.integers(0, 256, (n, 24), dtype=np.uint8)
        d_addrs = dev(addrs)
        T = session.SessionTables(eng, n, n)
        T.slot_peer[:] = words(np.arange(n))
        T.peer_slot[:] = words(np.arange(n))
        tm = timers.timer_rows(eng, n)
        ka, rk = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
        gate, counts = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
        d_now, ws_t = dev(np.array([10**12], np.int64)), timers.timer_workspace(eng, n, n)
        row["timer_turn_same_rows"] = measure(lambda: timers.turn_dev(eng, T, tm, d_now, ka, rk, gate, counts, workspace=ws_t))
        for mix in ("imix", "flood"):
            types, desc, buf = batch(n, mix)
            d_desc = dev(desc.view(np.uint8).reshape(-1, 16))
            seen = [int(((types == 1) | (types == 2)).sum()), int((types == 3).sum()), int((types == 4).sum())]
            res = {"seen": seen}
            for label, caps in (("demux_caps_n", (n, n, n)), ("demux_caps_seen", tuple(seen))):
                D = demux.Demux(eng, n, *caps)
                res[label] = measure(lambda: D.batch_dev(d_desc, d_addrs, buf))
                assert [int(x) for x in D.counts.cpu().numpy()] == seen + seen
                assert int((D.status == aead.PKT_PENDING).sum()) == n
            chain = [dev(rng.integers(0, 4, c, dtype=np.uint8)) for c in (seen[0], seen[0], seen[0], seen[1], seen[2])]
            saved = D.status.clone()

            def verdict():
                D.verdict_batch_dev(n, *chain)

            # the call finishes every pending status: give them back before each repetition, or the repetitions
            # after the first would find nothing pending and leave at once
            res["verdict"] = measure(verdict, reset=lambda: D.status.copy_(saved))
            assert int((D.status == aead.PKT_PENDING).sum()) == 0
            D.status.copy_(saved)
            pinned = torch.empty(n, dtype=torch.int32).pin_memory()
            at = dev((desc["offset"] // 4).astype(np.int64))

            def caller_today():
                pinned.copy_(buf.view(torch.int32)[at], non_blocking=True)  # the type words, gathered, to the host
                torch.cuda.synchronize()
                t = pinned.numpy()
                hs, ck, da = np.nonzero((t == 1) | (t == 2))[0], np.nonzero(t == 3)[0], np.nonzero(t == 4)[0]
                lists = [dev(desc[hs].view(np.uint8)), dev(addrs[hs]), dev(desc[ck].view(np.uint8)),
                         dev(desc[da].view(np.uint8)), dev(addrs[da])]
                return lists

            res["caller_today_wall"] = measure(caller_today, clock="wall")
            res["demux_wall"] = measure(lambda: D.batch_dev(d_desc, d_addrs, buf), clock="wall")
            # the same two with a resident receive of 64 Ki x 1500 B enqueued in front, as in a running loop: the
            # host path's synchronise waits for it, the demux queues behind it
            res["recv_then_caller_today_wall"] = measure(lambda: (recv(), caller_today()), clock="wall", reset=restore_recv)
            res["recv_then_demux_wall"] = measure(lambda: (recv(), D.batch_dev(d_desc, d_addrs, buf)), clock="wall",
                                                  reset=restore_recv)
            row[mix] = res
        out[f"datagrams_{n}"] = row
        del T, tm

    # init and finish over the padded lists against dense ones: 64 Ki datagrams, valid initiations and valid responses
    # in turn.  The responses answer 32 Ki pending handshakes of a second key pair S to a peer P, made here by the calls
    # the two sides would run.
    n = 1 << 16
    m = n // 2
    rb = lambda k: bytes(rng.integers(0, 256, k, dtype=np.uint8))  # noqa: E731
    sk_s, sk_p, psk = rb(32), rb(32), rb(32)
    pk_s, pk_p = hc.pubkey(sk_s), hc.pubkey(sk_p)
    own_s, own_p = dev(np.frombuffer(sk_s + pk_s, np.uint8)), dev(np.frombuffer(sk_p + pk_p, np.uint8))
    peers_i = dev(hc.peer_rows([(pk_p, psk, hc.mac1_key(pk_p))] * 8))
    rows_p = hc.peer_rows([(pk_s, psk, hc.mac1_key(pk_s))])
    sids = np.arange(m, dtype=np.uint32) + 0x0100_0000
    ts = dev(np.frombuffer(b"".join(hc.tai64n(1_900_000_000, i) for i in range(m)), np.uint8).reshape(m, 12))
    msgs, pending = (torch.zeros((m, w_), dtype=torch.uint8, device="cuda") for w_ in (160, 128))
    st_h = [torch.zeros(m, dtype=torch.uint8, device="cuda") for _ in range(3)]
    eng.handshake_initiate_dev(own_s, peers_i, words(np.arange(m) % 8), None, dev(rng.integers(0, 256, (m, 32), dtype=np.uint8)),
                               ts, dev(sids), None, None, msgs, pending, st_h[0])
    desc_m = np.zeros(m, DESC_DTYPE)
    desc_m["offset"], desc_m["len"] = np.arange(m, dtype=np.uint64) * 160, 148
    res_p, responses, keys_p = (torch.zeros((m, w_), dtype=torch.uint8, device="cuda") for w_ in (128, 96, 64))
    eng.handshake_init_dev(own_p, dev(rows_p), dev(aead.peer_table(rows_p)), dev(desc_m.view(np.uint8).reshape(-1, 16)), None,
                           msgs, res_p, st_h[1])
    eng.handshake_resp_dev(dev(rows_p), res_p, st_h[1], dev(rng.integers(0, 256, (m, 32), dtype=np.uint8)),
                           words(np.arange(m) + 0x0200_0000), None, None, responses, keys_p, st_h[2])
    torch.cuda.synchronize()
    assert all((s_ == aead.PKT_OK).all().item() for s_ in st_h)
    r = hc.Responder(41, npeers=8, neph=256)
    base = np.zeros((256, SLOT), np.uint8)
    for i in range(256):
        msg, _ = hc.make_initiation(r.sk_i[i % 8], r.pk_r, r.esk_i[i], hc.tai64n(1_800_000_000, i), i)
        base[i, :148] = np.frombuffer(msg, np.uint8)
    frames = np.tile(base, (n // 256, 1))
    frames[1::2] = 0
    frames[1::2, :92] = responses.cpu().numpy()[:, :92]
    buf = dev(frames.reshape(-1))
    desc = np.zeros(n, DESC_DTYPE)
    desc["offset"] = np.arange(n, dtype=np.uint64) * SLOT
    desc["len"] = np.where(np.arange(n) % 2 == 0, 148, 92)
    D = demux.Demux(eng, n, n, 0, 0)
    D.batch_dev(dev(desc.view(np.uint8).reshape(-1, 16)), dev(rng.integers(0, 256, (n, 24), dtype=np.uint8)), buf)
    peers = hc.peer_rows(r.peers)
    d_own, d_peers, d_table = dev(r.own), dev(peers), dev(aead.peer_table(peers))
    dense = dev(np.ascontiguousarray(desc[0::2]).view(np.uint8).reshape(-1, 16))
    results, st = torch.zeros((n, 128), dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    padded_ms = measure(lambda: eng.handshake_init_dev(d_own, d_peers, d_table, D.init_desc, None, buf, results, st))
    assert int((st == aead.PKT_OK).sum()) == n // 2 and int((st == aead.PKT_INVALID).sum()) == n // 2
    dense_ms = measure(lambda: eng.handshake_init_dev(d_own, d_peers, d_table, dense, None, buf, results[:n // 2], st[:n // 2]))
    assert (st[:n // 2] == aead.PKT_OK).all().item()
    out["init_over_padded_list"] = {"rows": n, "initiations": n // 2, "padded": padded_ms, "dense": dense_ms}
    pend_table, saved_pending = dev(aead.pending_table(sids)), pending.clone()
    tk = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    pi, ro = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
    claim = torch.zeros(m, dtype=torch.int32, device="cuda")
    dense_r = dev(np.ascontiguousarray(desc[1::2]).view(np.uint8).reshape(-1, 16))
    give_back = lambda: pending.copy_(saved_pending)  # noqa: E731  (a finished row is wiped)
    padded_ms = measure(lambda: eng.handshake_finish_dev(own_s, peers_i, pend_table, pending, D.resp_desc, None, buf, tk, pi, ro,
                                                         claim, st), reset=give_back)
    assert int((st == aead.PKT_OK).sum()) == m and int((st == aead.PKT_INVALID).sum()) == m
    dense_ms = measure(lambda: eng.handshake_finish_dev(own_s, peers_i, pend_table, pending, dense_r, None, buf, tk[:m], pi[:m],
                                                        ro[:m], claim, st[:m]), reset=give_back)
    assert (st[:m] == aead.PKT_OK).all().item()
    out["finish_over_padded_list"] = {"rows": n, "responses": m, "padded": padded_ms, "dense": dense_ms}
    out["note"] = ("stream events around one call each, medians of 7 repetitions after one warm-up; one 256-byte slot of "
                   "buf per datagram, so the type-word gather touches one line per datagram; caps_n = every list n rows "
                   "(the pad pass writes what the mix leaves empty), caps_seen = every list exactly as long as what "
                   "arrives; verdict with all five chain arrays, the pending statuses given back before every repetition; timer_turn_same_rows = rg_timer_turn_dev over n peers "
                   "of one row each, nothing due; *_wall = host wall clock around the call and a device sync; "
                   "caller_today = type words gathered on the device, copied to pinned memory, a synchronise, a numpy "
                   "split and five uploads; recv_then_* = the same pair with rg_recv_batch_dev_resident over 64 Ki x "
                   "1500 B of one session enqueued first inside the timed region (frames and window restored outside it); "
                   "init_over_padded_list / finish_over_padded_list = rg_handshake_init_batch_dev over init_desc and "
                   "rg_handshake_finish_batch_dev over resp_desc of a flood of valid initiations and valid responses in "
                   "turn (half the rows of each inert) against the same calls over the dense lists, the pending rows given "
                   "back before every repetition")
    with open(os.path.join(root, "profiles", "demux_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


def main():
    legs = sys.argv[1:] or ["mac1", "cookie", "rx", "sessions", "replay", "send", "route", "handshake", "initiator",
                            "peerstate", "session", "timers", "pending", "ratelimit", "endpoint", "demux"]
    eng = aead.Engine(0)
    out = {}
    for name, leg in (("mac1", mac1_leg), ("cookie", cookie_leg), ("rx", rx_leg), ("sessions", sessions_leg),
                      ("replay", replay_leg), ("send", send_leg), ("route", route_leg), ("handshake", handshake_leg),
                      ("initiator", initiator_leg), ("peerstate", peerstate_leg), ("session", session_leg),
                      ("timers", timers_leg), ("pending", pending_leg), ("ratelimit", ratelimit_leg),
                      ("endpoint", endpoint_leg), ("demux", demux_leg)):
        if name in legs:
            out[name] = leg(eng)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
