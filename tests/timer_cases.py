"""The device-resident session timers' model and cases, shared by test_timers_cpu.py and test_gpu_timers.py.

`arm_loop`, `note_send_loop`, `note_recv_loop` and `turn_loop` are the sequential loops of include/rg_aead.h
("device-resident session timers") over plain Python lists; they are the only source of expected values.  A table
is session_cases' dict of lists; the timers are a list of (rekey_at_ns, flags, pad) per row."""
import numpy as np

import session_cases as sc
from session_cases import M64, NONE, OK, REJECTED, SKIP  # noqa: F401

PENDING_FLAG = 1
KEEPALIVE_NS = 10 * 10**9
REKEY_NS = 120 * 10**9
REJECT_NS = 180 * 10**9
REKEY_MSGS = 1 << 60
REJECT_MSGS = M64 - (1 << 13)
TILE = sc.TILE


def past(t, span, now):
    """t + span < now, u64 wrapping add, strict"""
    return ((t + span) & M64) < now


def arm_loop(timers, rows, gate, now, rekey_after):
    timers = list(timers)
    for i, r in enumerate(rows):
        if (gate is None or gate[i] == OK) and r < len(timers):
            timers[r] = ((now + rekey_after) & M64 if rekey_after else 0, 0, 0)
    return timers


def note_send_loop(timers, slots, status, rekey_out, now):
    timers = list(timers)
    for i, r in enumerate(slots):
        if status[i] == OK and rekey_out[i] != 0 and r < len(timers):
            at, flags, pad = timers[r]
            if at == 0 or at > now:
                timers[r] = (now, flags, pad)
    return timers


def note_recv_loop(timers, send_state, key_idx, status, now):
    timers = list(timers)
    for i, k in enumerate(key_idx):
        if status[i] == OK and k < len(timers) and past(send_state[k][2], KEEPALIVE_NS, now):
            at, flags, pad = timers[k]
            timers[k] = (at, flags | PENDING_FLAG, pad)
    return timers


def turn_loop(t, timers, now):
    """-> (timers', ka_slots_out, rekey_peers_out, rekey_gate_out, counts_out); the tables are only read"""
    timers = list(timers)
    slot_peer, peer_slot, state = t["slot_peer"], t["peer_slot"], t["send_state"]
    nkeys, npeers = len(slot_peer), len(peer_slot)
    want_ka, want_rk = [0] * npeers, [0] * npeers
    for r in range(nkeys):
        p = slot_peer[r]
        if p == NONE or p >= npeers:
            continue
        at, flags, pad = timers[r]
        counter, started, sent = state[r]
        if flags & PENDING_FLAG:
            flags &= ~PENDING_FLAG
            if past(sent, KEEPALIVE_NS, now):
                want_ka[p] = 1
        if at != 0 and at < now:
            at = 0
            if past(started, REKEY_NS, now) or counter >= REKEY_MSGS:
                want_rk[p] = 1
        timers[r] = (at, flags, pad)
    ka, rk = [], []
    for p in range(npeers):
        c = peer_slot[p]
        if want_ka[p] and c < nkeys and slot_peer[c] == p and \
                not (past(state[c][1], REJECT_NS, now) or state[c][0] >= REJECT_MSGS):
            ka.append(c)
        if want_rk[p]:
            rk.append(p)
    counts = [len(ka), len(rk)]
    gate = [OK] * len(rk) + [REJECTED] * (npeers - len(rk))
    return timers, ka + [SKIP] * (npeers - len(ka)), rk + [NONE] * (npeers - len(rk)), gate, counts


# ------------------------------------------------------------------- cases
def tables(rows, peer_slot):
    """rows of (peer, counter, started_ns, sent_ns) -> a session_cases table (keys and windows stay zero: the timer
    calls read none of them)"""
    t = sc.empty_tables(len(rows), len(peer_slot))
    t["slot_peer"] = [r[0] for r in rows]
    t["send_state"] = [tuple(r[1:]) for r in rows]
    t["peer_slot"] = list(peer_slot)
    return t


def edge_times(now):
    """what a row's times are drawn from: one below, at and one above each of the three deadlines as seen from
    `now`, a fresh session, and a start whose sum with every timeout wraps to a small number"""
    sent = [now - KEEPALIVE_NS - 1, now - KEEPALIVE_NS, now - KEEPALIVE_NS + 1, now - 5]
    started = [now - span + d for span in (REKEY_NS, REJECT_NS) for d in (-1, 0, 1)] + [now - 7, (1 << 64) - 100]
    rekey_at = [0, 0, now - 1, now, now + 1, 1, now + REKEY_NS]
    return sent, started, rekey_at


COUNTERS = (0, 5, REKEY_MSGS - 1, REKEY_MSGS, REJECT_MSGS - 1, REJECT_MSGS)
FLAGS = (0, 0, PENDING_FLAG, PENDING_FLAG, 0x10, 0x10 | PENDING_FLAG)


def random_case(nkeys, npeers, seed, now=10**12, live=0.8):
    """-> (tables, timers): a share `live` of the rows live on peers below npeers (one in sixteen of them on a peer
    past the table, which the turn leaves alone), times, counters and flags drawn from the edge values; a peer's
    current row is one of its own rows, a free row, another peer's row, a row past the table or none"""
    rng = np.random.default_rng(seed)
    sent, started, rekey_at = edge_times(now)
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]  # noqa: E731
    rows, timers = [], []
    for r in range(nkeys):
        u = rng.random()
        peer = NONE if u >= live else (npeers + 3 if u < live / 16 else int(rng.integers(0, npeers)))
        rows.append((peer, pick(COUNTERS), pick(started), pick(sent)))
        timers.append((pick(rekey_at), pick(FLAGS), int(rng.integers(0, 3))))
    own = {}
    for r, row in enumerate(rows):
        own.setdefault(row[0], []).append(r)
    peer_slot = []
    for p in range(npeers):
        u = rng.random()
        if u < 0.7 and p in own:
            peer_slot.append(pick(own[p]))
        elif u < 0.8:
            peer_slot.append(int(rng.integers(0, nkeys)))
        elif u < 0.9:
            peer_slot.append(nkeys + int(rng.integers(0, 5)))
        else:
            peer_slot.append(SKIP)
    return tables(rows, peer_slot), timers


def due_case(nkeys, npeers, share, now=10**12, seed=5):
    """the benchmark's and the pile-up test's table: every row live, row r on peer r % npeers, the peer's current row
    its last one; a share `share` of the rows pending and silent and with a rekey entry due on an old session"""
    rng = np.random.default_rng(seed)
    due = rng.random(nkeys) < share
    rows = [(r % npeers, 3, now - REKEY_NS - 9 if due[r] else now - 9, now - KEEPALIVE_NS - 9 if due[r] else now - 9)
            for r in range(nkeys)]
    timers = [(now - 1, PENDING_FLAG, 0) if due[r] else (now + REKEY_NS, 0, 0) for r in range(nkeys)]
    peer_slot = [SKIP] * npeers
    for r in range(nkeys):
        peer_slot[r % npeers] = r
    return tables(rows, peer_slot), timers


def note_batch(nkeys, n, seed):
    """-> (rows, status, rekey_out) for the three note calls: rows repeat (a handful of rows take most of the
    batch), one in eight is RG_KEY_SKIP or past the table, one status in four is not RG_PKT_OK"""
    rng = np.random.default_rng(seed)
    hot = [int(x) for x in rng.integers(0, nkeys, 4)]
    rows, status, rekey = [], [], []
    for i in range(n):
        u = rng.random()
        rows.append(SKIP if u < 0.06 else nkeys + int(rng.integers(0, 9)) if u < 0.12 else
                    hot[i % 4] if u < 0.6 else int(rng.integers(0, nkeys)))
        status.append(OK if rng.random() < 0.75 else int(rng.integers(1, 11)))
        rekey.append(int(rng.integers(0, 2)) * int(rng.integers(1, 256)))
    return rows, status, rekey
