"""The device-resident pending handshakes' model and cases, shared by test_pending_cpu.py and test_gpu_pending.py.

`install_loop` and `turn_loop` are the sequential loops of include/rg_aead.h ("device-resident pending handshakes")
over plain Python lists; they are the only source of expected values.  A table is a dict of lists, one entry a peer:
pending (128 bytes), timers ((started_ns, sent_ns)) and hs_ids; pend_table is modelled by its lookup, `lookup`."""
import numpy as np

OK, INVALID, REJECTED = 0, 2, 3
NONE = 0xFFFFFFFF
M64 = (1 << 64) - 1
RETRY_NS = 5 * 10**9
ATTEMPT_NS = 90 * 10**9
ROW = 128
TILE = 2048
EMPTY = bytes(96) + NONE.to_bytes(4, "little") + bytes(28)  # a wiped row: zeros with peer = RG_PEER_NONE


def past(t, span, now):
    """t + span < now, u64 wrapping add, strict"""
    return ((t + span) & M64) < now


def before(now, t, span):
    """now < t + span, the same arithmetic"""
    return now < ((t + span) & M64)


def row_peer(row):
    return int.from_bytes(row[96:100], "little")


def row_sender(row):
    return int.from_bytes(row[100:104], "little")


def make_row(peer, sender, rng):
    """a synthetic rg_hs_pending: random state, key and padding around the two words the calls read"""
    body = rng.integers(0, 256, ROW, dtype=np.uint8).tobytes()
    return body[:96] + peer.to_bytes(4, "little") + sender.to_bytes(4, "little") + body[104:]


def empty_table(npeers):
    return {"pending": [EMPTY] * npeers, "timers": [(0, 0)] * npeers, "hs_ids": [0] * npeers}


def is_live(t, p):
    return row_peer(t["pending"][p]) == p


def lookup(t):
    """sender id -> peer over the live rows: what pend_table answers"""
    return {row_sender(r): p for p, r in enumerate(t["pending"]) if row_peer(r) == p}


def copy_table(t):
    return {k: list(v) for k, v in t.items()}


# ---------------------------------------------------------------- the loops
def install_loop(t, batch, gate, now):
    """-> (table', batch', status, installed_out); status of a call that never ran is not modelled"""
    t, batch = copy_table(t), list(batch)
    npeers = len(t["pending"])
    live0 = [is_live(t, p) for p in range(npeers)]
    started0 = [tm[0] for tm in t["timers"]]
    status, installed = [None] * len(batch), [NONE] * len(batch)
    last = {}
    for i in range(len(batch)):
        if gate is not None and gate[i] != OK:
            status[i] = REJECTED
            continue
        row, batch[i] = batch[i], EMPTY
        p = row_peer(row)
        if p >= npeers:
            status[i] = INVALID
            continue
        status[i] = OK
        if p in last:
            installed[last[p]] = NONE  # replaced by this one
        last[p] = i
        t["pending"][p] = row
        t["hs_ids"][p] = row_sender(row)
        t["timers"][p] = (started0[p] if live0[p] else now, now)
        installed[i] = p
    return t, batch, status, installed


def turn_loop(t, now, start_peers=(), start_status=None, start_match=OK):
    """-> (table', init_peers_out, init_gate_out, expired_out, counts_out)"""
    t = copy_table(t)
    npeers = len(t["pending"])
    want, expired = [0] * npeers, [0] * npeers
    for p in range(npeers):
        if not is_live(t, p):
            continue
        started, sent = t["timers"][p]
        if past(sent, ATTEMPT_NS, now):
            t["pending"][p], t["timers"][p], expired[p] = EMPTY, (0, 0), 1
        elif past(sent, RETRY_NS, now) and before(now, started, ATTEMPT_NS):
            want[p] = 1
            t["timers"][p] = (started, now)
    for j, q in enumerate(start_peers):
        if start_status is not None and start_status[j] != start_match:
            continue
        if q < npeers and not is_live(t, q):
            want[q] = 1
    init = [p for p in range(npeers) if want[p]]
    k = len(init)
    return (t, init + [NONE] * (npeers - k), [OK] * k + [REJECTED] * (npeers - k), expired, [k, sum(expired)])


# -------------------------------------------------------------------- cases
def sender_of(p, attempt=0):
    """the caller's session ids in these cases: unique over peers and attempts"""
    return (0x5000000 + 0x10000 * attempt + p * 2654435761) & 0xFFFFFFFF


def edge_timers(now):
    """(started_ns, sent_ns) pairs a live row draws from: the expiry one below, at and one above its deadline, the
    retry the same, a retry whose first attempt is exactly, one short of and one past REKEY_ATTEMPT_TIME old, and
    a fresh row"""
    e, r = now - ATTEMPT_NS, now - RETRY_NS
    return [(e - 9, e - 1), (e, e), (e - 3, e + 1),                 # expires; stays (no retry: started is too old); stays
            (r - 1, r - 1), (r, r), (r + 1, r + 1),                 # retries; not yet; not yet
            (e, r - 1), (e + 1, r - 1), (e - 1, r - 1),             # no retry at now == started + 90 s; retries; none
            (now - 1, now - 1)]


def random_table(npeers, seed, now=10**12, live=0.7):
    """a share `live` of the rows live with timers from edge_timers; the others wiped, never used (all zero) or
    naming another peer (a stale copy), their timers and ids garbage that must stay"""
    rng = np.random.default_rng(seed)
    pairs = edge_timers(now)
    t = empty_table(npeers)
    for p in range(npeers):
        u = rng.random()
        if u < live:
            t["pending"][p] = make_row(p, sender_of(p), rng)
            t["timers"][p] = pairs[int(rng.integers(0, len(pairs)))]
            t["hs_ids"][p] = sender_of(p)
        else:
            kind = int(rng.integers(0, 3))
            if kind == 1:
                t["pending"][p] = make_row((p + 1) % (npeers + 2), sender_of(p, 7), rng)  # not p: not live
            elif kind == 2:
                t["pending"][p] = make_row(NONE, sender_of(p, 7), rng)
            t["timers"][p] = (int(rng.integers(1, now)), int(rng.integers(1, now)))
            t["hs_ids"][p] = int(rng.integers(0, 1 << 32))
    return t


def request_list(npeers, m, seed):
    """-> (start_peers, start_status): peers with duplicates, RG_PEER_NONE padding and entries past the table; one
    status in three is not the matching one"""
    rng = np.random.default_rng(seed)
    hot = [int(x) for x in rng.integers(0, npeers, 3)]
    peers, status = [], []
    for j in range(m):
        u = rng.random()
        peers.append(NONE if u < 0.15 else npeers + int(rng.integers(0, 5)) if u < 0.25 else
                     hot[j % 3] if u < 0.45 else int(rng.integers(0, npeers)))
        status.append(REJECTED if rng.random() < 0.67 else int(rng.choice([OK, INVALID, 6])))
    return peers, status


def install_batch(n, npeers, seed):
    """-> (batch, gate): synthetic rows; one row in six is gated off, one in eight names a peer past the table (or
    RG_PEER_NONE, a failed initiation); peer 1 has rows on both sides of the wave edge (63 | 64) and of the tile
    edge (2047 | 2048) where the batch reaches them, and the last row is its own, so the claim crosses both"""
    rng = np.random.default_rng(seed)
    batch, gate = [], []
    straddle = {63, 64, 2047, 2048, n - 1}
    for i in range(n):
        u = rng.random()
        p = 1 % npeers if i in straddle else NONE if u < 0.06 else npeers + int(rng.integers(0, 3)) if u < 0.125 else \
            int(rng.integers(0, npeers))
        batch.append(make_row(p, (0x7100000 + i) & 0xFFFFFFFF, rng))
        gate.append(OK if i in straddle or rng.random() >= 1 / 6 else int(rng.choice([INVALID, REJECTED, 6])))
    return batch, gate


def rx_slot(ident, cap):
    """the home slot of an id in a table of cap entries (rg_rx_table_build's hash)"""
    return ((ident * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - (cap.bit_length() - 1)) if cap > 1 else 0


def colliding_ids(count, cap, slot=5):
    """`count` distinct ids whose home slot in a table of cap entries is `slot`"""
    out, ident = [], 1
    while len(out) < count:
        if rx_slot(ident, cap) == slot:
            out.append(ident)
        ident += 1
    return out
