"""The device-resident session table's model and cases, shared by test_session_cpu.py and test_gpu_session.py.

`install_loop` and `expire_loop` are the sequential loops of include/rg_aead.h ("device-resident session table")
over plain Python lists; they are the only source of expected values.  A table is a dict of lists, one entry per
row (keys, windows as bytes, send_state as (counter, started_ns, sent_ns)) or per peer (peer_slot); the receiver
table is not part of it: `rx_pairs` gives the pairs it must answer."""
import numpy as np

OK, ERR, INVALID, REJECTED, UNALIGNED, NOT_DATA, PENDING, COOKIE, KEYEXCHANGE, UNROUTABLE, FULL = range(11)
SKIP = 0xFFFFFFFF
NONE = 0xFFFFFFFF
WINDOW = 264
REJECT_AFTER_NS = 180 * 10**9
M64 = (1 << 64) - 1
TILE = 2048  # rows of one workgroup in the device's scans (rustyguard_amd/csrc/rg_grouped.h, kGroupTile)
ROW_ARRAYS = ("send_keys", "recv_keys", "receivers", "local_ids", "slot_peer", "windows", "send_state")


def empty_tables(nkeys, npeers):
    return dict(send_keys=[bytes(32)] * nkeys, recv_keys=[bytes(32)] * nkeys, receivers=[0] * nkeys,
                local_ids=[0] * nkeys, slot_peer=[NONE] * nkeys, windows=[bytes(WINDOW)] * nkeys,
                send_state=[(0, 0, 0)] * nkeys, peer_slot=[SKIP] * npeers)


def copy_tables(t):
    return {k: list(v) for k, v in t.items()}


def seed_row(t, r, local_id, remote_id, peer, rng, started=0, current=True):
    """a live row written by hand, as a caller that seeds rows itself would: random keys, a used window and a
    counter that has moved"""
    t["send_keys"][r] = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    t["recv_keys"][r] = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    t["receivers"][r], t["local_ids"][r], t["slot_peer"][r] = remote_id, local_id, peer
    t["windows"][r] = bytes(rng.integers(0, 256, WINDOW, dtype=np.uint8))
    t["send_state"][r] = (int(rng.integers(1, 1000)), started, started + 5)
    if current:
        t["peer_slot"][peer] = r


def rx_pairs(t):
    """what the receiver table must answer: id -> row over the live rows"""
    return {t["local_ids"][r]: r for r in range(len(t["slot_peer"])) if t["slot_peer"][r] != NONE}


def install_loop(t, gate, local_ids, remote_ids, peers, keys, now=None):
    """-> (tables', status, rows_out, keys'): keys'[i] is keys[i] for a gated row and 64 zero bytes otherwise"""
    t = copy_tables(t)
    nkeys, npeers, n = len(t["slot_peer"]), len(t["peer_slot"]), len(local_ids)
    free = [r for r in range(nkeys) if t["slot_peer"][r] == NONE]
    seen = set(rx_pairs(t))
    status, rows_out, keys_out = [PENDING] * n, [SKIP] * n, list(keys)
    now = 0 if now is None else now
    for i in range(n):
        if gate is not None and gate[i] != OK:
            status[i] = REJECTED
            continue
        key = keys[i]
        keys_out[i] = bytes(64)
        if peers[i] >= npeers:
            status[i] = INVALID
            continue
        if local_ids[i] in seen:
            status[i] = REJECTED
            continue
        seen.add(local_ids[i])
        if not free:
            status[i] = FULL
            continue
        r = free.pop(0)
        t["send_keys"][r], t["recv_keys"][r] = key[:32], key[32:]
        t["receivers"][r], t["local_ids"][r], t["slot_peer"][r] = remote_ids[i], local_ids[i], peers[i]
        t["windows"][r] = bytes(WINDOW)
        t["send_state"][r] = (0, now, now)
        t["peer_slot"][peers[i]] = r
        rows_out[i], status[i] = r, OK
    return t, status, rows_out, keys_out


def gather_resp(session_ids, results):
    """the response call's outputs -> (local_ids, remote_ids, peers); results: 128-byte rg_hs_init_result rows"""
    word = lambda row, at: int.from_bytes(row[at:at + 4], "little")  # noqa: E731
    return list(session_ids), [word(r, 112) for r in results], [word(r, 108) for r in results]


def gather_finish(gate, pend_idx, remote_out, pend_sids, pend_peers):
    """the finish call's outputs -> (local_ids, remote_ids, peers); a pending row that does not exist names no
    peer (RG_PKT_INVALID on a row whose gate is OK)"""
    ok = [p < len(pend_sids) for p in pend_idx]
    return ([pend_sids[p] if o else 0 for p, o in zip(pend_idx, ok)], list(remote_out),
            [pend_peers[p] if o else NONE for p, o in zip(pend_idx, ok)])


def expire_loop(t, now=None, rows=()):
    """-> (tables', expired)"""
    t = copy_tables(t)
    nkeys = len(t["slot_peer"])
    named = {r for r in rows if r < nkeys}
    expired = [0] * nkeys
    for r in range(nkeys):
        p = t["slot_peer"][r]
        if p == NONE:
            continue
        late = now is not None and ((t["send_state"][r][1] + REJECT_AFTER_NS) & M64) < now
        if not (late or r in named):
            continue
        t["send_keys"][r] = t["recv_keys"][r] = bytes(32)
        t["windows"][r], t["send_state"][r] = bytes(WINDOW), (0, 0, 0)
        t["receivers"][r] = t["local_ids"][r] = 0
        if p < len(t["peer_slot"]) and t["peer_slot"][p] == r:
            t["peer_slot"][p] = SKIP
        t["slot_peer"][r] = NONE
        expired[r] = 1
    return t, expired


# ------------------------------------------------------------------- cases
def rx_home(receiver, cap):
    """the home slot of an id in a receiver table of cap entries (include/rg_aead.h, rg_rx_entry)"""
    return ((receiver * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - cap.bit_length() + 1) if cap > 1 else 0


def same_home(first, cap, count):
    """`count` ids from `first` upwards that share first's home slot"""
    out, x = [], first
    while len(out) < count:
        if rx_home(x, cap) == rx_home(first, cap):
            out.append(x)
        x += 1
    return out


def key_rows(rng, n):
    return [bytes(rng.integers(0, 256, 64, dtype=np.uint8)) for _ in range(n)]


def batch(rows, rng):
    """rows of (gate, local id, remote id, peer) -> the install's arguments as a dict"""
    return dict(gate=[r[0] for r in rows], local_ids=[r[1] for r in rows], remote_ids=[r[2] for r in rows],
                peers=[r[3] for r in rows], keys=key_rows(rng, len(rows)))


def every_rule_case():
    """nkeys = 8, npeers = 4, n = 12: five live rows (free: 1, 4, 7), and a batch with gated rows between OK rows,
    a peer >= npeers, a duplicate of a live id, the free list running out at index 7, a duplicate (index 8) of
    that first RG_PKT_FULL row, a duplicate of an installed row, two handshakes of peer 1 (the later one stays in
    peer_slot) and two ids that share a home slot of the 16-entry receiver table.
    -> (tables, batch, now, expected status, expected rows_out, expected peer_slot)"""
    rng = np.random.default_rng(11)
    t = empty_tables(8, 4)
    for r, (lid, peer) in {0: (0x100, 0), 2: (0x101, 1), 3: (0x102, 2), 5: (0x103, 2), 6: (0x104, 0)}.items():
        seed_row(t, r, lid, 0x9000 + r, peer, rng, started=77)
    a, c = same_home(0x2000, 16, 2)
    b, d, e = 0x3001, 0x3002, 0x3003
    rows = [(OK, a, 0x51, 1), (REJECTED, 0x4000, 0x52, 0), (OK, 0x4001, 0x53, 9), (OK, 0x101, 0x54, 3),
            (OK, b, 0x55, 3), (PENDING, 0x4002, 0x56, 1), (OK, c, 0x57, 1), (OK, d, 0x58, 0), (OK, d, 0x59, 2),
            (OK, a, 0x5A, 2), (OK, e, 0x5B, 2), (OK, 0x4003, 0x5C, NONE)]
    status = [OK, REJECTED, INVALID, REJECTED, OK, REJECTED, OK, FULL, REJECTED, REJECTED, FULL, INVALID]
    rows_out = [1, SKIP, SKIP, SKIP, 4, SKIP, 7, SKIP, SKIP, SKIP, SKIP, SKIP]
    return t, batch(rows, rng), 123_456_789_000, status, rows_out, [6, 7, 5, 4]


def scattered_tables(nkeys, npeers, seed, extra_live=()):
    """every third row live (and the rows of extra_live), ids 0x10000 + r"""
    rng = np.random.default_rng(seed)
    t = empty_tables(nkeys, npeers)
    for r in range(nkeys):
        if r % 3 == 0 or r in extra_live:
            seed_row(t, r, 0x10000 + r, 0x20000 + r, r % npeers, rng, started=1000 + r)
    return t


def scattered_batch(n, npeers, seed):
    """every third handshake not eligible (gated, a peer past the table, the id of a live row, the id of an
    earlier row of the batch, in turn), the others eligible with ids 0x40000 + i"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        row = [OK, 0x40000 + i, 0x50000 + i, int(rng.integers(0, npeers))]
        if i % 3 == 0:
            kind = (i // 3) % 4
            if kind == 0:
                row[0] = (REJECTED, INVALID, PENDING, ERR)[(i // 12) % 4]
            elif kind == 1:
                row[3] = (npeers, npeers + 7, NONE)[(i // 12) % 3]
            elif kind == 2:
                row[1] = 0x10000  # row 0 is live
            else:
                j = int(rng.integers(1, i))
                row[1] = 0x40000 + j + (j % 3 == 0)  # an eligible row ahead of this one
        rows.append(tuple(row))
    return batch(rows, rng)


def expiry_case():
    """nkeys = 10, npeers = 4, now = 10^12.  Rows by started_ns: row 0 exactly at the limit (stays), row 1 one
    nanosecond past it (goes), row 2 near 2^64 (the add wraps to a small number: goes), row 3 fresh and named in
    `rows` (goes), row 4 fresh (stays), row 6 old and an older session of peer 1 whose current row is 4 (goes,
    peer_slot[1] stays 4); rows 5, 7, 8, 9 free; `rows` also names the free row 5 and two indices >= nkeys.
    -> (tables, now, rows, expected expired, expected peer_slot)"""
    rng = np.random.default_rng(12)
    now = 10**12
    t = empty_tables(10, 4)
    limit = now - REJECT_AFTER_NS
    seed_row(t, 6, 0x706, 0x806, 1, rng, started=5)
    for r, (peer, started) in {0: (0, limit), 1: (2, limit - 1), 2: (3, (1 << 64) - 100), 3: (0, now - 5),
                               4: (1, now - 9)}.items():
        seed_row(t, r, 0x700 + r, 0x800 + r, peer, rng, started=started)
    assert t["peer_slot"] == [3, 4, 1, 2]
    return t, now, [3, 5, 10, SKIP], [0, 1, 1, 1, 0, 0, 1, 0, 0, 0], [SKIP, 4, SKIP, SKIP]
