"""Cases shared by the device-send tests (test_send_cpu.py, test_gpu_send_reserve.py, test_gpu_send_resident.py).

A case is (name, state, slots, lens, now): `state` the starting rg_send_state rows as a (nkeys, 3) uint64 array
(counter, started_ns, sent_ns), `slots` / `lens` one per packet, `now` the clock in ns or None (no time rule).
`loop` is the definition: rg_send_batch's array-order loop (include/rg_aead.h, rg_send_reserve_batch_dev) in
plain Python integers.  It is the only source of expected values."""
import numpy as np

OK, ERR, INVALID, REJECTED, UNALIGNED, NOT_DATA, PENDING = range(7)
SKIP = 0xFFFFFFFF
M64 = (1 << 64) - 1
REKEY = 1 << 60
REJECT = M64 - (1 << 13)
REJECT_AFTER_TIME = 180 * 10**9
T0 = 1_000 * 10**9  # a start time well away from 0


def loop(state, slots, lens, now):
    """-> (status u8[n], counters u64[n], rekey u8[n], state' (nkeys, 3) u64)"""
    rows = [[int(x) for x in r] for r in np.asarray(state, np.uint64).reshape(-1, 3)]
    n = len(slots)
    status, counters, rekey = np.zeros(n, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.uint8)
    for i in range(n):
        w = int(slots[i])
        if w == SKIP or w >= len(rows):
            status[i] = REJECTED
        elif int(lens[i]) % 16 != 0:
            status[i] = INVALID
        elif rows[w][0] >= REJECT or (now is not None and ((rows[w][1] + REJECT_AFTER_TIME) & M64) < now):
            status[i] = REJECTED
        else:
            counters[i] = rows[w][0]
            rows[w][0] += 1
            if now is not None:
                rows[w][2] = now
            rekey[i] = rows[w][0] >= REKEY
            status[i] = PENDING
    return status, counters, rekey, np.array(rows, np.uint64).reshape(-1, 3)


def rows(*counters, started=T0, sent=T0 + 5):
    return np.array([[c, started, sent] for c in counters], np.uint64)


def _one_row(name, c0, n, now=T0 + 10):
    return (name, rows(c0), np.zeros(n, np.uint32), np.full(n, 64, np.uint32), now)


def _interleaved(name, n, nkeys=3, seed=0, c0=None):
    rng = np.random.default_rng(1000 + seed)
    start = rows(*(c0 if c0 is not None else [int(x) for x in rng.integers(0, 1 << 40, nkeys)]))
    slots = rng.integers(0, nkeys, n).astype(np.uint32)  # not sorted: every tile holds every row
    return (name, start, slots, np.full(n, 1504, np.uint32), T0 + 10)


def _ineligible(name, n, nkeys, seed):
    """Every kind of packet that takes no counter, between packets that do."""
    rng = np.random.default_rng(2000 + seed)
    slots = rng.integers(0, nkeys, n).astype(np.uint32)
    lens = (rng.integers(0, 95, n) * 16).astype(np.uint32)
    kind = rng.integers(0, 8, n)
    slots[kind == 0] = SKIP
    slots[kind == 1] = nkeys + rng.integers(0, 1000, int((kind == 1).sum()))
    lens[kind == 2] += rng.integers(1, 16, int((kind == 2).sum())).astype(np.uint32)
    both = kind == 3  # no row and a bad length: REJECTED comes first
    slots[both] = SKIP
    lens[both] += 8
    return (name, rows(*[int(x) for x in rng.integers(0, 1 << 34, nkeys)]), slots, lens, T0 + 10)


def _times(name, n=200):
    """Row 0 fresh, row 1 expired (started + 180 s < now), row 2 exactly at the limit (not expired), row 3 with a
    start so late that started + 180 s wraps 64 bits (the host's wrapping add: expired), row 4 without traffic."""
    now = T0 + REJECT_AFTER_TIME + 77
    st = np.array([[5, now - 10, 1], [6, now - REJECT_AFTER_TIME - 1, 2], [7, now - REJECT_AFTER_TIME, 3],
                   [8, M64 - 5, 4], [9, now - 10, 5]], np.uint64)
    slots = (np.arange(n) % 4).astype(np.uint32)
    return (name, st, slots, np.full(n, 16, np.uint32), now)


def cases():
    out = [
        _one_row("n1", 0, 1), _one_row("n64", 17, 64), _one_row("n65", 17, 65),
        _one_row("one_row_2049", 3, 2049), _one_row("one_row_4097", 3, 4097),
        _interleaved("three_rows_65", 65), _interleaved("three_rows_2049", 2049, seed=1),
        _interleaved("three_rows_4097", 4097, seed=2),
        _interleaved("rows_257_n600", 600, nkeys=257, seed=3),  # two radix passes
        _interleaved("rows_70000_n300", 300, nkeys=70000, seed=4),  # three
        _ineligible("ineligible_1row_100", 100, 1, 0), _ineligible("ineligible_3rows_700", 700, 3, 1),
        _ineligible("ineligible_300rows_2500", 2500, 300, 2),
        _one_row("carry_high_word", (1 << 32) - 2, 70),
        _one_row("rekey_edge", REKEY - 3, 6),
        _one_row("reject_edge_5", REJECT - 3, 5),
        _one_row("reject_edge_8300", REJECT - 3, 8300),  # ranks pass 8196: C0 + rank wraps 64 bits
        _interleaved("reject_edge_rows", 3000, c0=[REJECT - 3, REJECT - 900, 12], seed=5),
        _one_row("at_reject", REJECT, 9), _one_row("past_reject", REJECT + 5, 70),
        _one_row("counter_max", M64, 130),
        _times("times"),
        _one_row("no_clock", 40, 65, now=None),
    ]
    name, st, slots, lens, _ = _times("times_no_clock")
    out.append((name, st, slots, lens, None))
    # the head of a tile's row is an ineligible packet; rows change exactly at wave and tile boundaries
    slots = np.repeat(np.arange(5, dtype=np.uint32), [64, 448, 1536, 2048, 3])
    lens = np.full(len(slots), 32, np.uint32)
    lens[[0, 64, 512, 2048, 4096]] = 33
    out.append(("sorted_boundaries", rows(1, 2, 3, 4, 5), slots, lens, T0 + 10))
    return out


def expect_rekey_edge():
    return [0, 0, 1, 1, 1, 1]
