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
    lens = _mix(rng, slots, nkeys, 8)
    return (name, rows(*[int(x) for x in rng.integers(0, 1 << 34, nkeys)]), slots, lens, T0 + 10)


def _mix(rng, slots, nkeys, kinds):
    """Lengths for `slots`, and one packet in `kinds` of each way to take no counter (written into slots and the
    lengths): no row, a row out of range, a bad length, no row and a bad length."""
    n = len(slots)
    lens = (rng.integers(0, 95, n) * 16).astype(np.uint32)
    kind = rng.integers(0, kinds, n)
    slots[kind == 0] = SKIP
    slots[kind == 1] = nkeys + rng.integers(0, 1000, int((kind == 1).sum()))
    lens[kind == 2] += rng.integers(1, 16, int((kind == 2).sum())).astype(np.uint32)
    both = kind == 3  # no row and a bad length: REJECTED comes first
    slots[both] = SKIP
    lens[both] += 8
    return lens


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


# ---- batches large enough for the loops of the grouped scan (csrc/rg_grouped.h) to run more than once
TILE = 2048  # grouped packets per workgroup of the scans and the radix passes (kGroupTile)
# (packets, state rows, rows with traffic): the smallest batches at which the radix scan walks two entries a
# lane, three radix passes run with three entries a lane, and the carry walks two tiles a lane.
# test_send_cpu.py derives these from the numbers.
LARGE_SIZES = ((8193, 300, 300), (18433, 70000, 600), (524289, 300, 300))


def pool_rows(rng, nkeys, pool):
    """`pool` distinct rows of [0, nkeys), sorted.  Rows 0, 255, 256, 257, 65535, 65536 and nkeys - 1 are always
    among them where they exist: every 8-bit digit of the row index is zero for some and non-zero for others."""
    must = sorted({r for r in (0, 255, 256, 257, 65535, 65536, nkeys - 1) if 0 <= r < nkeys})
    assert len(must) <= pool <= nkeys
    if pool == nkeys:
        return np.arange(nkeys)
    rest = np.setdiff1d(np.arange(nkeys), must)
    return np.sort(np.concatenate([must, rng.choice(rest, pool - len(must), replace=False)])).astype(np.int64)


def heavy_rows(rows):
    """The two rows a skewed batch favours: neither the first nor the last of the grouped order."""
    return int(rows[2 * len(rows) // 3]), int(rows[len(rows) // 3])


def skewed_rows(rng, n, rows):
    """A row of `rows` per packet: about half of the packets on one row and a quarter on a second, whose grouped
    runs then span whole tiles without a head in them; the rest uniform."""
    heavy, second = heavy_rows(rows)
    u = rng.random(n)
    pick = np.asarray(rows)[rng.integers(0, len(rows), n)]
    return np.where(u < 0.5, heavy, np.where(u < 0.75, second, pick)).astype(np.uint32)


def _large(name, n, nkeys, pool, seed, heavy_c0=None):
    """_ineligible's kinds of packet, one in eight of them, between packets that take counters, over skewed
    rows.  heavy_c0: the heavy row's starting counter."""
    rng = np.random.default_rng(3000 + seed)
    live = pool_rows(rng, nkeys, pool)
    slots = skewed_rows(rng, n, live)
    lens = _mix(rng, slots, nkeys, 32)
    state = np.empty((nkeys, 3), np.uint64)
    state[:, 0] = rng.integers(0, 1 << 34, nkeys)
    state[:, 1:] = (T0, T0 + 5)
    if heavy_c0 is not None:
        state[heavy_rows(live)[0], 0] = heavy_c0
    return (name, state, slots, lens, T0 + 10)


def large_cases():
    out = [_large(f"large_{n}_rows_{nkeys}", n, nkeys, pool, k) for k, (n, nkeys, pool) in enumerate(LARGE_SIZES)]
    # the heavy row runs out 900 counters in, tiles past the one its run begins in: ranks meet the row's room
    # behind the carry
    n, nkeys, pool = LARGE_SIZES[0]
    out.append(_large(f"large_{n}_rows_{nkeys}_reject_edge", n, nkeys, pool, 7, heavy_c0=REJECT - 900))
    return out


def expect_rekey_edge():
    return [0, 0, 1, 1, 1, 1]
