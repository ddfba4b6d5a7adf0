"""Shared by test_replay_cpu.py and test_gpu_replay.py: the batched anti-replay commit as the header defines it
-- the host rg_antireplay_would_accept / rg_antireplay_mark_seen through ctypes, packet by packet in array
order -- and the seeded cases both tests run.  Windows are numpy uint64 [nwin, 33] (32 bitmap words, last: 264 bytes a row)."""
import ctypes
import functools

import numpy as np

from rustyguard_amd import _lib

OK, ERR, INVALID, REJECTED, PENDING = 0, 1, 2, 3, 6
SKIP = 0xFFFFFFFF
WINDOW = 1984
U64 = (1 << 64) - 1
CLASSES = ("accepted", "too_old", "seen_initial", "duplicate", "bad_tag_kept")


def fresh(nwin=1):
    return np.zeros((nwin, 33), np.uint64)


def live(last, seed):
    """One window with `last` and a random bitmap in every slot."""
    w = np.zeros(33, np.uint64)
    w[:32] = np.random.default_rng(seed).integers(0, 1 << 64, 32, dtype=np.uint64)
    w[32] = last
    return w


def host_commit(windows, win_idx, counters, status):
    """The sequential definition (include/rg_aead.h, rg_replay_batch_dev).  Returns (status, undo, windows,
    outcome class per packet or None)."""
    L = _lib.lib()
    W = np.ascontiguousarray(windows, np.uint64).copy()
    st = np.array(status, np.uint8).copy()
    undo = np.zeros(len(st), np.uint8)
    cls = [None] * len(st)
    seen = set()
    for i in range(len(st)):
        w = int(win_idx[i])
        if w == SKIP or w >= len(W) or st[i] not in (OK, ERR):
            continue
        c = int(counters[i])
        p = ctypes.c_void_p(W[w].ctypes.data)
        if not L.rg_antireplay_would_accept(p, c):
            last = int(W[w, 32])
            cls[i] = "too_old" if last - c >= WINDOW else "duplicate" if (w, c) in seen else "seen_initial"
            undo[i] = st[i] == OK
            st[i] = REJECTED
        elif st[i] == OK:
            L.rg_antireplay_mark_seen(p, c)
            seen.add((w, c))
            cls[i] = "accepted"
        else:
            cls[i] = "bad_tag_kept"
    return st, undo, W, cls


def reference_sequence():
    """check_accept_and_mark's counters (anti_replay.rs:78-97), in its order."""
    seq = []
    for i in range(2048):
        seq += [2 * i + 1, 2 * i + 1, 2 * i, 2 * i]
    seq += list(range(4096))
    seq += [4096 + 2048, 4097, 65535, 10000, 66000]
    return np.array(seq, np.uint64)


def edge_cases():
    """(name, starting window, counters, statuses): every edge from a fresh window and from last = 10 000 with a
    random live bitmap."""
    out = []
    for tag, win in (("fresh", fresh()[0]), ("live", live(10_000, 99))):
        L = int(win[32])
        nxt = (L >> 6) + 1

        def add(name, ctrs, sts=None):
            out.append((f"{name}-{tag}", win.copy(), np.array(ctrs, np.uint64),
                        np.array(sts if sts is not None else [OK] * len(ctrs), np.uint8)))

        add("zero_twice", [0, 0])
        add("behind_1983_1984", [L + 5000, L + 5000 - 1983, L + 5000 - 1984, L + 5000 - 1983])
        if L >= WINDOW:
            add("behind_start_1983_1984", [L - 1983, L - 1984, L - 1983])
        c32, c33 = ((nxt + 32) << 6) | 5, ((nxt + 33) << 6) | 5
        add("jump_32_blocks", [L + 1, L + 3, c32, L + 3, c32 - 64, c32 - 1983, L + 70])
        add("jump_33_blocks", [L + 1, L + 3, c33, L + 3, c33 - 64, c33 - 1983, L + 70])
        add("jump_2_40", [L + 1, L + (1 << 40), L + 1, L + (1 << 40) - 5, L + (1 << 40)])
        add("top_of_range", [U64, U64 - 1, U64 - WINDOW, U64, U64 - 1983])
        add("err_ok_ok_err", [L + 7] * 4, [ERR, OK, OK, ERR])
        add("above_last_in_its_block", [L + 10, L + 10, L + 5, L + 12, L + 5])
    return out


def _mix(rng, length, W, rows):
    """interleaved's traffic over the window rows `rows` of W: counters drawn around each window's moving edge;
    about one entry in eight has no window or no verdict to judge.  Returns (win_idx, counters, status)."""
    nwin = len(W)
    start = {int(w): int(W[w, 32]) for w in rows}
    edge = dict(start)
    drawn = {w: [] for w in start}
    widx, ctrs, sts = [], [], []
    for _ in range(length):
        w = int(rows[int(rng.integers(0, len(rows)))])
        kind = rng.random()
        if kind < 0.30:
            c = edge[w] + int(rng.integers(1, 9))
        elif kind < 0.45:
            c = edge[w] - int(rng.integers(0, 300))
        elif kind < 0.62 and drawn[w]:
            c = drawn[w][int(rng.integers(0, len(drawn[w])))]
        elif kind < 0.76:
            c = edge[w] - int(rng.integers(WINDOW, 4000))
        elif kind < 0.90:
            c = start[w] - int(rng.integers(0, 200))
        else:
            c = edge[w] + int(rng.integers(1, 3))
        c = min(max(c, 0), U64)
        st = ERR if rng.random() < 0.15 else OK
        if st == OK:
            edge[w] = max(edge[w], c)
        drawn[w].append(c)
        neutral = rng.random()
        if neutral < 0.03:
            w = SKIP
        elif neutral < 0.06:
            w = nwin + int(rng.integers(0, 5))
        elif neutral < 0.09:
            st = INVALID
        elif neutral < 0.125:
            st = PENDING
        widx.append(w)
        ctrs.append(c)
        sts.append(st)
    return np.array(widx, np.uint32), np.array(ctrs, np.uint64), np.array(sts, np.uint8)


def interleaved(seed, length, nwin=3):
    """Three windows mixed in one batch, counters drawn around each window's moving edge; about one entry in
    eight has no window or no verdict to judge.  Returns (windows, win_idx, counters, status)."""
    rng = np.random.default_rng(seed)
    W = np.stack([fresh()[0], live(10_000, seed + 1), live(1 << 40, seed + 2)][:nwin])
    return (W,) + _mix(rng, length, W, np.arange(nwin))


INTERLEAVED_LENGTHS = (1, 63, 64, 65, 257, 1025)
# Smallest share of every outcome class in the seeded batches of 257 and 1025 packets.  The generator above
# yields, over seeds 0-3 at these lengths (measured on the CPU, test_replay_cpu.py prints them): accepted
# 38-43 %, too old 7-10 %, seen in the initial bitmap 6-11 %, duplicate 19-25 %, bad tag kept 4.7-8.6 %.
MIN_SHARE = 0.04


def class_shares(cls):
    return {k: sum(1 for c in cls if c == k) / len(cls) for k in CLASSES}


def many_windows(seed=5, nwin=300):
    """300 windows, 1-3 packets each, shuffled."""
    rng = np.random.default_rng(seed)
    W = np.stack([fresh()[0] if w % 2 == 0 else live(5000 + 37 * w, 1000 + w) for w in range(nwin)])
    widx, ctrs, sts = [], [], []
    for w in range(nwin):
        last = int(W[w, 32])
        for _ in range(int(rng.integers(1, 4))):
            widx.append(w)
            ctrs.append(max(0, last + int(rng.integers(-40, 40))))
            sts.append(ERR if rng.random() < 0.1 else OK)
    perm = rng.permutation(len(widx))
    return (W, np.array(widx, np.uint32)[perm], np.array(ctrs, np.uint64)[perm], np.array(sts, np.uint8)[perm])


# ---- batches large enough for the loops of the grouped scan (csrc/rg_grouped.h) to run more than once
TILE = 2048  # grouped packets per workgroup of the scans and the radix passes (kGroupTile)
STRIDE = 2000  # between a window's consecutive counters in `strided`: two of them swapped are >= WINDOW apart
# (packets, window rows, rows with traffic): the smallest batches at which two radix passes run over three tiles,
# the radix scan walks two entries a lane, three passes run with three entries a lane, and (CARRY_SIZE) the carry
# walks two tiles a lane.  test_replay_cpu.py derives these from the numbers.
LARGE_SIZES = ((4097, 257, 257), (8193, 300, 300), (18433, 70000, 600))
CARRY_SIZE = (524289, 300, 300)


def pool_rows(rng, nwin, pool):
    """`pool` distinct rows of [0, nwin), sorted.  Rows 0, 255, 256, 257, 65535, 65536 and nwin - 1 are always
    among them where they exist: every 8-bit digit of the row index is zero for some and non-zero for others."""
    must = sorted({r for r in (0, 255, 256, 257, 65535, 65536, nwin - 1) if 0 <= r < nwin})
    assert len(must) <= pool <= nwin
    if pool == nwin:
        return np.arange(nwin)
    rest = np.setdiff1d(np.arange(nwin), must)
    return np.sort(np.concatenate([must, rng.choice(rest, pool - len(must), replace=False)])).astype(np.int64)


def pool_windows(nwin, rows, seed):
    """nwin windows, all zero but the pool's, which alternate fresh and live as many_windows' do."""
    W = fresh(nwin)
    for k, w in enumerate(rows):
        if k % 2:
            W[w] = live(5000 + 37 * k, 1000 + 7 * seed + k)
    return W


def heavy_rows(rows):
    """The two rows a skewed batch favours: neither the first nor the last of the grouped order."""
    return int(rows[2 * len(rows) // 3]), int(rows[len(rows) // 3])


def skewed_rows(rng, length, rows, skew):
    """A row of `rows` per packet, uniform; skewed: about half of the packets on one row and a quarter on a
    second, whose grouped runs then span whole tiles without a head in them."""
    pick = np.asarray(rows)[rng.integers(0, len(rows), length)]
    if skew:
        heavy, second = heavy_rows(rows)
        u = rng.random(length)
        pick = np.where(u < 0.5, heavy, np.where(u < 0.75, second, pick))
    return pick.astype(np.uint32)


def ranks(rows):
    """The rank of each packet among the packets of its row, in array order."""
    rows = np.asarray(rows)
    n = len(rows)
    order = np.argsort(rows, kind="stable")
    s = rows[order]
    first = np.concatenate([[True], s[1:] != s[:-1]])
    run_start = np.maximum.accumulate(np.where(first, np.arange(n), 0))
    r = np.empty(n, np.int64)
    r[order] = np.arange(n) - run_start
    return r


def pooled(seed, length, nwin, pool):
    """interleaved's traffic over `pool` of nwin window rows (pool_rows), drawn uniformly."""
    rng = np.random.default_rng(seed)
    rows = pool_rows(rng, nwin, pool)
    W = pool_windows(nwin, rows, seed)
    return (W,) + _mix(rng, length, W, rows)


def strided(seed, length, nwin, pool, skew, mixed=False):
    """The order-sensitive batch: the packet of rank r (array order) within window w carries L0_w + 1 + STRIDE r
    and status OK, so a stable grouping accepts every packet and any two packets of a window taken in the wrong
    order reject the earlier one (it is STRIDE >= WINDOW behind by then).
    mixed: every packet with i % 7 == 3 is a DECRYPT_ERR, and every packet with i % 11 == 5 repeats the
    counter of the packet ahead of it in its window."""
    rng = np.random.default_rng(seed)
    rows = pool_rows(rng, nwin, pool)
    W = pool_windows(nwin, rows, seed)
    widx = skewed_rows(rng, length, rows, skew)
    r = ranks(widx)
    sts = np.full(length, OK, np.uint8)
    if mixed:
        i = np.arange(length)
        sts[i % 7 == 3] = ERR
        r = r - ((i % 11 == 5) & (r > 0))
    return W, widx, W[widx, 32] + np.uint64(1) + (STRIDE * r).astype(np.uint64), sts


BOUNDARY_RUNS = (8, 9, 47, 448, 1536, 2048, 3)


def sorted_boundaries(neutral_heads=True):
    """Sorted windows whose runs begin at 0, 8, 17, 64, 512, 2048 and 4096: on a lane's first packet of the
    commit's walk (8 consecutive packets a lane), inside a lane, on a wave's first packet and on a tile's.
    Counters as in `strided`, each run's last packet repeating the one ahead of it.
    neutral_heads: each run's first packet has status INVALID, so the head of every row is a neutral element
    (else it is OK and judged against its own window alone)."""
    widx = np.repeat(np.arange(len(BOUNDARY_RUNS), dtype=np.uint32), BOUNDARY_RUNS)
    W = pool_windows(len(BOUNDARY_RUNS), np.arange(len(BOUNDARY_RUNS)), 3)
    r = ranks(widx)
    ends = np.cumsum(BOUNDARY_RUNS) - 1
    r[ends] -= 1
    sts = np.full(len(widx), OK, np.uint8)
    if neutral_heads:
        sts[ends - np.array(BOUNDARY_RUNS) + 1] = INVALID
    return W, widx, W[widx, 32] + np.uint64(1) + (STRIDE * r).astype(np.uint64), sts


def same_counter(n=3000):
    """One window, one counter: [ERR, ERR, OK, OK, ...] with every fifth packet ERR.  Only the first OK packet
    stays OK; every later OK packet finds it in the (window, counter) table, all of them in one slot."""
    sts = np.full(n, OK, np.uint8)
    sts[:2] = ERR
    sts[::5] = ERR
    return live(10_000, 7)[None, :], np.zeros(n, np.uint32), np.full(n, 10_005, np.uint64), sts


def _large():
    out = {}
    for n, nwin, pool in LARGE_SIZES:
        out[f"pooled-{n}-{nwin}"] = lambda n=n, nwin=nwin, pool=pool: pooled(11, n, nwin, pool)
        out[f"strided-{n}-{nwin}"] = lambda n=n, nwin=nwin, pool=pool: strided(12, n, nwin, pool, True)
        out[f"strided_mixed-{n}-{nwin}"] = lambda n=n, nwin=nwin, pool=pool: strided(13, n, nwin, pool, True, True)
    n, nwin, pool = CARRY_SIZE
    out[f"strided-{n}-{nwin}"] = lambda: strided(14, n, nwin, pool, True)
    out["sorted_boundaries"] = sorted_boundaries
    out["sorted_boundaries_judged_heads"] = lambda: sorted_boundaries(neutral_heads=False)
    out["same_counter"] = same_counter
    return out


_LARGE = _large()
LARGE_NAMES = tuple(_LARGE)


@functools.lru_cache(maxsize=None)
def large_case(name):
    """(windows, win_idx, counters, status) of the named case; built once, not to be written to."""
    case = _LARGE[name]()
    for a in case:
        a.setflags(write=False)
    return case
