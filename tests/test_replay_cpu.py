"""Device-resident anti-replay, the part that needs no GPU: the ABI surface (header, both libraries, ctypes
table), rg_replay_workspace_size, and the closed form the kernels implement ("Device-resident
anti-replay") restated in numpy and checked against the host rg_antireplay_* functions on the very cases
test_gpu_replay.py runs on the device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import replay_cases as rc
from conftest import REPO
from rustyguard_amd import _lib, build

NAMES = ("rg_replay_workspace_size", "rg_replay_batch_dev", "rg_recv_batch_dev_resident")


def test_header_libraries_and_binding_have_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "rg_aead.h")).read(), flags=re.S)
    build.build()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _lib.SIGNATURES
        for path in (build.LIB, build.TEST_LIB):
            out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
            assert f" T {name}\n" in out, (name, path)
    assert re.search(r"#define\s+RG_ABI_VERSION\s+6\b", text)


def test_workspace_size():
    size = _lib.lib().rg_replay_workspace_size
    assert size(1, 1) > 0
    assert size(1 << 63, 1) == 0
    for nwin in (0, 1, 2, 256, 257, 65536, 65537, 0xFFFFFFFF):
        sizes = [size(n, nwin) for n in (0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 65536, 1 << 20, (1 << 32) - 1)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (nwin, sizes)
    for n in (1, 1000, 1 << 20):
        sizes = [size(n, nwin) for nwin in (0, 1, 2, 3, 255, 256, 257, 65536, 65537, 1 << 24, (1 << 24) + 1, 0xFFFFFFFF)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (n, sizes)
    assert size(1 << 32, 1) == 0  # n > 2^32 - 1 is refused by the calls
    # the layout's bytes, pinned: (n, nwin) with no, one, two and three radix passes
    pinned = {(0, 0): 256, (1, 1): 2560, (2049, 2): 156160, (2049, 257): 164608, (65536, 256): 4358656,
              (1 << 20, 65537): 73930752, ((1 << 32) - 1, 257): 302820360192}
    assert {k: size(*k) for k in pinned} == pinned


def closed_form(windows, win_idx, counters, status):
    """The closed form of the sequential rule, window by window: a prefix maximum, three rejection tests, the
    final bitmap from the starting one and the accepted bits.  No window state is carried from packet to
    packet."""
    W = np.array(windows, np.uint64).copy()
    st = np.array(status, np.uint8).copy()
    undo = np.zeros(len(st), np.uint8)
    win_idx = np.asarray(win_idx, np.uint32)
    part = (win_idx != rc.SKIP) & (win_idx < len(W)) & (st <= rc.ERR)
    for w in np.unique(win_idx[part]):
        idx = np.nonzero(part & (win_idx == w))[0]  # the window's packets, in array order
        c = np.asarray(counters, np.uint64)[idx]
        ok = st[idx] == rc.OK
        L0 = np.uint64(W[w, 32])
        bm0 = W[w, :32].copy()
        incl = np.maximum.accumulate(np.maximum(np.where(ok, c, np.uint64(0)), L0))
        M = np.concatenate([[L0], incl[:-1]]).astype(np.uint64)  # last before each packet
        behind = c <= M
        too_old = behind & ((M - np.minimum(c, M)) >= np.uint64(rc.WINDOW))
        blk = c >> np.uint64(6)
        bit0 = (bm0[(blk & np.uint64(31)).astype(np.int64)] >> (c & np.uint64(63))) & np.uint64(1)
        seen0 = behind & (blk <= (L0 >> np.uint64(6))) & (bit0 == 1)
        first_ok, dup = {}, np.zeros(len(idx), bool)
        for k in range(len(idx)):
            if int(c[k]) in first_ok:
                dup[k] = True
            elif ok[k]:
                first_ok[int(c[k])] = k
        rej = too_old | seen0 | dup
        undo[idx] = rej & ok
        st[idx[rej]] = rc.REJECTED
        Lf = int(incl[-1])
        bf, b0 = Lf >> 6, int(L0) >> 6
        new = [0] * 32
        for s in range(32):
            j = bf - ((bf - s) & 31)  # the block slot s holds at the end
            if j <= b0:
                new[s] = int(bm0[s])
        for k in np.nonzero(ok & ~rej)[0]:
            j = int(c[k]) >> 6
            if bf - j < 32:
                new[j & 31] |= 1 << (int(c[k]) & 63)
        W[w, :32] = np.array(new, np.uint64)
        W[w, 32] = Lf
    return st, undo, W


def _same(case):
    W, widx, ctrs, sts = case
    st_h, undo_h, W_h, _ = rc.host_commit(W, widx, ctrs, sts)
    st_c, undo_c, W_c = closed_form(W, widx, ctrs, sts)
    assert np.array_equal(st_c, st_h)
    assert np.array_equal(undo_c, undo_h)
    assert np.array_equal(W_c, W_h)
    return st_h


def test_closed_form_reference_sequence():
    seq = rc.reference_sequence()
    z = np.zeros(len(seq), np.uint32)
    st = _same((rc.fresh(), z, seq, np.zeros(len(seq), np.uint8)))
    assert (st[-5:] == [rc.OK, rc.REJECTED, rc.OK, rc.REJECTED, rc.OK]).all()
    # split into batches: each batch's closed form starts from the host's window
    for size in (64, 1):
        Wc, Wh = rc.fresh(), rc.fresh()
        for at in range(0, len(seq) if size == 64 else 600, size):
            part = seq[at:at + size]
            zz = np.zeros(len(part), np.uint32)
            sh, uh, Wh, _ = rc.host_commit(Wh, zz, part, np.zeros(len(part), np.uint8))
            sc, uc, Wc = closed_form(Wc, zz, part, np.zeros(len(part), np.uint8))
            assert np.array_equal(sc, sh) and np.array_equal(uc, uh) and np.array_equal(Wc, Wh), at


def test_closed_form_unauthenticated_high_counter():
    st = _same((rc.fresh(), np.zeros(3, np.uint32), np.array([5, 1_000_000, 6], np.uint64),
                np.array([rc.OK, rc.ERR, rc.OK], np.uint8)))
    assert list(st) == [rc.OK, rc.ERR, rc.OK]


@pytest.mark.parametrize("case", rc.edge_cases(), ids=lambda c: c[0])
def test_closed_form_edges(case):
    name, win, ctrs, sts = case
    st = _same((win[None, :], np.zeros(len(ctrs), np.uint32), ctrs, sts))
    if name.startswith("err_ok_ok_err"):
        assert list(st) == [rc.ERR, rc.OK, rc.REJECTED, rc.REJECTED]


@pytest.mark.parametrize("length", rc.INTERLEAVED_LENGTHS)
@pytest.mark.parametrize("seed", range(4))
def test_closed_form_interleaved(seed, length):
    case = rc.interleaved(seed, length)
    _same(case)
    if length >= 257:
        shares = rc.class_shares(rc.host_commit(*case)[3])
        print(f"seed {seed} length {length}: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))
        assert min(shares.values()) >= rc.MIN_SHARE, shares
    W, widx, ctrs, sts = case
    if length >= 63:  # the untouched kinds are all there
        assert (widx == rc.SKIP).any() or (widx >= len(W)).any() or (sts > rc.ERR).any()


def test_closed_form_many_windows():
    _same(rc.many_windows())


# ---- the cases that run the grouped scan's loops more than once (replay_cases.large_case)
@pytest.fixture(scope="module")
def model():
    """name -> host_commit's result, computed once per case."""
    done = {}

    def get(name):
        if name not in done:
            done[name] = rc.host_commit(*rc.large_case(name))
        return done[name]

    return get


@pytest.mark.parametrize("name", rc.LARGE_NAMES)
def test_closed_form_large(model, name):
    W, widx, ctrs, sts = rc.large_case(name)
    st_h, undo_h, W_h, _ = model(name)
    st_c, undo_c, W_c = closed_form(W, widx, ctrs, sts)
    assert np.array_equal(st_c, st_h) and np.array_equal(undo_c, undo_h) and np.array_equal(W_c, W_h)


def _loops(n, nrows):
    """(tiles, radix passes, entries a lane of the radix scan, tiles a lane of the carry) of a batch: the
    arithmetic of csrc/rg_grouped.h restated."""
    nblk = -(-n // rc.TILE)
    passes = 0 if nrows <= 1 else -(-(nrows - 1).bit_length() // 8)
    return nblk, passes, -(-256 * nblk // 1024), -(-nblk // 256)


def test_large_sizes_reach_their_loops():
    assert [_loops(n, nwin) for n, nwin, _ in rc.LARGE_SIZES] == [(3, 2, 1, 1), (5, 2, 2, 1), (10, 3, 3, 1)]
    assert _loops(*rc.CARRY_SIZE[:2]) == (257, 2, 65, 2)
    # each is the smallest: one packet or one row fewer and the loop named in replay_cases runs once less
    assert _loops(4096, 257)[0] == 2 and _loops(4097, 256)[1] == 1
    assert _loops(8192, 300)[2] == 1
    assert _loops(18433, 65536)[1] == 2
    assert _loops(524288, 300)[3] == 1
    # 18433 is the first size whose scan, at three entries a lane, ends on a lane holding one entry; the
    # carry's last busy lane at 524289 holds one tile
    assert 256 * 10 == 853 * 3 + 1 and _loops(18432, 70000)[2] == 3 and 256 * 9 == 768 * 3
    assert 257 == 128 * 2 + 1
    # what the suite had before: one entry and one tile a lane wherever a radix pass ran
    assert _loops(4100, 3)[1:] == (1, 1, 1) and _loops(8300, 1)[1] == 0


@pytest.mark.parametrize("n,nwin,pool", rc.LARGE_SIZES)
def test_pooled_reaches_every_outcome_and_digit(model, n, nwin, pool):
    name = f"pooled-{n}-{nwin}"
    W, widx, _, sts = rc.large_case(name)
    shares = rc.class_shares(model(name)[3])
    print(f"{name}: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))
    assert min(shares.values()) >= rc.MIN_SHARE, shares
    assert (widx == rc.SKIP).any() and ((widx != rc.SKIP) & (widx >= nwin)).any() and (sts > rc.ERR).any()
    rows = np.unique(widx[widx < nwin])
    assert len(rows) == pool and not W[np.setdiff1d(np.arange(nwin), rows)].any()
    assert set(rows) >= {r for r in (0, 255, 256, 257, 65535, 65536, nwin - 1) if r < nwin}
    for shift in range(0, 8 * _loops(n, nwin)[1], 8):  # every digit a radix pass sorts by: zero and not
        digit = (rows >> shift) & 255
        assert (digit == 0).any() and (digit != 0).any(), shift


def _heavy(widx):
    """(row, packets, whole tiles of its grouped run) of the row with most packets, from the row counts."""
    rows, counts = np.unique(widx, return_counts=True)
    k = int(np.argmax(counts))
    start = int(counts[:k].sum())  # the grouped order is by row, and every packet here has one
    end = start + int(counts[k])
    return int(rows[k]), int(counts[k]), max(0, end // rc.TILE - -(-start // rc.TILE))


@pytest.mark.parametrize("n,nwin,pool", rc.LARGE_SIZES + (rc.CARRY_SIZE,))
def test_strided_is_order_sensitive(model, n, nwin, pool):
    name = f"strided-{n}-{nwin}"
    W, widx, ctrs, sts = rc.large_case(name)
    st, undo, _, _ = model(name)
    assert (sts == rc.OK).all() and (st == rc.OK).all() and not undo.any()
    row, count, tiles = _heavy(widx)
    print(f"{name}: row {row} holds {count} packets, {tiles} whole tiles of the grouped order")
    assert tiles >= {8193: 1, 524289: 100}.get(n, 0)
    # two neighbouring packets of the heavy window the other way round: the model rejects the later one
    mine = np.nonzero(widx == row)[0][:64]
    c = ctrs[mine].copy()
    c[[30, 31]] = c[[31, 30]]
    st2 = rc.host_commit(W, widx[mine], c, sts[mine])[0]
    assert list(np.nonzero(st2 == rc.REJECTED)[0]) == [31]


@pytest.mark.parametrize("n,nwin,pool", rc.LARGE_SIZES)
def test_strided_mixed_outcomes(model, n, nwin, pool):
    name = f"strided_mixed-{n}-{nwin}"
    _, widx, _, sts = rc.large_case(name)
    shares = rc.class_shares(model(name)[3])
    print(f"{name}: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))
    assert shares["accepted"] > 0.7 and shares["duplicate"] > 0.05 and shares["bad_tag_kept"] > 0.1
    assert shares["too_old"] == 0  # nothing is out of order in the array
    assert _heavy(widx)[2] >= (1 if n >= 8193 else 0)


def test_sorted_boundaries_and_same_counter_shapes(model):
    for name, head in (("sorted_boundaries", rc.INVALID), ("sorted_boundaries_judged_heads", rc.OK)):
        _, widx, ctrs, sts = rc.large_case(name)
        heads = np.nonzero(np.concatenate([[True], widx[1:] != widx[:-1]]))[0]
        assert list(heads) == [0, 8, 17, 64, 512, 2048, 4096] and len(widx) == 4099
        st = model(name)[0]
        assert (sts[heads] == head).all() and (st[heads] == head).all()
        tails = np.concatenate([heads[1:], [len(widx)]]) - 1
        assert (st[tails] == rc.REJECTED).all() and (ctrs[tails] == ctrs[tails - 1]).all()
        rest = np.setdiff1d(np.arange(len(widx)), np.concatenate([heads, tails]))
        assert (st[rest] == rc.OK).all()
        if head == rc.OK:
            # a head judged against the maximum of the row ahead of it, not against its own window alone, would
            # be too old: that maximum lies above the head's window and WINDOW or more above its counter
            W = rc.large_case(name)[0]
            for k in range(1, len(heads)):
                ahead = int(ctrs[heads[k] - 1])
                assert ahead > int(W[k, 32]) and ahead - int(ctrs[heads[k]]) >= rc.WINDOW, k
    _, _, _, sts = rc.large_case("same_counter")
    st = model("same_counter")[0]
    assert list(sts[:7]) == [rc.ERR, rc.ERR, rc.OK, rc.OK, rc.OK, rc.ERR, rc.OK]
    assert list(st[:3]) == [rc.ERR, rc.ERR, rc.OK] and (st[3:] == rc.REJECTED).all() and len(st) == 3000
