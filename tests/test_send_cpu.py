"""Device-resident send, the part that needs no GPU: the ABI surface (header, both libraries, ctypes table),
sizeof(rg_send_state), rg_send_workspace_size, and the closed form the kernels implement (DESIGN.md,
"Device-resident send") restated in numpy and checked against the array-order loop on the very cases
test_gpu_send_reserve.py runs on the device."""
import os
import re
import subprocess
import textwrap

import numpy as np
import pytest

import send_cases as sc
from conftest import REPO
from rustyguard_amd import _lib, build

NAMES = ("rg_send_workspace_size", "rg_send_reserve_batch_dev", "rg_send_batch_dev_resident")
CASES = sc.cases()


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
    assert len(_lib.SIGNATURES["rg_send_reserve_batch_dev"][1]) == 13
    assert len(_lib.SIGNATURES["rg_send_batch_dev_resident"][1]) == 17


def test_send_state_layout_with_gcc(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "rg_aead.h"
        int main(void) {
            printf("%zu %zu %zu %zu\\n", sizeof(rg_send_state), offsetof(rg_send_state, counter),
                   offsetof(rg_send_state, started_ns), offsetof(rg_send_state, sent_ns));
            return 0;
        }
    """))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                   check=True)
    vals = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert vals == [24, 0, 8, 16]


def test_workspace_size():
    size = _lib.lib().rg_send_workspace_size
    assert size(1, 1) > 0
    assert size(1 << 32, 1) == 0  # n > 2^32 - 1 is refused by the calls
    assert size(1 << 63, 1) == 0
    for nkeys in (0, 1, 2, 256, 257, 65536, 65537, 0xFFFFFFFF):
        sizes = [size(n, nkeys) for n in (0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 65536, 1 << 20, (1 << 32) - 1)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (nkeys, sizes)
        assert sizes[1] > 0 and sizes[-1] > 0
    for n in (1, 1000, 1 << 20):
        sizes = [size(n, nkeys) for nkeys in (0, 1, 2, 3, 255, 256, 257, 65536, 65537, 1 << 24, (1 << 24) + 1, 0xFFFFFFFF)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (n, sizes)
    assert size(4097, 3) >= 4097 * 16  # the working descriptors alone
    # the layout's bytes, pinned: (n, nkeys) with no, one, two and three radix passes
    pinned = {(0, 0): 256, (1, 1): 1536, (2049, 2): 71424, (2049, 257): 79872, (65536, 256): 2195968,
              (1 << 20, 65537): 39325696, ((1 << 32) - 1, 257): 161078050816}
    assert {k: size(*k) for k in pinned} == pinned


def closed_form(state, slots, lens, now):
    """The closed form of the loop, row by row: no state is carried from packet to packet.  Ranks are compared
    with REJECT - C0; C0 + rank is formed only where it cannot wrap."""
    S = np.array(state, np.uint64).reshape(-1, 3).copy()
    slots = np.asarray(slots, np.uint32)
    lens = np.asarray(lens, np.uint32)
    n, nkeys = len(slots), len(S)
    valid = (slots != sc.SKIP) & (slots < nkeys)
    status = np.full(n, sc.REJECTED, np.uint8)
    status[valid & (lens % 16 != 0)] = sc.INVALID
    counters, rekey = np.zeros(n, np.uint64), np.zeros(n, np.uint8)
    row = np.where(valid, slots, 0)
    if now is None:
        expired = np.zeros(nkeys, bool)
    else:
        with np.errstate(over="ignore"):
            expired = (S[:, 1] + np.uint64(sc.REJECT_AFTER_TIME)) < np.uint64(now)  # wrapping, as the host
    elig = valid & (lens % 16 == 0) & ~expired[row]
    for w in np.unique(row[elig]):
        idx = np.nonzero(elig & (row == w))[0]  # E, in array order
        C0 = int(S[w, 0])
        room = sc.REJECT - C0 if C0 < sc.REJECT else 0
        r = np.arange(len(idx), dtype=np.uint64)  # rank in E
        take = r < np.uint64(room) if room else np.zeros(len(idx), bool)
        got = idx[take]
        counters[got] = np.uint64(C0) + r[take]
        rekey[got] = (counters[got] + np.uint64(1)) >= np.uint64(sc.REKEY)
        status[got] = sc.PENDING
        took = min(len(idx), room)
        if took:
            S[w, 0] = C0 + took
            if now is not None:
                S[w, 2] = now
    return status, counters, rekey, S


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_closed_form_equals_the_loop(case):
    _, state, slots, lens, now = case
    st, ctr, rk, S = sc.loop(state, slots, lens, now)
    st_c, ctr_c, rk_c, S_c = closed_form(state, slots, lens, now)
    assert np.array_equal(st_c, st), np.nonzero(st_c != st)[0][:10]
    assert np.array_equal(ctr_c, ctr) and np.array_equal(rk_c, rk)
    assert np.array_equal(S_c, S)


def test_cases_reach_their_edges():
    """What each named case is there for, read off the loop's own output."""
    by = {c[0]: (c, sc.loop(*c[1:])) for c in CASES}
    assert list(by["rekey_edge"][1][2]) == sc.expect_rekey_edge()
    st, ctr, _, S = by["reject_edge_5"][1]
    assert list(st) == [sc.PENDING] * 3 + [sc.REJECTED] * 2 and int(S[0, 0]) == sc.REJECT
    st, ctr, _, S = by["reject_edge_8300"][1]
    assert (st[:3] == sc.PENDING).all() and (st[3:] == sc.REJECTED).all() and int(S[0, 0]) == sc.REJECT
    for name in ("at_reject", "past_reject", "counter_max"):
        (_, state, *_), (st, _, _, S) = by[name]
        assert (st == sc.REJECTED).all() and np.array_equal(S, state)
    st, ctr, _, S = by["carry_high_word"][1]
    assert int(ctr[1]) == (1 << 32) - 1 and int(ctr[2]) == 1 << 32 and int(S[0, 0]) == (1 << 32) + 68
    (_, state, slots, _, now), (st, _, _, S) = by["times"]
    assert (st[slots == 0] == sc.PENDING).all() and (st[slots == 1] == sc.REJECTED).all()
    assert (st[slots == 2] == sc.PENDING).all() and (st[slots == 3] == sc.REJECTED).all()
    assert list(S[:, 2]) == [now, 2, now, 4, 5]  # sent_ns moves only where a counter was taken
    (_, state, *_), (st, _, _, S) = by["times_no_clock"]
    assert (st == sc.PENDING).all() and np.array_equal(S[:, 1:], state[:, 1:])
    (_, _, slots, lens, _), (st, _, _, _) = by["ineligible_3rows_700"]
    assert {sc.PENDING, sc.INVALID, sc.REJECTED} == set(st)
    assert (st[(slots == sc.SKIP) & (lens % 16 != 0)] == sc.REJECTED).all()


# ---- the cases that run the grouped scan's loops more than once (send_cases.large_cases)
LARGE = sc.large_cases()


@pytest.fixture(scope="module")
def large_loop():
    """name -> the loop's result, computed once per case."""
    return {c[0]: sc.loop(*c[1:]) for c in LARGE}


@pytest.mark.parametrize("case", LARGE, ids=lambda c: c[0])
def test_closed_form_equals_the_loop_large(large_loop, case):
    name, state, slots, lens, now = case
    st, ctr, rk, S = large_loop[name]
    st_c, ctr_c, rk_c, S_c = closed_form(state, slots, lens, now)
    assert np.array_equal(st_c, st), np.nonzero(st_c != st)[0][:10]
    assert np.array_equal(ctr_c, ctr) and np.array_equal(rk_c, rk)
    assert np.array_equal(S_c, S)


def _loops(n, nrows):
    """(tiles, radix passes, entries a lane of the radix scan, tiles a lane of the carry) of a batch: the
    arithmetic of csrc/rg_grouped.h restated."""
    nblk = -(-n // sc.TILE)
    passes = 0 if nrows <= 1 else -(-(nrows - 1).bit_length() // 8)
    return nblk, passes, -(-256 * nblk // 1024), -(-nblk // 256)


def test_large_sizes_reach_their_loops():
    assert [_loops(n, nkeys) for n, nkeys, _ in sc.LARGE_SIZES] == [(5, 2, 2, 1), (10, 3, 3, 1), (257, 2, 65, 2)]
    assert _loops(8192, 300)[2] == 1 and _loops(18433, 65536)[1] == 2 and _loops(524288, 300)[3] == 1
    assert 256 * 10 == 853 * 3 + 1 and 257 == 128 * 2 + 1  # the last busy lane holds one entry, one tile
    # what the suite had before: no radix pass at 8300 packets, one entry and one tile a lane elsewhere
    assert _loops(8300, 1)[1] == 0 and _loops(4097, 3)[1:] == (1, 1, 1) and _loops(2500, 300)[1:] == (2, 1, 1)


@pytest.mark.parametrize("case", LARGE, ids=lambda c: c[0])
def test_large_cases_stay_meaningful(large_loop, case):
    name, state, slots, lens, _ = case
    st, ctr, _, S = large_loop[name]
    nkeys = len(state)
    valid = (slots != sc.SKIP) & (slots < nkeys)
    rows, counts = np.unique(np.where(valid, slots, 0), return_counts=True)  # the grouping key
    k = int(np.argmax(counts))
    heavy = int(rows[k])
    start = int(counts[:k].sum())
    tiles = (start + int(counts[k])) // sc.TILE - -(-start // sc.TILE)
    took = st == sc.PENDING
    print(f"{name}: {took.mean():.3f} take a counter; row {heavy} holds {counts[k]} packets, {tiles} whole tiles")
    assert tiles >= (100 if len(slots) == 524289 else 1)
    assert {sc.PENDING, sc.INVALID, sc.REJECTED} == set(st)
    assert (slots == sc.SKIP).any() and ((slots != sc.SKIP) & (slots >= nkeys)).any()
    live = np.unique(slots[valid])
    for shift in range(0, 8 * _loops(len(slots), nkeys)[1], 8):  # every digit a radix pass sorts by: zero and not
        assert (((live >> shift) & 255) == 0).any() and (((live >> shift) & 255) != 0).any()
    if name.endswith("reject_edge"):
        # the heavy row shuts 900 counters in, and by design takes most of the batch with it: the share is
        # asked of the other rows
        mine = valid & (slots == heavy)
        assert int(state[heavy, 0]) == sc.REJECT - 900 and int(S[heavy, 0]) == sc.REJECT
        assert took[mine].sum() == 900 and (st[mine] == sc.REJECTED).sum() > 1000
        last = np.nonzero(mine & took)[0][-1]
        assert int(ctr[last]) == sc.REJECT - 1
        # the row's last counter is taken in a later tile of the grouped order than the one its run begins in
        assert heavy != 0 and (start + int(mine[:last].sum())) // sc.TILE > start // sc.TILE
        assert took[~mine].mean() >= 0.8
    else:
        assert took.mean() >= 0.8
