"""The device-resident session timers, the part that needs no GPU: the ABI surface (header, both libraries, ctypes
table, source list), the layout of rg_session_timer and the constants, rg_timer_workspace_size, the argument rules
that are checked before the device is touched, and the sequential model (tests/timer_cases.py) against hand-written
expectations, one case per line of the loops."""
import ctypes
import os
import re
import subprocess
import textwrap

import timer_cases as tc
from conftest import REPO
from rustyguard_amd import _lib, build, session, timers

NAMES = ("rg_timer_workspace_size", "rg_timer_arm_batch_dev", "rg_timer_note_send_batch_dev",
         "rg_timer_note_recv_batch_dev", "rg_timer_turn_dev")
EINVAL = -1
NOW = 10**12
OK, REJ, SKIP, NONE = tc.OK, tc.REJECTED, tc.SKIP, tc.NONE
FRESH = (0, NOW - 9, NOW - 9)  # a send state no rule fires on


def test_header_libraries_and_binding_have_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "rg_aead.h")).read(), flags=re.S)
    build.build()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _lib.SIGNATURES
        for path in (build.LIB, build.TEST_LIB):
            out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
            assert f" T {name}\n" in out, (name, path)
    assert re.search(r"#define\s+RG_ABI_VERSION\s+6\b", text)  # additive: the version stays
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [2, 9, 9, 9, 11]
    assert "rg_timers.hip" in build.KERNELS and "rg_timers.hip" not in build.HOST
    for unit in build.HOST:
        assert "rg_timer_" not in open(os.path.join(build.CSRC, unit)).read(), unit


def test_timer_layout_and_constants_with_gcc(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "rg_aead.h"
        int main(void) {
            printf("%zu %zu %zu %zu %zu %u\\n", sizeof(rg_session_timer), _Alignof(rg_session_timer),
                   offsetof(rg_session_timer, rekey_at_ns), offsetof(rg_session_timer, flags),
                   offsetof(rg_session_timer, pad), RG_TIMER_KEEPALIVE_PENDING);
            printf("%llu %llu %llu %llu %llu\\n", RG_KEEPALIVE_TIMEOUT_NS, RG_REKEY_AFTER_TIME_NS,
                   RG_REJECT_AFTER_TIME_NS, RG_REKEY_AFTER_MESSAGES, RG_REJECT_AFTER_MESSAGES);
            return 0;
        }
    """))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                   check=True)
    vals = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert vals[:6] == [16, 8, 0, 8, 12, 1]
    assert vals[6:] == [10 * 10**9, 120 * 10**9, 180 * 10**9, 1 << 60, (1 << 64) - 1 - (1 << 13)]
    T = timers.TimerStruct
    assert (ctypes.sizeof(T), T.rekey_at_ns.offset, T.flags.offset, T.pad.offset) == (16, 0, 8, 12)
    assert timers.TIMER_BYTES == 16 and timers.KEEPALIVE_PENDING == tc.PENDING_FLAG == 1
    assert (timers.KEEPALIVE_TIMEOUT_NS, timers.REKEY_AFTER_TIME_NS, timers.REJECT_AFTER_TIME_NS) == \
        (tc.KEEPALIVE_NS, tc.REKEY_NS, tc.REJECT_NS) == tuple(vals[6:9])
    assert (tc.REKEY_MSGS, tc.REJECT_MSGS) == tuple(vals[9:])


def test_workspace_size_is_monotone_and_refuses_absurd_sizes():
    size = _lib.lib().rg_timer_workspace_size
    sizes = [0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 4099, 65536, 1 << 20, (1 << 31) + 1, (1 << 32) - 1]
    for k in sizes:
        col = [size(k, p) for p in sizes]
        assert all(a <= b for a, b in zip(col, col[1:])) and col[0] >= 256, (k, col)
        assert all(c % 256 == 0 for c in col)
    for p in sizes:
        row = [size(k, p) for k in sizes]
        assert all(a <= b for a, b in zip(row, row[1:])), (p, row)
    assert size(1 << 32, 4) == 0 and size(4, 1 << 32) == 0 and size((1 << 64) - 1, 0) == 0 and size(0, (1 << 63) + 5) == 0
    # two want words per peer, and twelve bytes of aggregates per tile of 2048 peers
    assert size(0, 4099) >= 4099 * 8 + 3 * 12 and size(0, (1 << 32) - 1) > 8 * ((1 << 32) - 1)


def test_calls_refuse_a_null_context_before_anything_else():
    L = _lib.lib()
    t = session.TablesStruct()
    assert L.rg_timer_arm_batch_dev(None, None, 0, None, None, 1, None, 0, None) == EINVAL
    assert L.rg_timer_note_send_batch_dev(None, None, 0, None, None, None, 1, None, None) == EINVAL
    assert L.rg_timer_note_recv_batch_dev(None, None, None, 0, None, None, 1, None, None) == EINVAL
    assert L.rg_timer_turn_dev(None, ctypes.byref(t), None, None, None, None, None, None, None, 0, None) == EINVAL
    assert L.rg_timer_arm_batch_dev(None, None, 0, None, None, 0, None, 0, None) == EINVAL  # also with n == 0


# ---------------------------------------------------------------- the model
def test_model_arm_sets_the_whole_row():
    t = [(7, 0x11, 9)] * 5
    got = tc.arm_loop(t, [1, 3, 5, SKIP, 4], [OK, REJ, OK, OK, OK], NOW, tc.REKEY_NS)
    assert got == [(7, 0x11, 9), (NOW + tc.REKEY_NS, 0, 0), (7, 0x11, 9), (7, 0x11, 9), (NOW + tc.REKEY_NS, 0, 0)]
    assert tc.arm_loop(t, [0], None, NOW, 0)[0] == (0, 0, 0)  # a session we responded to: no rekey entry; no gate
    assert tc.arm_loop(t, [0], [OK], (1 << 64) - 5, 9)[0] == (4, 0, 0)  # the add wraps


def test_model_note_send():
    t = [(0, 0, 0), (NOW + 1, 1, 2), (NOW, 0, 0), (NOW - 1, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)]
    slots = [0, 1, 2, 3, 4, 5, 0, 7, SKIP]
    status = [OK, OK, OK, OK, REJ, OK, OK, OK, OK]
    rekey = [1, 200, 1, 1, 1, 0, 1, 1, 1]
    got = tc.note_send_loop(t, slots, status, rekey, NOW)
    # unarmed and later entries become now; now and earlier stay; a rejected packet and one below the limit note nothing
    assert got == [(NOW, 0, 0), (NOW, 1, 2), (NOW, 0, 0), (NOW - 1, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)]
    assert tc.note_send_loop([(0, 0, 0), (5, 0, 0)], [0, 1], [OK, OK], [1, 1], 0) == [(0, 0, 0), (0, 0, 0)]  # a clock of 0


def test_model_note_recv_at_the_keepalive_deadline():
    state = [(0, 0, NOW - tc.KEEPALIVE_NS - 1 + d) for d in range(3)] + [(0, 0, (1 << 64) - 100), FRESH]
    t = [(5, 0x10, 3)] * 5
    got = tc.note_recv_loop(t, state, [0, 1, 2, 3, 4, 0, 9, SKIP], [OK] * 8, NOW)
    assert got == [(5, 0x11, 3), (5, 0x10, 3), (5, 0x10, 3), (5, 0x11, 3), (5, 0x10, 3)]  # strict <; the sum wraps
    assert tc.note_recv_loop(t, state, [0, 3], [REJ, 1], NOW) == t  # only RG_PKT_OK packets


def _turn(rows, peer_slot, timer_rows, now=NOW):
    return tc.turn_loop(tc.tables(rows, peer_slot), timer_rows, now)


def test_model_turn_with_nothing_armed_lists_nothing():
    got = _turn([(0,) + FRESH, (1,) + FRESH], [0, 1], [(0, 0, 0), (NOW + 1, 0x10, 7)])
    assert got == ([(0, 0, 0), (NOW + 1, 0x10, 7)], [SKIP, SKIP], [NONE, NONE], [REJ, REJ], [0, 0])
    assert tc.turn_loop(tc.tables([], []), [], NOW) == ([], [], [], [], [0, 0])


def test_model_turn_free_rows_and_peers_past_the_table_are_not_touched():
    old = (0, NOW - tc.REKEY_NS - 5, 5)
    got = _turn([(NONE,) + old, (2,) + old, (0,) + old], [2, SKIP], [(1, 1, 0)] * 3)
    assert got[0] == [(1, 1, 0), (1, 1, 0), (0, 0, 0)]
    assert got[1:] == ([2, SKIP], [0, NONE], [OK, REJ], [1, 1])


def test_model_turn_keepalive_at_each_instant():
    """sent_ns + 10 s against now, one below, at and one above; the flag is cleared whatever the answer"""
    for d, due in ((-1, True), (0, False), (1, False)):
        row = (0, 0, NOW - 9, NOW - tc.KEEPALIVE_NS + d)
        got = _turn([row], [0], [(0, 0x11, 4)])
        assert got == ([(0, 0x10, 4)], [0 if due else SKIP], [NONE], [REJ], [1 if due else 0, 0]), d
    # without the flag a silent session asks for nothing
    assert _turn([(0, 0, NOW - 9, 5)], [0], [(0, 0x10, 0)])[4] == [0, 0]


def test_model_turn_rekey_entry_at_each_instant():
    """rekey_at_ns against now: one below fires (and is popped), at and one above stay armed"""
    old = (0, 0, NOW - tc.REKEY_NS - 1, NOW - 9)
    for d, fires in ((-1, True), (0, False), (1, False)):
        got = _turn([old], [0], [(NOW + d, 0, 0)])
        assert got[0] == [(0 if fires else NOW + d, 0, 0)] and got[2:] == ([0 if fires else NONE], [OK if fires else REJ],
                                                                           [0, 1 if fires else 0]), d
    assert _turn([old], [0], [(0, 0, 0)])[4] == [0, 0]  # 0 is not armed, however old the session


def test_model_turn_should_rekey_at_each_instant_and_counter():
    """a fired entry is popped whether or not the session needs a rekey: started_ns + 120 s one below, at and one
    above now; the counter at 2^60 - 1 and 2^60; a start whose sum wraps"""
    for started, counter, want in ((NOW - tc.REKEY_NS - 1, 0, 1), (NOW - tc.REKEY_NS, 0, 0), (NOW - tc.REKEY_NS + 1, 0, 0),
                                   (NOW - 9, tc.REKEY_MSGS - 1, 0), (NOW - 9, tc.REKEY_MSGS, 1),
                                   ((1 << 64) - 100, 0, 1)):
        got = _turn([(0, counter, started, NOW - 9)], [0], [(NOW - 1, 0, 0)])
        assert got[0] == [(0, 0, 0)] and got[4] == [0, want], (started, counter)
        assert got[2] == [0 if want else NONE] and got[3] == [OK if want else REJ]


def test_model_turn_keepalive_goes_out_on_the_current_row_unless_it_rejects():
    """two live rows of one peer, the old one pending: the keepalive names the current row, whose own sent_ns is
    not asked; should_reject of that row at each instant, at REJECT - 1 and REJECT, and with a wrapping start"""
    silent = (0, 0, NOW - 9, NOW - tc.KEEPALIVE_NS - 1)
    for started, counter, sends in ((NOW - tc.REJECT_NS - 1, 0, 0), (NOW - tc.REJECT_NS, 0, 1), (NOW - tc.REJECT_NS + 1, 0, 1),
                                    (NOW - 9, tc.REJECT_MSGS - 1, 1), (NOW - 9, tc.REJECT_MSGS, 0),
                                    ((1 << 64) - 100, 0, 0)):
        got = _turn([silent, (0, counter, started, NOW - 1)], [1], [(0, 1, 0), (0, 0, 0)])
        assert got[0] == [(0, 0, 0)] * 2 and got[1] == [1 if sends else SKIP] and got[4] == [sends, 0], (started, counter)
    # both pending and silent: one keepalive for the peer
    got = _turn([silent, silent], [1], [(0, 1, 0), (0, 1, 0)])
    assert got[1] == [1] and got[4] == [1, 0]


def test_model_turn_peer_whose_current_row_is_free_or_names_another_peer():
    silent = (0, 0, NOW - 9, 5)
    for peer_slot in ([1, SKIP], [2, SKIP], [7, SKIP], [SKIP, SKIP]):
        got = _turn([silent, (NONE, 0, 0, 0), (1,) + FRESH], peer_slot, [(0, 1, 0)] * 3)
        assert got[0] == [(0, 0, 0), (0, 1, 0), (0, 0, 0)] and got[1] == [SKIP, SKIP] and got[4] == [0, 0], peer_slot


def test_model_turn_lists_are_ascending_by_peer_and_padded():
    """rows in an order unlike their peers'; peer 3 has two due rows; peer 1 nothing; every decision on the state
    before the turn"""
    due = (0, NOW - tc.REKEY_NS - 1, NOW - tc.KEEPALIVE_NS - 1)
    rows = [(3,) + due, (0,) + due, (2,) + FRESH, (3,) + due, (1,) + FRESH, (2,) + due]
    got = _turn(rows, [1, 4, 2, 0, SKIP], [(NOW - 1, 1, 0)] * 6)
    assert got[0] == [(0, 0, 0)] * 6  # peer 1's flag and entry are taken too, and ask for nothing
    assert got[1] == [1, 2, 0, SKIP, SKIP] and got[2] == [0, 2, 3, NONE, NONE]
    assert got[3] == [OK, OK, OK, REJ, REJ] and got[4] == [3, 3]
    again = tc.turn_loop(tc.tables(rows, [1, 4, 2, 0, SKIP]), got[0], NOW)
    assert again == (got[0], [SKIP] * 5, [NONE] * 5, [REJ] * 5, [0, 0])  # the same clock twice


def test_random_cases_cover_what_they_claim():
    t, tm = tc.random_case(4099, 4099, 3)
    got = tc.turn_loop(t, tm, NOW)
    assert 100 < got[4][0] < 4099 and 100 < got[4][1] < 4099
    assert {r // tc.TILE for r in got[1] if r != SKIP} >= {0, 1} and {p // tc.TILE for p in got[2] if p != NONE} >= {0, 1}
    assert any(p != NONE and p >= 4099 for p in t["slot_peer"]) and NONE in t["slot_peer"]
    changed = sum(a != b for a, b in zip(tm, got[0]))
    assert 500 < changed < 4099
    t, tm = tc.due_case(4099, 3, 0.5)
    assert tc.turn_loop(t, tm, NOW)[1:] == ([4098, 4096, 4097], [0, 1, 2], [OK] * 3, [3, 3])
