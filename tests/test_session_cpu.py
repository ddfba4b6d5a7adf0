"""The device-resident session table, the part that needs no GPU: the ABI surface (header, both libraries, ctypes
table), the layout of rg_session_tables, RG_PKT_FULL, rg_session_workspace_size, the argument rules that are
checked before the device is touched, and the sequential model (tests/session_cases.py) against hand-written
expectations, one case per line of the loop."""
import ctypes
import os
import re
import subprocess
import textwrap

import numpy as np

import session_cases as sc
from conftest import REPO
from rustyguard_amd import _lib, build, session

NAMES = ("rg_session_workspace_size", "rg_session_install_batch_dev", "rg_session_install_resp_batch_dev",
         "rg_session_install_finish_batch_dev", "rg_session_expire_batch_dev", "rg_session_index_dev")
EINVAL = -1


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
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [3, 14, 13, 16, 9, 3]
    assert "rg_session.hip" in build.KERNELS and "rg_session.hip" not in build.HOST


def test_host_units_name_no_session_launcher():
    for unit in build.HOST:
        assert "rg_session_" not in open(os.path.join(build.CSRC, unit)).read(), unit


def test_tables_layout_and_status_value_with_gcc(tmp_path):
    fields = [name for name, _ in session.TablesStruct._fields_]
    src = tmp_path / "layout.c"
    src.write_text(textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "rg_aead.h"
        int main(void) {
            printf("%%zu %%d %%d", sizeof(rg_session_tables), (int)RG_PKT_FULL, RG_ABI_VERSION);
            %s
            printf("\\n");
            return 0;
        }
    """) % "\n    ".join(f'printf(" %zu", offsetof(rg_session_tables, {f}));' for f in fields))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                   check=True)
    vals = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert vals[:3] == [88, 10, 6]
    assert vals[3:] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76, 80]
    assert ctypes.sizeof(session.TablesStruct) == 88
    assert vals[3:] == [getattr(session.TablesStruct, f).offset for f in fields]
    assert fields == ["send_keys", "recv_keys", "receivers", "local_ids", "slot_peer", "windows", "send_state",
                      "rx_table", "peer_slot", "nkeys", "rx_cap", "npeers"]
    assert session.PKT_FULL == sc.FULL == 10 and session.WINDOW_BYTES == sc.WINDOW == 264


def test_workspace_size_is_monotone_and_refuses_absurd_batches():
    size = _lib.lib().rg_session_workspace_size
    ns = [0, 1, 2, 31, 32, 33, 255, 256, 2047, 2048, 2049, 4099, 65536, 1 << 20, (1 << 31) + 1, (1 << 32) - 1]
    ks = [0, 1, 2, 255, 256, 257, 2048, 2049, 65536, 1 << 20, (1 << 24) + 1, 0xFFFFFFFF]
    for k in ks:
        for p in (0, 1, 0xFFFFFFFF):
            col = [size(n, k, p) for n in ns]
            assert all(a <= b for a, b in zip(col, col[1:])) and col[0] >= 256, (k, p, col)
            assert all(c % 256 == 0 for c in col)
    for n in (0, 1, 4099):
        for p in (0, 7):
            row = [size(n, k, p) for k in ks]
            assert all(a <= b for a, b in zip(row, row[1:])), (n, p, row)
        for k in (0, 9):
            row = [size(n, k, p) for p in ks]
            assert all(a <= b for a, b in zip(row, row[1:])), (n, k, row)
    assert size(1 << 32, 4, 4) == 0 and size((1 << 63) + 5, 1, 1) == 0 and size((1 << 64) - 1, 0, 0) == 0
    # the largest sizes the calls take are computed without overflow: well above what the arrays alone need
    assert size((1 << 32) - 1, 0xFFFFFFFF, 0xFFFFFFFF) > 16 * ((1 << 32) - 1) + 8 * (1 << 32) + 9 * 0xFFFFFFFF
    # three gathered words, a rank and two id entries of 8 bytes per handshake; a free-list word and a mark per row
    assert size(4099, 0, 0) >= 4099 * (16 + 16) and size(0, 4099, 0) >= 4099 * 5 and size(0, 0, 4099) >= 4099 * 4


def test_calls_refuse_a_null_context_before_anything_else():
    L = _lib.lib()
    t = session.TablesStruct()
    tp = ctypes.byref(t)
    assert L.rg_session_install_batch_dev(None, tp, None, None, None, None, None, 1, None, None, None, None, 0, None) == EINVAL
    assert L.rg_session_install_resp_batch_dev(None, tp, None, None, None, None, 1, None, None, None, None, 0, None) == EINVAL
    assert L.rg_session_install_finish_batch_dev(None, tp, None, None, None, None, None, 0, None, 1, None, None, None, None,
                                                 0, None) == EINVAL
    assert L.rg_session_expire_batch_dev(None, tp, None, None, 0, None, None, 0, None) == EINVAL
    assert L.rg_session_index_dev(None, tp, None) == EINVAL
    assert L.rg_session_install_batch_dev(None, None, None, None, None, None, None, 0, None, None, None, None, 0, None) == EINVAL
    assert session.rx_capacity(0) == 2 and session.rx_capacity(1) == 2 and session.rx_capacity(8) == 16
    assert session.rx_capacity(9) == 32 and session.rx_capacity(4099) == 16384


# ---------------------------------------------------------------- the model
def _one(t, rows, now=None, seed=1):
    b = sc.batch(rows, np.random.default_rng(seed))
    return b, sc.install_loop(t, b["gate"], b["local_ids"], b["remote_ids"], b["peers"], b["keys"], now)


def _table_with_one_live_row():
    t = sc.empty_tables(3, 2)
    sc.seed_row(t, 1, 0x77, 0x88, 1, np.random.default_rng(2), started=9)
    return t


def test_model_gated_row_is_rejected_and_untouched():
    t = _table_with_one_live_row()
    b, (after, st, rows, keys) = _one(t, [(sc.REJECTED, 5, 6, 0), (sc.PENDING, 5, 6, 0)])
    assert st == [sc.REJECTED] * 2 and rows == [sc.SKIP] * 2 and keys == b["keys"] and after == t


def test_model_key_row_is_consumed_whatever_follows():
    t = _table_with_one_live_row()
    b, (after, st, rows, keys) = _one(t, [(sc.OK, 5, 6, 2), (sc.OK, 0x77, 6, 0), (sc.OK, 9, 6, 0), (sc.OK, 10, 6, 0),
                                          (sc.OK, 11, 6, 0)])
    assert st == [sc.INVALID, sc.REJECTED, sc.OK, sc.OK, sc.FULL] and keys == [bytes(64)] * 5


def test_model_peer_past_the_table_is_invalid():
    b, (after, st, rows, _) = _one(sc.empty_tables(2, 2), [(sc.OK, 5, 6, 2), (sc.OK, 7, 8, sc.NONE)])
    assert st == [sc.INVALID] * 2 and rows == [sc.SKIP] * 2 and after == sc.empty_tables(2, 2)


def test_model_id_of_a_live_row_is_rejected():
    t = _table_with_one_live_row()
    b, (after, st, rows, _) = _one(t, [(sc.OK, 0x77, 6, 0)])
    assert st == [sc.REJECTED] and after == t


def test_model_id_is_seen_before_the_capacity_check():
    """the first holder of an id finds the table full; its duplicate is still a duplicate"""
    t = sc.empty_tables(1, 2)
    b, (after, st, rows, _) = _one(t, [(sc.OK, 1, 6, 0), (sc.OK, 2, 6, 0), (sc.OK, 2, 6, 1), (sc.OK, 1, 6, 1)])
    assert st == [sc.OK, sc.FULL, sc.REJECTED, sc.REJECTED] and rows == [0, sc.SKIP, sc.SKIP, sc.SKIP]
    # an invalid or gated row does not enter seen
    b, (after, st, rows, _) = _one(sc.empty_tables(4, 2), [(sc.OK, 1, 6, 5), (sc.REJECTED, 1, 6, 0), (sc.OK, 1, 6, 0)])
    assert st == [sc.INVALID, sc.REJECTED, sc.OK]


def test_model_free_rows_are_taken_ascending_and_run_out():
    t = sc.empty_tables(5, 2)
    rng = np.random.default_rng(3)
    sc.seed_row(t, 0, 0x70, 1, 0, rng)
    sc.seed_row(t, 2, 0x71, 1, 0, rng)
    b, (after, st, rows, _) = _one(t, [(sc.OK, 10 + i, 20 + i, i % 2) for i in range(5)])
    assert rows == [1, 3, 4, sc.SKIP, sc.SKIP] and st == [sc.OK] * 3 + [sc.FULL] * 2
    assert after["local_ids"] == [0x70, 10, 0x71, 11, 12] and after["slot_peer"] == [0, 0, 0, 1, 0]


def test_model_row_fields_and_the_clock():
    t = _table_with_one_live_row()
    b, (after, st, rows, _) = _one(t, [(sc.OK, 0x31, 0x32, 0)], now=555)
    r = rows[0]
    assert r == 0 and st == [sc.OK]
    assert after["send_keys"][r] == b["keys"][0][:32] and after["recv_keys"][r] == b["keys"][0][32:]
    assert (after["receivers"][r], after["local_ids"][r], after["slot_peer"][r]) == (0x32, 0x31, 0)
    assert after["windows"][r] == bytes(264) and after["send_state"][r] == (0, 555, 555)
    for name in sc.ROW_ARRAYS:
        assert after[name][1:] == t[name][1:], name  # the other rows keep every field
    _, (after0, _, _, _) = _one(t, [(sc.OK, 0x31, 0x32, 0)], now=None)
    assert after0["send_state"][0] == (0, 0, 0)  # now_ns NULL


def test_model_last_handshake_of_a_peer_is_current_and_the_old_row_stays():
    t = _table_with_one_live_row()
    b, (after, st, rows, _) = _one(t, [(sc.OK, 1, 2, 1), (sc.OK, 3, 4, 1)])
    assert rows == [0, 2] and after["peer_slot"] == [sc.SKIP, 2]
    assert after["slot_peer"] == [1, 1, 1] and after["local_ids"][1] == 0x77  # the previous session still receives
    assert sc.rx_pairs(after) == {1: 0, 0x77: 1, 3: 2}


def test_model_every_rule_case_matches_its_hand_written_expectations():
    t, b, now, status, rows_out, peer_slot = sc.every_rule_case()
    assert len(t["slot_peer"]) == 8 and len(t["peer_slot"]) == 4 and len(status) == 12
    after, st, rows, keys = sc.install_loop(t, b["gate"], b["local_ids"], b["remote_ids"], b["peers"], b["keys"], now)
    assert st == status and rows == rows_out and after["peer_slot"] == peer_slot
    assert [k == b["keys"][i] for i, k in enumerate(keys)] == [g != sc.OK for g in b["gate"]]
    a, c = b["local_ids"][0], b["local_ids"][6]
    assert a != c and sc.rx_home(a, 16) == sc.rx_home(c, 16)
    assert sc.rx_pairs(after) == {0x100: 0, a: 1, 0x101: 2, 0x102: 3, 0x3001: 4, 0x103: 5, 0x104: 6, c: 7}
    assert after["send_state"][7] == (0, now, now)


def test_model_wrappers_gather_the_handshake_outputs():
    row = bytearray(128)
    row[108:112], row[112:116] = (3).to_bytes(4, "little"), (0xABCD).to_bytes(4, "little")
    assert sc.gather_resp([9], [bytes(row)]) == ([9], [0xABCD], [3])
    got = sc.gather_finish([sc.OK] * 3, [1, 2, sc.NONE], [70, 71, 0], [100, 101], [5, 6])
    assert got == ([101, 0, 0], [70, 71, 0], [6, sc.NONE, sc.NONE])  # no such pending row: no peer, RG_PKT_INVALID


def test_model_expiry_case_matches_its_hand_written_expectations():
    t, now, rows, expired, peer_slot = sc.expiry_case()
    after, got = sc.expire_loop(t, now, rows)
    assert got == expired and after["peer_slot"] == peer_slot
    for r, gone in enumerate(expired):
        if gone:
            assert all(after[name][r] == sc.empty_tables(1, 0)[name][0] for name in sc.ROW_ARRAYS), r
        else:
            assert all(after[name][r] == t[name][r] for name in sc.ROW_ARRAYS), r
    assert sc.rx_pairs(after) == {0x700: 0, 0x704: 4}
    # the list alone (now_ns NULL): the old rows stay
    after, got = sc.expire_loop(t, None, rows)
    assert got == [0, 0, 0, 1, 0, 0, 0, 0, 0, 0] and after["peer_slot"] == [sc.SKIP, 4, 1, 2]
    # a following install takes the lowest freed rows
    after, _ = sc.expire_loop(t, now, rows)
    _, (_, st, got_rows, _) = _one(after, [(sc.OK, 0x900 + i, 1, 0) for i in range(3)])
    assert got_rows == [1, 2, 3] and st == [sc.OK] * 3


def test_scattered_cases_cover_what_they_claim():
    n = nkeys = 2 * sc.TILE + 3
    t = sc.scattered_tables(nkeys, 5, 21, extra_live=(1, 2, 4, 5, 7))
    b = sc.scattered_batch(n, 5, 22)
    after, st, rows, _ = sc.install_loop(t, b["gate"], b["local_ids"], b["remote_ids"], b["peers"], b["keys"], 7)
    free = sum(p == sc.NONE for p in t["slot_peer"])
    assert st.count(sc.OK) == free and 0 < st.count(sc.FULL) <= 8
    assert st.count(sc.INVALID) > 300 and st.count(sc.REJECTED) > 600
    # (the table's last row is live before the call)
    assert max(r for r in rows if r != sc.SKIP) == nkeys - 2 and sc.NONE not in after["slot_peer"]
    ok = [i for i, s in enumerate(st) if s == sc.OK]
    full = [i for i, s in enumerate(st) if s == sc.FULL]
    assert {i // sc.TILE for i in ok} == {0, 1} and {i // sc.TILE for i in full} == {1, 2}  # a rank past every tile
    assert {r // sc.TILE for r in rows if r != sc.SKIP} == {0, 1, 2}  # and free rows in every tile of the table
