"""The device-resident pending handshakes, the part that needs no GPU: the ABI surface (header, both libraries,
ctypes table, source list), the layout of rg_pending_timer and the constants, rg_pending_workspace_size, the
argument rules -- each answered before the device is touched -- and the sequential model (tests/pending_cases.py)
against hand-written expectations, one case per line of the loops."""
import ctypes
import os
import re
import subprocess
import textwrap

import numpy as np

import pending_cases as pc
from conftest import REPO
from rustyguard_amd import _lib, build, pending

NAMES = ("rg_pending_workspace_size", "rg_pending_index_dev", "rg_pending_install_batch_dev", "rg_pending_turn_dev")
EINVAL, EDEVICE = -1, -2
NOW = 10**12
OK, INV, REJ, NONE = pc.OK, pc.INVALID, pc.REJECTED, pc.NONE
RNG = np.random.default_rng(11)


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
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [3, 3, 11, 14]
    assert "rg_pending.hip" in build.KERNELS and "rg_pending.hip" not in build.HOST
    for unit in build.HOST:
        assert "rg_pending_" not in open(os.path.join(build.CSRC, unit)).read(), unit


def test_timer_layout_and_constants_with_gcc(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "rg_aead.h"
        int main(void) {
            printf("%zu %zu %zu %zu\\n", sizeof(rg_pending_timer), _Alignof(rg_pending_timer),
                   offsetof(rg_pending_timer, started_ns), offsetof(rg_pending_timer, sent_ns));
            printf("%llu %llu\\n", RG_REKEY_TIMEOUT_NS, RG_REKEY_ATTEMPT_TIME_NS);
            printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(rg_pending_tables), offsetof(rg_pending_tables, pending),
                   offsetof(rg_pending_tables, timers), offsetof(rg_pending_tables, hs_ids),
                   offsetof(rg_pending_tables, pend_table), offsetof(rg_pending_tables, npeers),
                   offsetof(rg_pending_tables, pend_cap));
            return 0;
        }
    """))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                   check=True)
    vals = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert vals[:4] == [16, 8, 0, 8]
    assert vals[4:6] == [5 * 10**9, 90 * 10**9] == [pc.RETRY_NS, pc.ATTEMPT_NS]
    assert (pending.REKEY_TIMEOUT_NS, pending.REKEY_ATTEMPT_TIME_NS) == tuple(vals[4:6])
    T, S = pending.PendingTimerStruct, pending.PendingTablesStruct
    assert (ctypes.sizeof(T), T.started_ns.offset, T.sent_ns.offset) == (16, 0, 8) and pending.TIMER_BYTES == 16
    assert [ctypes.sizeof(S)] + [getattr(S, n).offset for n, _ in S._fields_] == vals[6:]
    assert pending.PENDING_BYTES == pc.ROW == 128 and len(pc.EMPTY) == 128
    assert pc.row_peer(pc.EMPTY) == NONE and 4 * pending.PEER_WORD == 96 and 4 * pending.SENDER_WORD == 100


def test_workspace_size_is_monotone_and_refuses_absurd_sizes():
    size = _lib.lib().rg_pending_workspace_size
    sizes = [0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 4099, 65536, 1 << 20, (1 << 31) + 1, (1 << 32) - 1]
    for a in (0, 5, 4099, (1 << 32) - 1):
        for b in (0, 7, (1 << 32) - 1):
            col = [size(a, b, p) for p in sizes]
            assert all(x <= y for x, y in zip(col, col[1:])) and col[0] >= 256, (a, b, col)
            assert all(c % 256 == 0 for c in col)
    for p in sizes:
        assert all(x <= y for x, y in zip([size(k, 0, p) for k in sizes], [size(k, 0, p) for k in sizes][1:]))
        assert all(x <= y for x, y in zip([size(0, k, p) for k in sizes], [size(0, k, p) for k in sizes][1:]))
    assert size(1 << 32, 0, 4) == 0 and size(0, 1 << 32, 4) == 0 and size((1 << 64) - 1, 0, 0) == 0
    # one claim / want word per peer, and twelve bytes of aggregates per tile of 2048 peers
    assert size(0, 0, 4099) >= 4099 * 4 + 3 * 12 and size(0, 0, (1 << 32) - 1) > 4 * ((1 << 32) - 1)


# ------------------------------------------------------------------ refusals
class Args:
    """A set of arguments every rule accepts, as plain addresses that nothing may dereference: the context is a block
    whose device ordinal no machine has, so a call that got past its argument rules ends in RG_EDEVICE at
    hipSetDevice, with nothing enqueued, and every refusal below is the work of the one thing changed."""

    NPEERS, N, M = 6, 4, 3

    def __init__(self):
        self.ctx = ctypes.create_string_buffer(1 << 16)
        ctypes.memmove(self.ctx, (ctypes.c_int * 1)(0x3FFFFFF0), 4)  # rg_ctx.device
        self.need = int(_lib.lib().rg_pending_workspace_size(self.N, self.M, self.NPEERS))
        self.t = pending.PendingTablesStruct(pending=0x10000, timers=0x20000, hs_ids=0x30000, pend_table=0x40000,
                                             npeers=self.NPEERS, pend_cap=16)
        self.batch, self.gate, self.now, self.status, self.out = 0x50000, 0x60000, 0x70000, 0x80000, 0x90000
        self.start, self.start_st, self.peers_out, self.gate_out = 0xA0000, 0xB0000, 0xC0000, 0xD0000
        self.expired, self.counts, self.ws = 0xE0000, 0xF0000, 0x100000

    def index(self, ctx="ctx", tables="t", **fields):
        return _lib.lib().rg_pending_index_dev(self._ctx(ctx), self._tables(tables, fields), None)

    def install(self, ctx="ctx", tables="t", batch=None, gate=None, n=None, now=None, status=None, out=None, ws=None,
                wl=None, **fields):
        d = lambda v, x: x if v is None else (None if v == 0 else v)  # noqa: E731
        return _lib.lib().rg_pending_install_batch_dev(
            self._ctx(ctx), self._tables(tables, fields), d(batch, self.batch), d(gate, self.gate),
            self.N if n is None else n, d(now, self.now), d(status, self.status), d(out, self.out), d(ws, self.ws),
            self.need if wl is None else wl, None)

    def turn(self, ctx="ctx", tables="t", now=None, start=None, start_st=None, m=None, peers_out=None, gate_out=None,
             expired=None, counts=None, ws=None, wl=None, **fields):
        d = lambda v, x: x if v is None else (None if v == 0 else v)  # noqa: E731
        return _lib.lib().rg_pending_turn_dev(
            self._ctx(ctx), self._tables(tables, fields), d(now, self.now), d(start, self.start),
            d(start_st, self.start_st), REJ, self.M if m is None else m, d(peers_out, self.peers_out),
            d(gate_out, self.gate_out), d(expired, self.expired), d(counts, self.counts), d(ws, self.ws),
            self.need if wl is None else wl, None)

    def _ctx(self, ctx):
        return ctypes.cast(self.ctx, ctypes.c_void_p) if ctx == "ctx" else None

    def _tables(self, tables, fields):
        if tables is None:
            return None
        t = pending.PendingTablesStruct.from_buffer_copy(self.t)
        for k, v in fields.items():
            setattr(t, k, v)
        return ctypes.byref(t)


TABLE_RULES = (dict(tables=None), dict(pending=0), dict(timers=0), dict(hs_ids=0), dict(pend_table=0),
               dict(pending=0x10001), dict(pending=0x10008), dict(timers=0x20001), dict(timers=0x20004),
               dict(hs_ids=0x30001), dict(hs_ids=0x30002), dict(pend_table=0x40001), dict(pend_table=0x40004),
               dict(pend_cap=3), dict(pend_cap=Args.NPEERS), dict(pend_cap=0), dict(pend_cap=8), dict(pend_cap=12))


def _refused(call, name, bad):
    assert call(**bad) == EINVAL, (name, bad)
    assert name in _lib.lib().rg_last_error(), (name, bad, _lib.lib().rg_last_error())


def test_every_argument_rule_is_answered_before_the_device_is_touched():
    a = Args()
    # the arguments as they stand pass every rule: the calls get as far as selecting the device
    assert a.index() == EDEVICE and a.install() == EDEVICE and a.turn() == EDEVICE
    assert a.install(pend_cap=16, npeers=8) == EDEVICE and a.turn(wl=a.need + 1) == EDEVICE
    # the optional arrays, and sizes of zero
    assert a.install(gate=0) == EDEVICE and a.turn(expired=0) == EDEVICE and a.turn(start_st=0) == EDEVICE
    assert a.turn(start=0, m=0) == EDEVICE and a.install(n=0) == 0
    assert a.turn(npeers=0, pending=0, timers=0, hs_ids=0, peers_out=0, gate_out=0, pend_cap=1) == EDEVICE
    # a null context, whatever else
    assert a.index(ctx=None) == EINVAL and a.install(ctx=None) == EINVAL and a.turn(ctx=None) == EINVAL
    assert a.install(ctx=None, n=0) == EINVAL
    for bad in TABLE_RULES:
        _refused(a.index, b"pending index", bad)
        _refused(a.install, b"pending install", bad)
        _refused(a.turn, b"pending turn", bad)
    row = 128
    for bad in (dict(batch=0), dict(now=0), dict(status=0), dict(out=0), dict(ws=0), dict(n=1 << 32),
                dict(batch=a.batch + 1), dict(batch=a.batch + 8), dict(now=a.now + 1), dict(now=a.now + 4),
                dict(out=a.out + 1), dict(out=a.out + 2), dict(ws=a.ws + 1), dict(ws=a.ws + 8), dict(wl=a.need - 1),
                dict(wl=0),
                # batch over tables.pending: the same array, its last row on the table's first, its first on the last
                dict(batch=0x10000), dict(batch=0x10000 - (a.N - 1) * row), dict(batch=0x10000 + (a.NPEERS - 1) * row),
                dict(batch=0x10000 - 16 * row, n=20)):
        _refused(a.install, b"pending install", bad)
    assert a.install(batch=0x10000 - a.N * row) == EDEVICE and a.install(batch=0x10000 + a.NPEERS * row) == EDEVICE
    for bad in (dict(now=0), dict(counts=0), dict(ws=0), dict(peers_out=0), dict(gate_out=0), dict(start=0),
                dict(m=1 << 32), dict(now=a.now + 1), dict(now=a.now + 4), dict(start=a.start + 1),
                dict(start=a.start + 2), dict(peers_out=a.peers_out + 1), dict(peers_out=a.peers_out + 2),
                dict(counts=a.counts + 1), dict(counts=a.counts + 2), dict(ws=a.ws + 1), dict(ws=a.ws + 8),
                dict(wl=a.need - 1), dict(wl=0)):
        _refused(a.turn, b"pending turn", bad)


# ---------------------------------------------------------------- the model
def _live_table(rows):
    """rows of (started_ns, sent_ns) or None -> a table whose peer p is live with those times"""
    t = pc.empty_table(len(rows))
    for p, tm in enumerate(rows):
        if tm is not None:
            t["pending"][p], t["timers"][p], t["hs_ids"][p] = pc.make_row(p, 0x100 + p, RNG), tm, 0x100 + p
    return t


def test_model_turn_expiry_at_the_deadline_and_one_past_it():
    """sent + 90 s == now is not expired (strict); one ns later it is, and the row, its timers and the flag show it"""
    sent = NOW - pc.ATTEMPT_NS
    t = _live_table([(sent, sent), (sent - 1, sent - 1)])
    got, init, gate, expired, counts = pc.turn_loop(t, NOW)
    assert got["pending"] == [t["pending"][0], pc.EMPTY] and got["timers"] == [(sent, sent), (0, 0)]
    assert expired == [0, 1] and counts == [0, 1] and init == [NONE, NONE] and gate == [REJ, REJ]
    assert got["hs_ids"] == t["hs_ids"] and pc.lookup(got) == {0x100: 0}  # hs_ids is the install's alone


def test_model_turn_retry_at_the_deadline_and_at_the_end_of_the_attempt_time():
    """sent + 5 s == now does not retry, one ns later it does and `sent` moves while `started` stays; at
    now == started + 90 s there is no retry, one ns earlier there is"""
    r, e = NOW - pc.RETRY_NS, NOW - pc.ATTEMPT_NS
    t = _live_table([(r, r), (r - 1, r - 1), (e, r - 1), (e + 1, r - 1), (e - 5, e + 5)])
    got, init, gate, expired, counts = pc.turn_loop(t, NOW)
    assert got["timers"] == [(r, r), (r - 1, NOW), (e, r - 1), (e + 1, NOW), (e - 5, e + 5)]
    assert init == [1, 3, NONE, NONE, NONE] and gate == [OK, OK, REJ, REJ, REJ] and counts == [2, 0]
    assert got["pending"] == t["pending"] and expired == [0] * 5
    again = pc.turn_loop(got, NOW)  # the same clock twice: nothing is due, no byte moves
    assert again == (got, [NONE] * 5, [REJ] * 5, [0] * 5, [0, 0])


def test_model_turn_requests_for_a_live_a_dead_a_just_expired_and_an_out_of_range_peer():
    sent = NOW - pc.ATTEMPT_NS - 1
    t = _live_table([(NOW - 1, NOW - 1), None, (sent, sent), None])
    got, init, gate, expired, counts = pc.turn_loop(t, NOW, [0, 1, 2, 4, NONE, 1])
    # the live row's own retry governs; the dead and the just-expired peer start; peer 3 was not asked for
    assert init == [1, 2, NONE, NONE] and gate == [OK, OK, REJ, REJ] and expired == [0, 0, 1, 0] and counts == [2, 1]
    assert got["timers"][0] == (NOW - 1, NOW - 1) and got["pending"][2] == pc.EMPTY
    # a row that names another peer is not live
    t["pending"][3] = pc.make_row(2, 9, RNG)
    assert pc.turn_loop(t, NOW, [3])[1] == [3, NONE, NONE, NONE]


def test_model_turn_start_match_filters_the_requests():
    t = _live_table([None] * 4)
    peers, status = [0, 1, 2, 3], [OK, REJ, INV, REJ]
    assert pc.turn_loop(t, NOW, peers, status, REJ)[1] == [1, 3, NONE, NONE]
    assert pc.turn_loop(t, NOW, peers, status, OK)[1] == [0, NONE, NONE, NONE]
    assert pc.turn_loop(t, NOW, peers, None, REJ)[1] == [0, 1, 2, 3] and pc.turn_loop(t, NOW)[4] == [0, 0]


def test_model_turn_near_the_end_of_the_clock():
    """the adds wrap: a row sent 3 ns before 2^64 is 90 s old once now passes 90e9 - 3, and its sum is small"""
    top = (1 << 64) - 3
    t = _live_table([(top, top), (top, top)])
    assert pc.turn_loop(t, pc.ATTEMPT_NS - 3)[3] == [0, 0] and pc.turn_loop(t, pc.ATTEMPT_NS - 2)[3] == [1, 1]
    got = pc.turn_loop(t, pc.RETRY_NS - 2)
    assert got[1] == [0, 1] and got[0]["timers"] == [(top, pc.RETRY_NS - 2)] * 2
    assert pc.turn_loop(_live_table([(5, 5)]), (1 << 64) - 1)[4] == [0, 1]  # 5 + 90e9 < 2^64 - 1: long expired
    # one ns after it was sent, below the wrap: the sum is small, so the row reads as expired (the send path's rule)
    assert pc.turn_loop(_live_table([(top, top)]), top + 1)[4] == [0, 1]


def test_model_install_gate_consumed_rows_and_peers_past_the_table():
    t = pc.empty_table(3)
    rows = [pc.make_row(p, 0x40 + i, RNG) for i, p in enumerate((0, 3, NONE, 2, 1))]
    got, batch, status, installed = pc.install_loop(t, rows, [OK, OK, OK, REJ, 6], NOW)
    assert status == [OK, INV, INV, REJ, REJ] and installed == [0, NONE, NONE, NONE, NONE]
    assert batch == [pc.EMPTY] * 3 + rows[3:]  # a row is consumed whatever follows; a gated one is not touched
    assert got["pending"] == [rows[0], pc.EMPTY, pc.EMPTY] and got["hs_ids"] == [0x40, 0, 0]
    assert got["timers"] == [(NOW, NOW), (0, 0), (0, 0)] and pc.lookup(got) == {0x40: 0}
    assert pc.install_loop(t, rows, None, NOW)[2] == [OK, INV, INV, OK, OK]  # no gate: every row passes


def test_model_install_two_rows_of_one_peer_and_a_retry_keeps_started():
    t = _live_table([(NOW - 7 * 10**9, NOW - 6 * 10**9), None])
    rows = [pc.make_row(0, 0x50, RNG), pc.make_row(1, 0x51, RNG), pc.make_row(0, 0x52, RNG), pc.make_row(1, 0x53, RNG)]
    got, batch, status, installed = pc.install_loop(t, rows, None, NOW)
    assert status == [OK] * 4 and installed == [NONE, NONE, 0, 1] and batch == [pc.EMPTY] * 4
    assert got["pending"] == [rows[2], rows[3]] and got["hs_ids"] == [0x52, 0x53]
    assert got["timers"] == [(NOW - 7 * 10**9, NOW), (NOW, NOW)]  # the live peer keeps `started`, the dead one starts
    assert pc.lookup(got) == {0x52: 0, 0x53: 1}  # the replaced ids and the old one answer nothing


def test_cases_cover_what_they_claim():
    t = pc.random_table(4099, 3, NOW)
    got, init, gate, expired, counts = pc.turn_loop(t, NOW)
    assert 300 < counts[0] < 4099 and 100 < counts[1] < 4099
    assert {p // pc.TILE for p in init if p != NONE} == {0, 1, 2}  # the carry runs over two tiles
    assert {p // pc.TILE for p, e in enumerate(expired) if e} >= {0, 1}
    kinds = {pc.row_peer(r) == p for p, r in enumerate(t["pending"])}
    assert kinds == {True, False} and any(r == pc.EMPTY for r in t["pending"])
    assert any(pc.row_peer(r) not in (p, NONE) for p, r in enumerate(t["pending"]))
    ids = [pc.sender_of(p, a) for p in range(4099) for a in (0, 1, 2, 7)]
    assert len(set(ids)) == len(ids)
    peers, status = pc.request_list(4099, 2049, 4)
    assert NONE in peers and any(NONE > q >= 4099 for q in peers) and len(set(peers)) < len(peers)
    with_st, without = pc.turn_loop(t, NOW, peers, status, REJ), pc.turn_loop(t, NOW, peers)
    assert counts[0] < with_st[4][0] < without[4][0]
    for n, npeers in ((65, 5), (2049, 4099)):
        batch, gate = pc.install_batch(n, npeers, 6)
        after, wiped, st, installed = pc.install_loop(pc.random_table(npeers, 8, NOW), batch, gate, NOW)
        assert {OK, INV, REJ} == set(st) and installed[n - 1] == 1 and installed[63] == NONE
        assert pc.row_peer(batch[63]) == pc.row_peer(batch[64]) == 1 and (n == 65 or installed[64] == installed[2047] == NONE)
        assert sum(x != NONE for x in installed) == len({x for x in installed if x != NONE})
    ids = pc.colliding_ids(65, 256)
    assert len(set(ids)) == 65 and {pc.rx_slot(i, 256) for i in ids} == {5}
    table = np.zeros((256, 2), np.uint32)
    assert _lib.lib().rg_rx_table_build(np.array(ids, np.uint32).ctypes.data_as(ctypes.c_void_p),
                                        np.arange(65, dtype=np.uint32).ctypes.data_as(ctypes.c_void_p), 65,
                                        table.ctypes.data_as(ctypes.c_void_p), 256) == 0
    assert [int(x) for x in table[5:70, 0]] == ids  # the library's hash is the cases' hash
