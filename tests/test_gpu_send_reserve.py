"""rg_send_reserve_batch_dev on the GPU against its definition: rg_send_batch's array-order loop over the state
rows (send_cases.loop).  status, counters, rekey flags and every byte of every state row (24 a row) are compared
exactly, and so are the working descriptors the call leaves at the start of its workspace."""
import ctypes

import numpy as np
import pytest
import torch

import send_cases as sc
from rustyguard_amd import aead
from rustyguard_amd.workloads import DESC_DTYPE

pytestmark = pytest.mark.gpu

CASES = sc.cases()


def _i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()


def _desc(lens):
    d = np.zeros(len(lens), DESC_DTYPE)
    d["offset"] = np.arange(len(lens), dtype=np.uint64) * 1552 + 16
    d["len"] = lens
    d["key_idx"] = 0x5A5A5A5A  # ignored by the call
    return d


class Dev:
    """One batch's device arrays, outputs preset to a pattern no result has."""

    def __init__(self, state, slots, lens, now, rekey=True):
        n = len(slots)
        self.desc = _desc(lens)
        self.state = _i64(np.asarray(state, np.uint64).reshape(-1))
        self.slots = torch.from_numpy(np.asarray(slots, np.uint32).view(np.int32).copy()).cuda()
        self.dd = torch.from_numpy(self.desc.view(np.uint8).reshape(-1, 16).copy()).cuda()
        self.now = None if now is None else _i64(np.array([now], np.uint64))
        self.status = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        self.ctr = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        self.rekey = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda") if rekey else None

    def rows(self):
        return self.state.cpu().numpy().view(np.uint64).reshape(-1, 3)

    def results(self):
        return (self.status.cpu().numpy(), self.ctr.cpu().numpy().view(np.uint64),
                None if self.rekey is None else self.rekey.cpu().numpy(), self.rows())


def _compare(got, want):
    st, ctr, rk, S = got
    st_w, ctr_w, rk_w, S_w = want
    assert np.array_equal(st, st_w), np.nonzero(st != st_w)[0][:10]
    assert np.array_equal(ctr, ctr_w), np.nonzero(ctr != ctr_w)[0][:10]
    if rk is not None:
        assert np.array_equal(rk, rk_w), np.nonzero(rk != rk_w)[0][:10]
    assert np.array_equal(S, S_w), np.nonzero((S != S_w).any(axis=1))[0][:10]


def _run(engine, case):
    name, state, slots, lens, now = case
    want = sc.loop(state, slots, lens, now)
    d = Dev(state, slots, lens, now)
    ws = engine.send_reserve_batch_dev(d.state, d.slots, d.dd, d.status, d.ctr, d.rekey, d.now)
    torch.cuda.synchronize()
    _compare(d.results(), want)
    # the working descriptors: the caller's rows under the packet's key row, RG_KEY_SKIP without a counter
    work = ws[:16 * len(slots)].cpu().numpy().view(DESC_DTYPE)
    assert np.array_equal(work["offset"], d.desc["offset"]) and np.array_equal(work["len"], d.desc["len"])
    took = want[0] == sc.PENDING
    assert np.array_equal(work["key_idx"], np.where(took, np.asarray(slots, np.uint32), sc.SKIP))
    return d, took


@pytest.mark.parametrize("case", sc.large_cases(), ids=lambda c: c[0])
def test_large_case(engine, case):
    """The loops of the grouped scan that run more than once (send_cases.LARGE_SIZES; test_send_cpu.py shows
    which loop each size reaches): the radix scan with two and three entries a lane, two and three radix passes
    over several tiles, the carry with two tiles a lane, rows whose grouped runs span whole tiles."""
    _run(engine, case)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_case(engine, case):
    name, state, slots, lens, now = case
    d, took = _run(engine, case)
    if name == "rekey_edge":
        assert list(d.rekey.cpu().numpy()) == sc.expect_rekey_edge()
    if name == "reject_edge_8300":
        assert took.sum() == 3 and int(d.rows()[0, 0]) == sc.REJECT
    if name in ("at_reject", "past_reject", "counter_max"):
        assert np.array_equal(d.rows(), state)


def test_rekey_out_is_optional(engine):
    _, state, slots, lens, now = next(c for c in CASES if c[0] == "ineligible_3rows_700")
    d = Dev(state, slots, lens, now, rekey=False)
    engine.send_reserve_batch_dev(d.state, d.slots, d.dd, d.status, d.ctr, None, d.now)
    torch.cuda.synchronize()
    _compare(d.results(), sc.loop(state, slots, lens, now))


def test_no_rows_at_all(engine):
    """nkeys == 0: every packet is rejected (the counter pass accepts it; the resident send does not)."""
    L, h = engine.library, engine.handle
    n = 70
    d = Dev(sc.rows(9), np.zeros(n, np.uint32), np.full(n, 16, np.uint32), None)
    ws = engine.send_workspace(n, 0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert L.rg_send_reserve_batch_dev(h, p(d.state), 0, p(d.slots), p(d.dd), n, None, p(d.status), p(d.ctr),
                                       p(d.rekey), p(ws), ws.numel(), aead._stream_handle(None)) == 0
    torch.cuda.synchronize()
    st, ctr, rk, S = d.results()
    assert (st == sc.REJECTED).all() and not ctr.any() and not rk.any() and np.array_equal(S, sc.rows(9))
    assert (ws[:16 * n].cpu().numpy().view(DESC_DTYPE)["key_idx"] == sc.SKIP).all()


@pytest.mark.parametrize("name", ["three_rows_2049", "times", "reject_edge_rows"])
def test_two_calls_share_a_workspace(engine, name):
    """Back to back on one stream, nothing waited for in between: the second call continues the counters."""
    _, state, slots, lens, now = next(c for c in CASES if c[0] == name)
    n, half = len(slots), len(slots) // 2 + 1
    st1, c1, r1, S1 = sc.loop(state, slots[:half], lens[:half], now)
    later = None if now is None else now + 1000
    st2, c2, r2, S2 = sc.loop(S1, slots[half:], lens[half:], later)
    d = Dev(state, slots, lens, now)
    now2 = None if later is None else _i64(np.array([later], np.uint64))
    ws = engine.send_workspace(half, len(state))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    engine.send_reserve_batch_dev(d.state, d.slots[:half], d.dd[:half], d.status[:half], d.ctr[:half], d.rekey[:half],
                                  d.now, workspace=ws, stream=s)
    engine.send_reserve_batch_dev(d.state, d.slots[half:], d.dd[half:], d.status[half:], d.ctr[half:], d.rekey[half:],
                                  now2, workspace=ws, stream=s)
    torch.cuda.synchronize()
    _compare(d.results(), (np.concatenate([st1, st2]), np.concatenate([c1, c2]), np.concatenate([r1, r2]), S2))
    assert n - half >= 1


def test_argument_errors(engine):
    L, h = engine.library, engine.handle
    _, state, slots, lens, now = next(c for c in CASES if c[0] == "three_rows_65")
    d = Dev(state, slots, lens, now)
    d.state = torch.cat([d.state, torch.zeros(1, dtype=torch.int64, device="cuda")])  # room for the misaligned view
    ws = engine.send_workspace(65, 3)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    need = L.rg_send_workspace_size(65, 3)
    before = [t.cpu().numpy().copy() for t in (d.state, d.status, d.ctr, d.rekey)]
    stream = aead._stream_handle(None)

    def call(state=p(d.state), status=p(d.status), ctr=p(d.ctr), wsp=p(ws), wlen=need, n=65, slots=p(d.slots),
             desc=p(d.dd)):
        return L.rg_send_reserve_batch_dev(h, state, 3, slots, desc, n, p(d.now), status, ctr, p(d.rekey), wsp, wlen,
                                           stream)

    bad = {
        "short workspace": call(wlen=need - 1),
        "misaligned state": call(state=p(d.state, 4)),
        "misaligned workspace": call(wsp=p(ws, 8)),
        "null status": call(status=None),
        "null state": call(state=None),
        "null slots": call(slots=None),
        "null desc": call(desc=None),
        "null counters": call(ctr=None),
        "null workspace": call(wsp=None),
        "too many packets": call(n=1 << 32, wlen=1 << 62),
    }
    assert all(rc == -1 for rc in bad.values()), bad  # RG_EINVAL
    torch.cuda.synchronize()
    after = [t.cpu().numpy() for t in (d.state, d.status, d.ctr, d.rekey)]
    assert all(np.array_equal(a, b) for a, b in zip(after, before))
    assert L.rg_send_reserve_batch_dev(h, None, 3, None, None, 0, None, None, None, None, None, 0, stream) == 0  # n == 0
