"""rg_replay_batch_dev on the GPU against its definition: the host rg_antireplay_would_accept /
rg_antireplay_mark_seen applied in array order (replay_cases.host_commit; the reference's own unit tests pin
those in test_antireplay_cpu.py).  status, undo and every byte of every window (264 a row) are compared exactly."""
import ctypes

import numpy as np
import pytest
import torch

import replay_cases as rc
from rustyguard_amd import aead

pytestmark = pytest.mark.gpu


def gpu_commit(engine, windows, win_idx, counters, status, with_undo=True):
    dW = torch.from_numpy(np.ascontiguousarray(windows, np.uint64).view(np.int64).copy()).cuda()
    dw = torch.from_numpy(np.asarray(win_idx, np.uint32).view(np.int32).copy()).cuda()
    dc = torch.from_numpy(np.asarray(counters, np.uint64).view(np.int64).copy()).cuda()
    ds = torch.from_numpy(np.array(status, np.uint8)).cuda()
    du = torch.full((len(status),), 0xEE, dtype=torch.uint8, device="cuda") if with_undo else None
    engine.replay_batch_dev(dW, dw, dc, ds, du)
    torch.cuda.synchronize()
    return (ds.cpu().numpy(), du.cpu().numpy() if with_undo else None,
            dW.cpu().numpy().view(np.uint64).reshape(-1, 33))


def check(engine, case):
    W, widx, ctrs, sts = case
    st_h, undo_h, W_h, cls = rc.host_commit(W, widx, ctrs, sts)
    st_g, undo_g, W_g = gpu_commit(engine, W, widx, ctrs, sts)
    assert np.array_equal(st_g, st_h), np.nonzero(st_g != st_h)[0][:10]
    assert np.array_equal(undo_g, undo_h), np.nonzero(undo_g != undo_h)[0][:10]
    assert np.array_equal(W_g, W_h), np.nonzero((W_g != W_h).any(axis=1))[0][:10]
    return st_h, W_h, cls


@pytest.fixture(scope="module")
def ref_seq():
    seq = rc.reference_sequence()
    return seq, rc.host_commit(rc.fresh(), np.zeros(len(seq), np.uint32), seq, np.zeros(len(seq), np.uint8))


def test_reference_sequence_one_batch(engine, ref_seq):
    seq, (st_h, undo_h, W_h, _) = ref_seq
    st_g, undo_g, W_g = gpu_commit(engine, rc.fresh(), np.zeros(len(seq), np.uint32), seq, np.zeros(len(seq), np.uint8))
    assert np.array_equal(st_g, st_h) and np.array_equal(undo_g, undo_h) and np.array_equal(W_g, W_h)
    assert list(st_g[-5:]) == [rc.OK, rc.REJECTED, rc.OK, rc.REJECTED, rc.OK]


@pytest.mark.parametrize("size", [64, 1])
def test_reference_sequence_split(engine, ref_seq, size):
    """The same sequence in batches of 64 and of 1: the device window is carried from call to call."""
    seq, (st_h, undo_h, W_h, _) = ref_seq
    n = len(seq)
    dW = torch.zeros(33, dtype=torch.int64, device="cuda")
    dc = torch.from_numpy(seq.view(np.int64).copy()).cuda()
    dw = torch.zeros(n, dtype=torch.int32, device="cuda")
    ds = torch.zeros(n, dtype=torch.uint8, device="cuda")
    du = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    ws = engine.replay_workspace(size, 1)
    for at in range(0, n, size):
        engine.replay_batch_dev(dW, dw[at:at + size], dc[at:at + size], ds[at:at + size], du[at:at + size], workspace=ws)
    torch.cuda.synchronize()
    assert np.array_equal(ds.cpu().numpy(), st_h)
    assert np.array_equal(du.cpu().numpy(), undo_h)
    assert np.array_equal(dW.cpu().numpy().view(np.uint64).reshape(1, 33), W_h)


def test_unauthenticated_high_counter_does_not_lock_out(engine):
    st, W, _ = check(engine, (rc.fresh(), np.zeros(3, np.uint32), np.array([5, 1_000_000, 6], np.uint64),
                              np.array([rc.OK, rc.ERR, rc.OK], np.uint8)))
    assert list(st) == [rc.OK, rc.ERR, rc.OK] and int(W[0, 32]) == 6


@pytest.mark.parametrize("case", rc.edge_cases(), ids=lambda c: c[0])
def test_edges(engine, case):
    name, win, ctrs, sts = case
    st, _, _ = check(engine, (win[None, :], np.zeros(len(ctrs), np.uint32), ctrs, sts))
    if name.startswith("err_ok_ok_err"):
        assert list(st) == [rc.ERR, rc.OK, rc.REJECTED, rc.REJECTED]


@pytest.mark.parametrize("length", rc.INTERLEAVED_LENGTHS)
@pytest.mark.parametrize("seed", range(4))
def test_interleaved_windows(engine, seed, length):
    case = rc.interleaved(seed, length)
    if length >= 257:  # from the host result alone, before the GPU's is looked at
        shares = rc.class_shares(rc.host_commit(*case)[3])
        assert min(shares.values()) >= rc.MIN_SHARE, shares
    W, widx, ctrs, sts = case
    st, _, _ = check(engine, case)
    untouched = (widx == rc.SKIP) | (widx >= len(W)) | (sts > rc.ERR)
    assert np.array_equal(st[untouched], sts[untouched])


def test_interleaved_windows_beyond_one_tile(engine):
    """Three windows over 4100 packets: three scan tiles, and the third window's first grouped packet lies
    inside the second, so its verdicts depend on the head flag that the carry hands from tile to tile."""
    check(engine, rc.interleaved(0, 4100))


@pytest.mark.parametrize("name", rc.LARGE_NAMES)
def test_large(engine, name):
    """The loops of the grouped scan that run more than once (replay_cases.LARGE_SIZES; test_replay_cpu.py shows
    which loop each size reaches and that the cases hold what they are for): the radix scan with two and three
    entries a lane, two and three radix passes over several tiles, the carry with two tiles a lane, rows whose
    grouped runs span whole tiles, heads on the boundaries of the commit's walk, one contended table slot."""
    case = rc.large_case(name)
    st, _, _ = check(engine, case)
    if name.startswith("strided-"):
        assert (st == rc.OK).all()  # the grouping kept every window's packets in array order
    if name == "same_counter":
        assert list(st[:3]) == [rc.ERR, rc.ERR, rc.OK] and (st[3:] == rc.REJECTED).all()


def test_many_windows_few_packets(engine):
    check(engine, rc.many_windows())


def test_undo_is_optional(engine):
    case = rc.interleaved(1, 257)
    st_h, _, W_h, _ = rc.host_commit(*case)
    st_g, _, W_g = gpu_commit(engine, *case, with_undo=False)
    assert np.array_equal(st_g, st_h) and np.array_equal(W_g, W_h)


def test_argument_errors(engine):
    L, h = engine.library, engine.handle
    W, widx, ctrs, sts = rc.interleaved(2, 65)
    dW = torch.from_numpy(np.concatenate([W.view(np.uint8).reshape(-1), np.zeros(8, np.uint8)])).cuda()
    dw = torch.from_numpy(widx.view(np.int32).copy()).cuda()
    dc = torch.from_numpy(ctrs.view(np.int64).copy()).cuda()
    ds = torch.from_numpy(sts.copy()).cuda()
    ws = engine.replay_workspace(65, 3)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    need = L.rg_replay_workspace_size(65, 3)
    before_W, before_s = dW.cpu().numpy().copy(), ds.cpu().numpy().copy()
    stream = aead._stream_handle(None)
    calls = {
        "short workspace": (p(dW), p(ds), p(ws), need - 1),
        "misaligned windows": (p(dW, 4), p(ds), p(ws), need),
        "null status": (p(dW), None, p(ws), need),
    }
    for what, (win, st, wsp, wlen) in calls.items():
        rc_ = L.rg_replay_batch_dev(h, win, 3, p(dw), p(dc), 65, st, None, wsp, wlen, stream)
        assert rc_ == -1, what  # RG_EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(dW.cpu().numpy(), before_W) and np.array_equal(ds.cpu().numpy(), before_s)
    assert L.rg_replay_batch_dev(h, p(dW), 3, p(dw), p(dc), 0, None, None, None, 0, stream) == 0  # n == 0
