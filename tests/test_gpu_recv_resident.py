"""rg_recv_batch_dev_resident: receiver resolution, would_accept gate, open, in-order commit and re-seal with no
host step.  Frames are sealed with the oracle; the expected statuses come from a model that runs the oracle's
open and the host window functions in replay_step's order (replay_cases.host_commit)."""
import ctypes

import numpy as np
import pytest
import torch

import replay_cases as rc
from oracle import oracle
from rustyguard_amd import aead
from rustyguard_amd.aead import Sessions
from rustyguard_amd.workloads import DESC_DTYPE

pytestmark = pytest.mark.gpu

RECV = np.array([0x1111, 0x3333], np.uint32)  # our receiver ids; key row = window row = index
KEYS = np.random.default_rng(21).integers(0, 256, (2, 32), dtype=np.uint8)
UNALIGNED, NOT_DATA = 4, 5


def _seal(specs, rng, keys=KEYS, recv=RECV):
    """specs: (session, counter, payload bytes) -> list of sealed frames (uint8 arrays)."""
    desc = np.zeros(len(specs), DESC_DTYPE)
    off = 0
    for i, (s, c, p) in enumerate(specs):
        desc[i] = (off, p, s)
        off += p + 32
    buf = rng.integers(0, 256, off, dtype=np.uint8)
    oracle.seal_batch(keys, recv, desc, np.array([c for _, c, _ in specs], np.uint64), buf)
    return [buf[int(d["offset"]):int(d["offset"]) + int(d["len"]) + 32].copy() for d in desc]


def _pack(frames, shift=()):
    """Frames at 16-byte aligned offsets (those in `shift` 8 bytes off) -> (desc, buf)."""
    desc = np.zeros(len(frames), DESC_DTYPE)
    off = 0
    for i, f in enumerate(frames):
        o = off + (8 if i in shift else 0)
        desc[i] = (o, len(f), 0)
        off += (len(f) + 16 + 15) // 16 * 16
    buf = np.zeros(off + 64, np.uint8)
    for d, f in zip(desc, frames):
        buf[int(d["offset"]):int(d["offset"]) + len(f)] = f
    return desc, buf


@pytest.fixture(scope="module")
def traffic():
    rng = np.random.default_rng(22)
    P = lambda: int(rng.integers(1, 10)) * 16  # noqa: E731  W = 48 .. 176
    first = _seal([(0, c, P()) for c in range(8)], rng)  # the previous call
    fr = _seal([(0, 8 + c, P()) for c in range(10)] + [(1, c, P()) for c in range(10)] +
               [(0, 3000, P()), (0, 3000 - 1984, P()), (0, 3000 - 1983, P()), (0, 40, P()), (1, 50, P()),
                (0, 41, P()), (1, 51, P())], rng)
    forged0, forged1 = fr[23].copy(), fr[24].copy()
    forged0[-1] ^= 1
    forged1[20] ^= 0x80
    hdr = lambda t, r, c: np.frombuffer(np.array([t, r], np.uint32).tobytes() + np.uint64(c).tobytes(), np.uint8)  # noqa: E731
    batch = (fr[:6] + [fr[2]] + fr[10:16] + [first[1], first[3], fr[12]] + fr[6:10] +
             [forged0, fr[23], forged1, fr[24]] + fr[16:20] + [fr[20], fr[21], fr[22], first[0]] +
             [np.concatenate([hdr(4, 0x9999, 7), np.zeros(32, np.uint8)]),   # unknown receiver
              np.concatenate([hdr(1, 0, 0), np.zeros(132, np.uint8)])[:144],  # handshake type
              fr[25], fr[26], fr[5], first[7]])
    batch = batch + [first[2]] * (48 - len(batch) - 1) + [fr[25]]
    assert len(batch) == 48
    d1, b1 = _pack(first)
    d2, b2 = _pack(batch, shift={37})
    return d1, b1, d2, b2


def _model(windows, desc, buf, keys=KEYS, recv=RECV):
    """Final statuses, expected buffer, windows, counters and key rows for one call."""
    opened = buf.copy()
    st, ctr, kidx = oracle.open_batch_rx(keys, recv, desc, opened)
    widx = np.where(kidx < len(recv), kidx, rc.SKIP).astype(np.uint32)
    fin, undo, W, _ = rc.host_commit(windows, widx, ctr, st)
    want = buf.copy()
    for i, d in enumerate(desc):
        if fin[i] == rc.OK:
            o, w = int(d["offset"]), int(d["len"])
            want[o:o + w] = opened[o:o + w]
    return fin, want, W, ctr, kidx


class Dev:
    def __init__(self, engine, n, keys=KEYS, recv=RECV):
        self.engine = engine
        self.nkeys = len(recv)
        self.keys = torch.from_numpy(keys.copy()).cuda()
        table = aead.rx_table(recv, np.arange(self.nkeys, dtype=np.uint32))
        self.rx = torch.from_numpy(table.view(np.int32).copy()).cuda()
        self.win = torch.zeros(self.nkeys * 33, dtype=torch.int64, device="cuda")
        self.ws = engine.replay_workspace(n, self.nkeys)

    def recv(self, desc, buf, stream=None):
        n = len(desc)
        dd = torch.from_numpy(desc.view(np.uint8).reshape(-1, 16).copy()).cuda()
        db = torch.from_numpy(buf.copy()).cuda()
        st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        ctr = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        key = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        self.engine.recv_batch_dev_resident(self.keys, self.rx, self.win, dd, db, st, ctr, key, workspace=self.ws,
                                            stream=stream)
        torch.cuda.synchronize()
        return (st.cpu().numpy(), db.cpu().numpy(), ctr.cpu().numpy().view(np.uint64), key.cpu().numpy().view(np.uint32))

    def windows(self):
        return self.win.cpu().numpy().view(np.uint64).reshape(self.nkeys, 33)

    def working_keys(self, n):
        return self.ws[:16 * n].cpu().numpy().view(DESC_DTYPE)["key_idx"]


def _run_both_calls(engine, traffic):
    d1, b1, d2, b2 = traffic
    dev = Dev(engine, 48)
    W = rc.fresh(2)
    for desc, buf in ((d1, b1), (d2, b2)):
        fin, want, W, ctr, kidx = _model(W, desc, buf)
        st, got, gctr, gkey = dev.recv(desc, buf)
        assert list(st) == list(fin)
        assert np.array_equal(got, want)
        assert np.array_equal(dev.windows(), W)
        assert np.array_equal(gkey, kidx)
        data = kidx < 2  # a resolved data frame reports its header counter, gated or not
        assert np.array_equal(gctr[data], ctr[data])
    return dev, fin, W


def test_outcome_coverage(engine, traffic):
    dev, fin, W = _run_both_calls(engine, traffic)
    d2, b2 = traffic[2], traffic[3]
    assert {rc.OK, rc.ERR, rc.REJECTED, UNALIGNED, NOT_DATA} <= set(fin)
    assert list(fin[20:24]) == [rc.ERR, rc.OK, rc.ERR, rc.OK]  # a forged tag, then the genuine frame, twice
    assert fin[6] == rc.REJECTED and fin[29] == rc.REJECTED and fin[30] == rc.OK  # duplicate; 1984 / 1983 behind
    assert fin[13] == rc.REJECTED and fin[32] == rc.REJECTED and fin[33] == NOT_DATA and fin[37] == UNALIGNED
    # the identical batch again: every data frame is stale, none reaches the AEAD
    st, got, _, gkey = dev.recv(d2, b2)
    data = gkey < 2
    assert data.sum() >= 40 and (st[data] == rc.REJECTED).all()
    assert np.array_equal(got, b2) and np.array_equal(dev.windows(), W)
    assert (dev.working_keys(48)[data] == rc.SKIP).all()


def _many_sessions(n=4100, nsess=300, seed=23):
    """n frames of 16-byte payload over nsess sessions (two radix passes over three tiles in the commit): per
    session mostly ascending counters; repeated frames; jumps ahead followed by the frames 1984 and 1983 behind;
    about one frame in twenty with a forged tag or ciphertext, its genuine twin right behind it or ahead of it.
    -> (keys, receiver ids, desc, buf, forged)"""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 256, (nsess, 32), dtype=np.uint8)
    recv = (0x1000 + 7 * rng.permutation(nsess)).astype(np.uint32)
    specs, seq = [], []  # frames to seal: (session, counter, 16); the batch: (index into specs, forged)
    edge, mine = [0] * nsess, [[] for _ in range(nsess)]

    def new(s, c):
        specs.append((s, c, 16))
        mine[s].append(len(specs) - 1)
        edge[s] = max(edge[s], c)
        return len(specs) - 1

    while len(seq) < n:
        s = int(rng.integers(0, nsess))
        kind = rng.random()
        if kind < 0.10 and mine[s]:
            seq.append((mine[s][int(rng.integers(0, len(mine[s])))], False))
        elif kind < 0.15:
            f = new(s, edge[s] + int(rng.integers(1, 4)))
            seq += [(f, True), (f, False)] if rng.random() < 0.5 else [(f, False), (f, True)]
        elif kind < 0.18:
            top = edge[s] + 3000
            seq += [(new(s, top), False), (new(s, top - 1984), False), (new(s, top - 1983), False)]
        else:
            seq.append((new(s, edge[s] + int(rng.integers(1, 4))), False))
    seq = seq[:n]
    sealed = _seal(specs, rng, keys, recv)
    frames = []
    for f, forged in seq:
        fr = sealed[f].copy()
        if forged:
            fr[int(rng.integers(16, 48))] ^= 1 << int(rng.integers(0, 8))  # ciphertext or tag
        frames.append(fr)
    desc, buf = _pack(frames)
    return keys, recv, desc, buf, np.array([forged for _, forged in seq])


def test_many_sessions_beyond_one_tile(engine):
    """4100 frames over 300 sessions: the commit groups by two radix passes over three tiles, and every byte of
    300 windows is the model's.  Then the same batch again: all of it is stale."""
    keys, recv, desc, buf, forged = _many_sessions()
    n, nsess = len(desc), len(recv)
    fin, want, W, ctr, kidx = _model(rc.fresh(nsess), desc, buf, keys, recv)
    # what the batch is there for, from the model alone
    assert (kidx < nsess).all() and len(np.unique(kidx)) == nsess
    assert 0.03 < forged.mean() < 0.07 and (fin[forged] != rc.OK).all()
    assert {rc.OK, rc.ERR, rc.REJECTED} == set(fin)
    assert (fin == rc.ERR).sum() > 50 and (fin[~forged] == rc.REJECTED).sum() > 300
    dev = Dev(engine, n, keys, recv)
    st, got, gctr, gkey = dev.recv(desc, buf)
    assert np.array_equal(st, fin), np.nonzero(st != fin)[0][:10]
    assert np.array_equal(got, want)
    assert np.array_equal(dev.windows(), W)
    assert np.array_equal(gkey, kidx) and np.array_equal(gctr, ctr)
    st, got, _, gkey = dev.recv(desc, buf)
    assert np.array_equal(gkey, kidx) and (st == rc.REJECTED).all()
    assert np.array_equal(got, buf) and np.array_equal(dev.windows(), W)
    assert (dev.working_keys(n) == rc.SKIP).all()


@pytest.mark.parametrize("family", [0, 1, 3])
def test_kernel_families(engine, traffic, family):
    engine.set_staged(family)
    try:
        _run_both_calls(engine, traffic)
        assert engine.last_kernel() == family
    finally:
        engine.set_staged(-1)


def test_matches_session_table(engine, traffic):
    d1, b1, d2, b2 = traffic
    dev = Dev(engine, 48)
    tab = Sessions(engine, 8)
    other = bytes(32)
    slots = [tab.insert(int(RECV[s]), 0x7000 + s, other, KEYS[s].tobytes()) for s in range(2)]
    for desc, buf in ((d1, b1), (d2, b2)):
        st, got, _, _ = dev.recv(desc, buf)
        db = torch.from_numpy(buf.copy()).cuda()
        ds = torch.zeros(len(desc), dtype=torch.uint8, device="cuda")
        tab.recv_batch_dev(torch.from_numpy(desc.view(np.uint8).reshape(-1, 16).copy()).cuda(), db, ds)
        st_t, _, _ = tab.recv_batch_dev_finish(len(desc))
        torch.cuda.synchronize()
        assert list(st) == list(st_t) == list(ds.cpu().numpy())
        assert np.array_equal(got, db.cpu().numpy())
    for s, slot in enumerate(slots):
        host = np.frombuffer(ctypes.string_at(engine.library.rg_sessions_replay(tab._h, slot), 264), np.uint64)
        assert np.array_equal(host, dev.windows()[s])


def test_graph_capture(engine, traffic):
    d1, b1, d2, b2 = traffic
    fin, want, W, _, _ = _model(rc.fresh(2), d2, b2)
    dev = Dev(engine, 48)
    st0, got0, _, _ = dev.recv(d2, b2)  # the direct call (also grows the context's buffers outside the capture)
    assert list(st0) == list(fin) and np.array_equal(got0, want)
    dev.win.zero_()
    dd = torch.from_numpy(d2.view(np.uint8).reshape(-1, 16).copy()).cuda()
    db = torch.from_numpy(b2.copy()).cuda()
    st = torch.full((48,), 0xEE, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin()
        engine.recv_batch_dev_resident(dev.keys, dev.rx, dev.win, dd, db, st, workspace=dev.ws, stream=s)
        g.capture_end()
    torch.cuda.synchronize()
    assert np.array_equal(db.cpu().numpy(), b2) and not dev.windows().any()  # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert list(st.cpu().numpy()) == list(fin)
    assert np.array_equal(db.cpu().numpy(), want) and np.array_equal(dev.windows(), W)
    db.copy_(torch.from_numpy(b2))  # frames restored, windows kept: everything is stale now
    g.replay()
    torch.cuda.synchronize()
    data = np.array([int(k) < 2 for k in _model(rc.fresh(2), d2, b2)[4]])
    assert (st.cpu().numpy()[data] == rc.REJECTED).all()
    assert np.array_equal(db.cpu().numpy(), b2) and np.array_equal(dev.windows(), W)
