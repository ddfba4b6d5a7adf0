"""rg_send_batch_dev_resident: counters reserved on the device, then the seal, with no host step.  The expected
counters and verdicts come from the array-order loop (send_cases.loop), the expected frames from the oracle's
seal under those counters; a second witness is the host session table (rg_send_batch_dev)."""
import numpy as np
import pytest
import torch

import send_cases as sc
from oracle import oracle
from rustyguard_amd.aead import Sessions
from rustyguard_amd.workloads import DESC_DTYPE

pytestmark = pytest.mark.gpu

NK = 3
KEYS = np.random.default_rng(31).integers(0, 256, (NK, 32), dtype=np.uint8)
RECV = np.array([0x1111, 0x3333, 0x5555], np.uint32)  # the peers' receiver ids; key row = state row = index
PAYLOADS = (0, 16, 64, 1504)


def _frames(sizes, rng, shift=()):
    """Plaintext frames at 16-byte aligned offsets (those in `shift` 8 bytes off) -> (desc, buf)."""
    desc = np.zeros(len(sizes), DESC_DTYPE)
    off = 0
    for i, p in enumerate(sizes):
        desc[i] = (off + (8 if i in shift else 0), p, 0xABCD)  # key_idx is ignored
        off += (int(p) + 32 + 16 + 15) // 16 * 16
    return desc, rng.integers(0, 256, off + 64, dtype=np.uint8)


def _i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()


def _model(state, slots, desc, buf, now, keys=KEYS, recv=RECV):
    """-> (final status, counters, rekey, state', frames) for descriptors that all lie in the buffer, aligned."""
    st, ctr, rk, S = sc.loop(state, slots, desc["len"], now)
    took = st == sc.PENDING
    want = buf.copy()
    if took.any():
        d = desc[took].copy()
        d["key_idx"] = np.asarray(slots, np.uint32)[took]
        oracle.seal_batch(keys, recv, d, ctr[took], want)
    return np.where(took, sc.OK, st).astype(np.uint8), ctr, rk, S, want


class Dev:
    def __init__(self, engine, state, n, keys=KEYS, recv=RECV):
        self.engine = engine
        self.model_keys = keys, recv
        self.keys = torch.from_numpy(keys.copy()).cuda()
        self.recv = torch.from_numpy(recv.view(np.int32).copy()).cuda()
        self.state = _i64(np.asarray(state, np.uint64).reshape(-1))
        self.ws = engine.send_workspace(n, len(recv))

    def send(self, slots, desc, buf, now, stream=None, outputs=True):
        n = len(desc)
        ds = torch.from_numpy(np.asarray(slots, np.uint32).view(np.int32).copy()).cuda()
        dd = torch.from_numpy(desc.view(np.uint8).reshape(-1, 16).copy()).cuda()
        db = torch.from_numpy(buf.copy()).cuda()
        st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        ctr = torch.full((n,), -1, dtype=torch.int64, device="cuda") if outputs else None
        rk = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda") if outputs else None
        dn = None if now is None else _i64(np.array([now], np.uint64))
        self.engine.send_batch_dev_resident(self.keys, self.recv, self.state, ds, dd, db, st, ctr, rk, dn,
                                            workspace=self.ws, stream=stream)
        torch.cuda.synchronize()
        return (st.cpu().numpy(), ctr.cpu().numpy().view(np.uint64) if outputs else None,
                rk.cpu().numpy() if outputs else None, db.cpu().numpy())

    def rows(self):
        return self.state.cpu().numpy().view(np.uint64).reshape(-1, 3)


def _traffic(n, seed, ineligible=True):
    rng = np.random.default_rng(seed)
    sizes = rng.choice(PAYLOADS, n).astype(np.uint32)
    slots = rng.integers(0, NK, n).astype(np.uint32)
    if ineligible:
        kind = rng.integers(0, 10, n)
        slots[kind == 0] = sc.SKIP
        slots[kind == 1] = NK + 4
        sizes[kind == 2] += 8  # len % 16 != 0: RG_PKT_INVALID, no counter, frame untouched
    desc, buf = _frames(sizes, rng)
    return slots, desc, buf


def _check(dev, state, slots, desc, buf, now, outputs=True):
    fin, ctr, rk, S, want = _model(state, slots, desc, buf, now, *dev.model_keys)
    st, gctr, grk, got = dev.send(slots, desc, buf, now, outputs=outputs)
    assert np.array_equal(st, fin), np.nonzero(st != fin)[0][:10]
    if outputs:
        assert np.array_equal(gctr, ctr) and np.array_equal(grk, rk)
    assert np.array_equal(got, want)  # sealed frames byte for byte; rejected and invalid ones, and the gaps, untouched
    assert np.array_equal(dev.rows(), S)
    return fin, S


START = np.array([[(1 << 32) - 40, sc.T0, sc.T0], [sc.REKEY - 30, sc.T0, sc.T0], [sc.REJECT - 25, sc.T0, sc.T0]], np.uint64)


@pytest.mark.parametrize("family", [0, 1, 2, 3])
def test_kernel_families(engine, family):
    slots, desc, buf = _traffic(300, 40 + family)
    engine.set_staged(family)
    try:
        dev = Dev(engine, START, 300)
        fin, S = _check(dev, START, slots, desc, buf, sc.T0 + 9)
        assert engine.last_kernel() == family
        assert {sc.OK, sc.INVALID, sc.REJECTED} == set(fin)
        assert int(S[2, 0]) == sc.REJECT  # row 2 ran out inside the batch
        # the next batch continues the counters; row 2 is shut
        slots2, desc2, buf2 = _traffic(65, 50 + family, ineligible=False)
        fin2, _ = _check(dev, S, slots2, desc2, buf2, sc.T0 + 10)
        assert (fin2[slots2 == 2] == sc.REJECTED).all() and (fin2[slots2 != 2] == sc.OK).all()
    finally:
        engine.set_staged(-1)


@pytest.mark.parametrize("n,nrows", [(1, 1), (64, 3), (65, 3), (2049, 1), (4097, 3)])
def test_sizes(engine, n, nrows):
    rng = np.random.default_rng(60 + n)
    sizes = rng.choice(PAYLOADS[:3] if n > 300 else PAYLOADS, n).astype(np.uint32)
    slots = rng.integers(0, nrows, n).astype(np.uint32)
    desc, buf = _frames(sizes, rng)
    state = sc.rows((1 << 32) - 100, 7, 1 << 40)
    dev = Dev(engine, state, n)
    fin, _ = _check(dev, state, slots, desc, buf, sc.T0 + 9)
    assert (fin == sc.OK).all()


def test_size_8193_rows_300(engine):
    """Two radix passes over five tiles, the radix scan with two entries a lane (send_cases.LARGE_SIZES), then
    the seal: 300 keys, rows skewed so that one row's grouped run spans whole tiles."""
    n, nrows = 8193, 300
    rng = np.random.default_rng(61)
    keys = rng.integers(0, 256, (nrows, 32), dtype=np.uint8)
    recv = (0x1000 + 7 * rng.permutation(nrows)).astype(np.uint32)
    sizes = rng.choice((16, 32, 48), n).astype(np.uint32)
    slots = sc.skewed_rows(rng, n, np.arange(nrows))
    desc, buf = _frames(sizes, rng)
    state = np.empty((nrows, 3), np.uint64)
    state[:, 0] = rng.integers(0, 1 << 40, nrows)
    state[:, 1:] = sc.T0
    state[sc.heavy_rows(np.arange(nrows))[0], 0] = (1 << 32) - 100  # the heavy row's counters cross 2^32
    dev = Dev(engine, state, n, keys, recv)
    fin, S = _check(dev, state, slots, desc, buf, sc.T0 + 9)
    assert (fin == sc.OK).all() and len(np.unique(slots)) == nrows
    assert int(S[:, 0].sum() - state[:, 0].sum()) == n and int(np.bincount(slots).max()) > n // 2 - 200


def test_optional_outputs_and_no_clock(engine):
    slots, desc, buf = _traffic(130, 70)
    dev = Dev(engine, START, 130)
    _, S = _check(dev, START, slots, desc, buf, None, outputs=False)
    assert np.array_equal(S[:, 1:], START[:, 1:])  # sent_ns untouched without a clock


def test_expired_row_is_left_alone(engine):
    now = sc.T0 + sc.REJECT_AFTER_TIME + 1
    state = np.array([[5, sc.T0, 1], [6, sc.T0 + 1, 2], [7, now, 3]], np.uint64)  # expired, at the limit, fresh
    slots, desc, buf = _traffic(200, 71, ineligible=False)
    dev = Dev(engine, state, 200)
    fin, S = _check(dev, state, slots, desc, buf, now)
    assert (fin[slots == 0] == sc.REJECTED).all() and (fin[slots != 0] == sc.OK).all()
    assert list(S[:, 2]) == [1, now, now]


def test_bad_frames_consume_their_counters(engine):
    """A misaligned and an out-of-bounds frame report what rg_seal_batch_dev reports for the same descriptor, stay
    untouched, and have taken their counters (as in rg_send_batch: nonces stay unique)."""
    rng = np.random.default_rng(72)
    n = 40
    sizes = rng.choice(PAYLOADS, n).astype(np.uint32)
    desc, buf = _frames(sizes, rng, shift={7})
    desc["offset"][21] = (len(buf) - 48) // 16 * 16  # 64 + 32 bytes do not fit behind it
    desc["len"][21] = 64
    slots = (np.arange(n) % 2).astype(np.uint32)
    state = sc.rows(100, 200, 300)
    st_l, ctr_l, rk_l, S_l = sc.loop(state, slots, desc["len"], sc.T0 + 9)
    assert (st_l == sc.PENDING).all() and int(S_l[1, 0]) == 220  # 7 and 21 are row 1's: 20 counters gone
    # the witness: rg_seal_batch_dev over the same descriptors under the loop's counters
    work = desc.copy()
    work["key_idx"] = slots
    wb = torch.from_numpy(buf.copy()).cuda()
    wst = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    dev = Dev(engine, state, n)
    engine.seal_dev(dev.keys, dev.recv, torch.from_numpy(work.view(np.uint8).reshape(-1, 16).copy()).cuda(),
                    _i64(ctr_l), wb, wst)
    torch.cuda.synchronize()
    st, ctr, _, got = dev.send(slots, desc, buf, sc.T0 + 9)
    assert np.array_equal(st, wst.cpu().numpy()) and np.array_equal(got, wb.cpu().numpy())
    # (the seal kernels report both as RG_PKT_INVALID; the witness above is what binds)
    assert st[7] in (sc.UNALIGNED, sc.INVALID) and st[21] == sc.INVALID and (np.delete(st, [7, 21]) == sc.OK).all()
    assert np.array_equal(ctr, ctr_l) and np.array_equal(dev.rows(), S_l)
    good = np.ones(n, bool)
    good[[7, 21]] = False
    want = buf.copy()
    d = work[good].copy()
    oracle.seal_batch(KEYS, RECV, d, ctr_l[good], want)
    assert np.array_equal(got, want)


def test_keepalive_frame(engine):
    """An empty payload seals to the 32-byte frame the oracle gives: header and tag."""
    desc, buf = _frames([0], np.random.default_rng(73))
    state = sc.rows(41, 42, 43)
    dev = Dev(engine, state, 1)
    fin, ctr, _, S, want = _model(state, [1], desc, buf, sc.T0 + 9)
    st, gctr, _, got = dev.send([1], desc, buf, sc.T0 + 9)
    assert list(st) == [sc.OK] and list(gctr) == [42] and np.array_equal(got, want)
    frame = got[:32]
    assert bytes(frame[:16]) == np.array([4, 0x3333], np.uint32).tobytes() + np.uint64(42).tobytes()
    assert not np.array_equal(frame[16:32], buf[16:32]) and np.array_equal(got[32:], buf[32:])
    assert int(dev.rows()[1, 2]) == sc.T0 + 9  # sent_ns: what the keepalive rule reads


def test_matches_session_table(engine):
    """The host session table driven through rg_send_batch_dev on the same slots and frames."""
    t_ins, now = sc.T0, sc.T0 + 5 * 10**9
    tab = Sessions(engine, 8)
    tab.set_time(t_ins)
    slot_of = [tab.insert(0x7000 + s, int(RECV[s]), KEYS[s].tobytes(), bytes(32)) for s in range(NK)]
    assert slot_of == list(range(NK))  # key row = slot
    start = [7, sc.REKEY - 20, sc.REJECT - 30]
    for s, c in enumerate(start):
        tab.set_send_counter(s, c)
    state = np.array([[c, t_ins, t_ins] for c in start], np.uint64)  # started_ns is the insert time
    dev = Dev(engine, state, 400)
    rng = np.random.default_rng(74)
    for step, (n, clock) in enumerate([(400, now), (130, now + 1), (64, t_ins + sc.REJECT_AFTER_TIME + 1)]):
        sizes = rng.choice(PAYLOADS, n).astype(np.uint32)
        slots = rng.integers(0, NK + 1, n).astype(np.uint32)
        slots[slots == NK] = 6  # a slot without a session: beyond the device's rows, unused in the table
        desc, buf = _frames(sizes, rng)
        tab.set_time(clock)
        db = torch.from_numpy(buf.copy()).cuda()
        ds = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        rk_t = tab.send_batch_dev(slots, torch.from_numpy(desc.view(np.uint8).reshape(-1, 16).copy()).cuda(), db, ds)
        st, _, rk, got = dev.send(slots, desc, buf, clock)
        assert np.array_equal(st, ds.cpu().numpy()) and np.array_equal(rk, rk_t)
        assert np.array_equal(got, db.cpu().numpy())
        assert [int(c) for c in dev.rows()[:, 0]] == [tab.send_counter(s) for s in range(NK)]
        if step == 0:
            assert rk.any() and {sc.OK, sc.REJECTED} == set(st)
        if step == 2:
            assert (st == sc.REJECTED).all() and np.array_equal(got, buf)  # every session has expired


def test_graph_capture(engine):
    n = 130
    slots, desc, buf = _traffic(n, 75)
    state = sc.rows(10, (1 << 32) - 50, sc.REKEY - 60)
    dev = Dev(engine, state, n)
    _, S = _check(dev, state, slots, desc, buf, sc.T0 + 9)  # the direct call (also grows the context's buffers)
    ds = torch.from_numpy(slots.view(np.int32).copy()).cuda()
    dd = torch.from_numpy(desc.view(np.uint8).reshape(-1, 16).copy()).cuda()
    db = torch.from_numpy(buf.copy()).cuda()
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    ctr = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    rk = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    dn = _i64(np.array([0], np.uint64))
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin()
        engine.send_batch_dev_resident(dev.keys, dev.recv, dev.state, ds, dd, db, st, ctr, rk, dn, workspace=dev.ws,
                                       stream=s)
        g.capture_end()
    torch.cuda.synchronize()
    assert np.array_equal(db.cpu().numpy(), buf) and np.array_equal(dev.rows(), S)  # captured, not run
    took = []
    # three replays, *now_ns rewritten in between; the last clock expires every row
    for clock in (sc.T0 + 20, sc.T0 + 30, sc.T0 + sc.REJECT_AFTER_TIME + 1):
        fin, c_w, rk_w, S, want = _model(S, slots, desc, buf, clock)
        db.copy_(torch.from_numpy(buf))  # plaintext again; the state rows carry on
        dn.copy_(_i64(np.array([clock], np.uint64)))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(st.cpu().numpy(), fin) and np.array_equal(ctr.cpu().numpy().view(np.uint64), c_w)
        assert np.array_equal(rk.cpu().numpy(), rk_w) and np.array_equal(db.cpu().numpy(), want)
        assert np.array_equal(dev.rows(), S)
        took.append(int((fin == sc.OK).sum()))
        assert list(S[:2, 2]) == ([clock] * 2 if took[-1] else [sc.T0 + 30] * 2)
    per_call = int((slots == 0).sum() - ((slots == 0) & (desc["len"] % 16 != 0)).sum())
    assert took[0] > 60 and took[1] == took[0] and took[2] == 0
    assert int(S[0, 0]) == 10 + 3 * per_call  # the direct call and two replays, each continuing the last
