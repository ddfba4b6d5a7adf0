"""rg_handshake_initiate_batch_dev and rg_handshake_finish_batch_dev on the GPU against the Python model
(tests/initiator_cases.py), against the responder calls of the same library (a handshake from GPU to GPU) and
against the reference's recorded handshakes.  Every status and every byte of every message, pending row and key
row is compared; nothing is approximate."""
import ctypes

import numpy as np
import pytest

import handshake_cases as hc
import initiator_cases as ic
from conftest import load_golden
from rustyguard_amd import aead
from rustyguard_amd.workloads import DESC_DTYPE

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL = 0xA5
INITIATE_COUNTS = [("valid", 80), ("valid_cookie", 60), ("gated", 20), ("bad_peer", 20), ("low_order_peer", 20)]


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _fill(shape, dtype=torch.uint8):
    if dtype == torch.uint8:
        return torch.full(shape, FILL, dtype=dtype, device="cuda")
    return torch.full(shape, 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device="cuda")  # the same bytes


def _kinds(counts, seed):
    kinds = [k for k, c in counts for _ in range(c)]
    order = np.random.default_rng(seed).permutation(len(kinds))
    return [kinds[i] for i in order]


# ------------------------------------------------------------------ initiate
def _initiate(engine, ini, b, gate, n=None, stream=None):
    """One call over the batch b of ic.initiate_batch: (messages, pending, status) with one guard row each."""
    n = len(b["peer_idx"]) if n is None else n
    msgs, pend, st = _fill((n + 1, 160)), _fill((n + 1, 128)), _fill((n + 1,))
    engine.handshake_initiate_dev(_dev(ini.own), _dev(b["peers"]), _dev(b["peer_idx"][:n]),
                                  None if gate is None else _dev(gate[:n]), _dev(b["esk"][:n]), _dev(b["ts"][:n]),
                                  _dev(b["sids"][:n]), _dev(b["cookies"][:n]), _dev(b["has_cookie"][:n]), msgs[:n],
                                  pend[:n], st[:n], stream=stream)
    torch.cuda.synchronize()
    m, p, s = msgs.cpu().numpy(), pend.cpu().numpy(), st.cpu().numpy()
    assert (m[n:] == FILL).all() and (p[n:] == FILL).all() and (s[n:] == FILL).all()
    return m[:n], p[:n], s[:n]


def _check_initiate(b, kinds, m, p, s):
    for i, (k, want) in enumerate(zip(kinds, b["want"])):
        if want is None:  # gated: the status alone, the rows untouched
            assert s[i] == ic.REJECTED and (m[i] == FILL).all() and (p[i] == FILL).all(), (i, k)
            continue
        assert (int(s[i]), m[i].tobytes(), p[i].tobytes()) == want, (i, k)


@pytest.fixture(scope="module")
def initiate_world():
    ini = ic.Initiator(2026)
    kinds = _kinds(INITIATE_COUNTS, 13)
    return ini, kinds, ic.initiate_batch(ini, kinds)


def test_initiate_mixed_batch_vs_model(engine, initiate_world):
    """200 rows over 5 peers in five categories, dealt by a seeded permutation: every status, every byte of
    every message row and pending row (zero rows with peer = RG_PEER_NONE for a failure, nothing written for a
    gated row); gate = NULL equals a gate of all RG_PKT_OK."""
    ini, kinds, b = initiate_world
    want_st = {"valid": ic.OK, "valid_cookie": ic.OK, "bad_peer": ic.INVALID, "low_order_peer": ic.KEYEXCHANGE}
    for k, w in zip(kinds, b["want"]):  # the model agrees with the header's table
        assert (w is None) if k == "gated" else (w[0] == want_st[k]), k
    m, p, s = _initiate(engine, ini, b, b["gate"])
    _check_initiate(b, kinds, m, p, s)
    ok = s == ic.OK
    assert ok.sum() == 140 and (m[ok][:, 148:] == 0).all()
    assert (m[ok & (b["has_cookie"] == 0)][:, 132:148] == 0).all() and m[ok & (b["has_cookie"] != 0)][:, 132:148].any(1).all()
    assert set(np.ascontiguousarray(p[ok][:, 96:100]).view(np.uint32).ravel()) == set(range(5))
    # without a gate the gated rows are judged like any other: here they are valid
    m_n, p_n, s_n = _initiate(engine, ini, b, None)
    m_z, p_z, s_z = _initiate(engine, ini, b, np.zeros(len(kinds), np.uint8))
    assert np.array_equal(m_n, m_z) and np.array_equal(p_n, p_z) and np.array_equal(s_n, s_z)
    for i, k in enumerate(kinds):
        if k != "gated":
            assert (int(s_n[i]), m_n[i].tobytes(), p_n[i].tobytes()) == b["want"][i], i
            continue
        want = ic.initiate(ini.sk_i, b["peer_list"], int(b["peer_idx"][i]), b["esk"][i].tobytes(), b["ts"][i].tobytes(),
                           int(b["sids"][i]), None)
        assert want[0] == ic.OK and (int(s_n[i]), m_n[i].tobytes(), p_n[i].tobytes()) == want, i


@pytest.mark.parametrize("n", [1, 65])
def test_initiate_small_batches(engine, initiate_world, n):
    """one lane; one wave plus one lane: the first n rows of the mixed batch."""
    ini, kinds, b = initiate_world
    m, p, s = _initiate(engine, ini, b, b["gate"], n=n)
    _check_initiate(b, kinds[:n], m, p, s)
    assert n == 1 or len(set(kinds[:n])) == 5


# -------------------------------------------------------------------- finish
class Finish:
    """A FinishWorld on the device with one batch of messages and the model's verdicts."""

    def __init__(self, seed, plan, npending=40):
        self.w = w = ic.FinishWorld(seed, npending)
        self.plan = plan
        self.desc, self.gate, self.buf, self.msgs, self.flags = ic.finish_batch(w, plan, DESC_DTYPE)
        self.peers = hc.peer_rows(w.ini.peers)
        self.rows = np.frombuffer(b"".join(w.pending), np.uint8).reshape(npending, 128).copy()
        self.table = aead.pending_table(self.rows)
        assert {int(r): int(k) for r, k in self.table if k != ic.KEY_SKIP} == \
            {s: r for s, r in w.table.items() if r not in w.consumed}
        # the rows consumed earlier keep their table entries, as a finished handshake's session keeps its id
        self.table = aead.pending_table(w.sids)
        self.d_own, self.d_peers, self.d_table = _dev(w.ini.own), _dev(self.peers), _dev(self.table)
        self.d_desc, self.d_buf = _dev(self.desc.view(np.uint8).reshape(-1, 16)), _dev(self.buf)
        self.n = len(plan)

    def outputs(self):
        n = self.n
        return (_fill((n + 1, 64)), _fill((n + 1,), torch.int32), _fill((n + 1,), torch.int32),
                _fill((len(self.rows) + 1,), torch.int32), _fill((n + 1,)))

    def call(self, engine, d_pending, gate, out, stream=None):
        n = self.n
        keys, pidx, remote, claim, st = out
        engine.handshake_finish_dev(self.d_own, self.d_peers, self.d_table, d_pending[:len(self.rows)], self.d_desc,
                                    gate, self.d_buf, keys[:n], pidx[:n], remote[:n], claim[:len(self.rows)], st[:n],
                                    stream=stream)

    def read(self, d_pending, out):
        """host copies, the guard rows checked: (statuses, key rows, pending rows out, remote ids, pending)."""
        n, npend = self.n, len(self.rows)
        keys, pidx, remote, claim, st = (t.cpu().numpy() for t in out)
        pend = d_pending.cpu().numpy()
        guard = np.uint32(0xA5A5A5A5)
        assert (keys[n:] == FILL).all() and (st[n:] == FILL).all() and (pend[npend:] == FILL).all()
        assert pidx.view(np.uint32)[n] == guard and remote.view(np.uint32)[n] == guard
        assert claim.view(np.uint32)[npend] == guard
        assert np.array_equal(self.d_buf.cpu().numpy(), self.buf)  # buf is never written
        return (list(st[:n]), [k.tobytes() for k in keys[:n]], [int(x) for x in pidx.view(np.uint32)[:n]],
                [int(x) for x in remote.view(np.uint32)[:n]], [r.tobytes() for r in pend[:npend]])

    def pending_dev(self):
        t = _fill((len(self.rows) + 1, 128))
        t[:len(self.rows)] = _dev(self.rows)
        return t

    def model(self, pending):
        w = self.w
        return ic.commit(self.msgs, self.flags, w.table, pending, w.ini.sk_i, w.ini.peers)


def _finish_plan():
    """200 messages against 40 pending rows (37 live): 30 rows get exactly one valid response, the others are
    hit by duplicates and failures.  Indices 3 and 130 (different workgroups) both hold a valid response for
    row 30; index 5 holds a forged one for row 31 and index 140 the valid one."""
    rng = np.random.default_rng(99)
    fails = [("tag_flipped", 14), ("eph_zero", 8), ("eph_one", 8), ("type1", 10), ("len148", 10), ("offset8", 10),
             ("past_buf", 8), ("gated", 14), ("key_skip", 10), ("unknown_receiver", 12), ("consumed_row", 10),
             ("bad_peer_row", 6)]
    plan = [("valid", r) for r in range(30)] + [(k, int(rng.integers(32, 37))) for k, c in fails for _ in range(c)]
    plan += [("valid", int(rng.integers(32, 35))) for _ in range(200 - 4 - len(plan))]  # more duplicates: rows 32-34
    order = rng.permutation(len(plan))
    plan = [plan[i] for i in order]
    for at, item in ((3, ("valid", 30)), (5, ("tag_flipped", 31)), (130, ("valid", 30)), (140, ("valid", 31))):
        plan.insert(at, item)
    assert len(plan) == 200 and plan[3] == plan[130] == ("valid", 30) and plan[5][1] == plan[140][1] == 31
    return plan


@pytest.fixture(scope="module")
def finish_world():
    return Finish(2027, _finish_plan())


def test_finish_mixed_batch_vs_model(engine, finish_world):
    """every status, key row, pend_idx_out, remote_out and the pending array afterwards against the in-order
    loop; of two valid duplicates the lower index wins, a forged lower duplicate does not stop the valid higher
    one; buf untouched.  The same messages again: every formerly finished message is RG_PKT_REJECTED and the
    pending rows stay as the first call left them."""
    f = finish_world
    want = f.model(f.w.pending)
    st = want[0]
    kinds = [k for k, _ in f.plan]
    assert st[3] == ic.OK and st[130] == ic.REJECTED and st[5] == ic.DECRYPT_ERR and st[140] == ic.OK
    assert want[2][3] == 30 and want[2][140] == 31 and want[4][30] == want[4][31] == ic.ZERO_PENDING
    want_kind = {"tag_flipped": {ic.DECRYPT_ERR}, "eph_zero": {ic.KEYEXCHANGE}, "eph_one": {ic.KEYEXCHANGE}, "type1": {ic.INVALID}, "len148": {ic.INVALID},
                 "offset8": {ic.UNALIGNED}, "past_buf": {ic.INVALID}, "gated": {ic.REJECTED}, "key_skip": {ic.REJECTED},
                 "unknown_receiver": {ic.REJECTED}, "consumed_row": {ic.REJECTED}, "bad_peer_row": {ic.INVALID},
                 "valid": {ic.OK, ic.REJECTED}}
    for k, s in zip(kinds, st):  # the model agrees with the header's table
        assert s in want_kind[k], k
    assert st.count(ic.OK) == 35 and {ic.DECRYPT_ERR, ic.KEYEXCHANGE, ic.UNALIGNED, ic.INVALID} <= set(st)
    d_pending, out = f.pending_dev(), f.outputs()
    f.call(engine, d_pending, _dev(f.gate), out)
    torch.cuda.synchronize()
    got = f.read(d_pending, out)
    for name, g, w_ in zip(("status", "keys", "pend_idx", "remote", "pending"), got, want):
        bad = [i for i, (x, y) in enumerate(zip(g, w_)) if x != y]
        assert not bad, (name, bad[:10], [kinds[i] for i in bad[:10]] if name != "pending" else None)
    claim = out[3].cpu().numpy().view(np.uint32)
    assert claim[30] == 3 and claim[31] == 140 and claim[f.w.bad_peer] == 0xFFFFFFFF
    # again, against what the first call left
    out2 = f.outputs()
    f.call(engine, d_pending, _dev(f.gate), out2)
    torch.cuda.synchronize()
    got2, want2 = f.read(d_pending, out2), f.model(want[4])
    assert got2 == want2
    assert all(s2 == ic.REJECTED for s1, s2 in zip(st, got2[0]) if s1 == ic.OK)
    assert got2[4] == got[4] and all(k == bytes(64) for k in got2[1]) and ic.OK not in got2[0]
    # gate = NULL: the gated messages are judged like any other
    d_pending, out3 = f.pending_dev(), f.outputs()
    f.call(engine, d_pending, None, out3)
    torch.cuda.synchronize()
    w = f.w
    want3 = ic.commit(f.msgs, [{} if k == "gated" else kw for k, kw in zip(kinds, f.flags)], w.table, w.pending,
                      w.ini.sk_i, w.ini.peers)
    assert f.read(d_pending, out3) == want3


@pytest.mark.parametrize("n", [1, 65])
def test_finish_small_batches(engine, n):
    """one lane; one wave plus one lane, the last lane a duplicate of lane 0 (another workgroup)."""
    plan = [("valid", 0)] if n == 1 else (
        [("valid", r) for r in range(8)] + [(k, 8) for k in ic.FINISH_KINDS[1:] for _ in range(4)] +
        [("valid", 9 + r) for r in range(8)] + [("valid", 0)])
    assert len(plan) == n
    f = Finish(2028, plan, npending=20)
    d_pending, out = f.pending_dev(), f.outputs()
    f.call(engine, d_pending, _dev(f.gate), out)
    torch.cuda.synchronize()
    got, want = f.read(d_pending, out), f.model(f.w.pending)
    assert got == want
    assert want[0][0] == ic.OK and (n == 1 or want[0][64] == ic.REJECTED)


def test_finish_graph_replay(engine, finish_world):
    """one finish call (memset, kernel, commit) captured into a graph: the first replay equals the eager
    result, the second finds every formerly finished row consumed."""
    f = finish_world
    want = f.model(f.w.pending)
    d_pending, out, d_gate = f.pending_dev(), f.outputs(), _dev(f.gate)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        f.call(engine, d_pending, d_gate, out, stream=s)
    torch.cuda.synchronize()
    d_pending[:len(f.rows)] = _dev(f.rows)  # whatever the capture did or did not run, start from the rows
    for t in out:
        t.fill_(FILL if t.dtype == torch.uint8 else 0xA5A5A5A5 - (1 << 32))
    g.replay()
    torch.cuda.synchronize()
    assert f.read(d_pending, out) == want
    g.replay()
    torch.cuda.synchronize()
    got2 = f.read(d_pending, out)
    assert got2 == f.model(want[4])
    assert all(s2 == ic.REJECTED for s1, s2 in zip(want[0], got2[0]) if s1 == ic.OK) and got2[4] == want[4]


# ---------------------------------------------------------------- GPU to GPU
def test_gpu_to_gpu_handshake_and_transport(engine):
    """initiate -> filter -> init -> response -> finish on one stream, chained through the status arrays with no
    host step; one initiation's mac1 is broken on the device and drops out at the filter.  Both ends derive
    mirrored keys, and with them inserted into two session tables a packet crosses in each direction."""
    rng = np.random.default_rng(8)
    rb = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
    n = 7
    sk_a, sk_b, other = rb(32), rb(32), [hc.pubkey(rb(32)) for _ in range(3)]
    pk_a, pk_b = hc.pubkey(sk_a), hc.pubkey(sk_b)
    psk = rb(32)
    peers_a = [(other[0], rb(32), hc.mac1_key(other[0])), (pk_b, psk, hc.mac1_key(pk_b))]  # B is A's row 1
    peers_b = [(other[1], rb(32), hc.mac1_key(other[1])), (other[2], rb(32), hc.mac1_key(other[2])),
               (pk_a, psk, hc.mac1_key(pk_a))]  # A is B's row 2
    rows_b = hc.peer_rows(peers_b)
    sid_a = np.arange(n, dtype=np.uint32) * 3 + 0x0A00
    sid_b = np.arange(n, dtype=np.uint32) * 5 + 0x0B00
    desc_i = np.array([(160 * i, 148, 0) for i in range(n)], DESC_DTYPE)
    desc_r = np.array([(96 * i, 92, 0) for i in range(n)], DESC_DTYPE)
    ck = hc.mac1_key(pk_b) + rb(64)  # B's filter: its own mac1 key, a cookie key, a secret
    addrs = np.frombuffer(b"".join(aead.encode_src_addr("192.0.2.%d" % i, 4000 + i) for i in range(n)), np.uint8)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a_own, a_peers = _dev(np.frombuffer(sk_a + pk_a, np.uint8)), _dev(hc.peer_rows(peers_a))
        b_own, b_peers, b_table = _dev(np.frombuffer(sk_b + pk_b, np.uint8)), _dev(rows_b), _dev(aead.peer_table(rows_b))
        a_pidx, a_esk = _dev(np.ones(n, np.uint32)), _dev(rng.integers(0, 256, (n, 32), dtype=np.uint8))
        a_ts = _dev(np.frombuffer(b"".join(hc.tai64n(1_900_000_000, i) for i in range(n)), np.uint8).reshape(n, 12))
        a_sid, b_sid, b_esk = _dev(sid_a), _dev(sid_b), _dev(rng.integers(0, 256, (n, 32), dtype=np.uint8))
        a_table = _dev(aead.pending_table(sid_a))
        d_desc_i, d_desc_r = _dev(desc_i.view(np.uint8).reshape(-1, 16)), _dev(desc_r.view(np.uint8).reshape(-1, 16))
        d_ck, d_addrs = _dev(np.frombuffer(ck, np.uint8)), _dev(addrs.reshape(n, 24))
        d_over, d_nonces = _dev(np.zeros(n, np.uint8)), _dev(rng.integers(0, 256, (n, 24), dtype=np.uint8))
        msgs, pending = torch.zeros((n, 160), dtype=torch.uint8, device="cuda"), _fill((n, 128))
        replies, results = torch.zeros((n, 64), dtype=torch.uint8, device="cuda"), _fill((n, 128))
        responses, keys_b, keys_a = _fill((n, 96)), _fill((n, 64)), _fill((n, 64))
        st = [_fill((n,)) for _ in range(5)]
        pidx, remote, claim = _fill((n,), torch.int32), _fill((n,), torch.int32), _fill((n,), torch.int32)
    s.synchronize()
    with torch.cuda.stream(s):
        engine.handshake_initiate_dev(a_own, a_peers, a_pidx, None, a_esk, a_ts, a_sid, None, None, msgs, pending, st[0],
                                      stream=s)
        msgs[2, 120] ^= 1  # mac1 broken on its way
        engine.cookie_reply_dev(d_ck, d_desc_i, d_addrs, d_over, d_nonces, msgs, replies, st[1], stream=s)
        engine.handshake_init_dev(b_own, b_peers, b_table, d_desc_i, st[1], msgs, results, st[2], stream=s)
        engine.handshake_resp_dev(b_peers, results, st[2], b_esk, b_sid, None, None, responses, keys_b, st[3], stream=s)
        engine.handshake_finish_dev(a_own, a_peers, a_table, pending, d_desc_r, st[3], responses, keys_a, pidx, remote,
                                    claim, st[4], stream=s)
    s.synchronize()
    want = [ic.OK] * n
    assert list(st[0].cpu().numpy()) == want
    want[2] = ic.REJECTED
    for t in st[1:]:
        assert list(t.cpu().numpy()) == want
    ka, kb = keys_a.cpu().numpy(), keys_b.cpu().numpy()
    live = [i for i in range(n) if i != 2]
    assert (ka[2] == 0).all() and (kb[2] == FILL).all()  # the response call never touched the gated row
    assert list(pidx.cpu().numpy().view(np.uint32)) == [i if i != 2 else ic.PEER_NONE for i in range(n)]
    assert list(remote.cpu().numpy().view(np.uint32)) == [int(sid_b[i]) if i != 2 else 0 for i in range(n)]
    pend = pending.cpu().numpy()
    zero = np.frombuffer(ic.ZERO_PENDING, np.uint8)
    assert all((pend[i] == zero).all() for i in live)
    assert pend[2, 96:104].tobytes() == (1).to_bytes(4, "little") + int(sid_a[2]).to_bytes(4, "little")  # still waiting
    sa, sb = aead.Sessions(engine, 16), aead.Sessions(engine, 16)
    for i in live:
        assert ka[i, :32].tobytes() == kb[i, 32:].tobytes() and ka[i, 32:].tobytes() == kb[i, :32].tobytes(), i
        assert ka[i, :32].any() and ka[i, 32:].any() and ka[i, :32].tobytes() != ka[i, 32:].tobytes()
        sa.insert(int(sid_a[i]), int(sid_b[i]), ka[i, :32].tobytes(), ka[i, 32:].tobytes())
        sb.insert(int(sid_b[i]), int(sid_a[i]), kb[i, :32].tobytes(), kb[i, 32:].tobytes())
    for src, dst, ids in ((sa, sb, sid_a), (sb, sa, sid_b)):
        fdesc = np.array([(64 * j, 32, 0) for j in range(len(live))], DESC_DTYPE)
        frames = rng.integers(0, 256, 64 * len(live), dtype=np.uint8)
        plain = frames.copy()
        stt, _ = src.send_batch([src.lookup(int(ids[i])) for i in live], fdesc, frames)
        assert (stt == ic.OK).all()
        fdesc["len"] = 64
        stt, _ = dst.recv_batch(fdesc, frames)
        assert list(stt) == [ic.OK] * len(live)
        for j in range(len(live)):
            assert np.array_equal(frames[64 * j + 16:64 * j + 48], plain[64 * j + 16:64 * j + 48])


# ---------------------------------------------------------- recorded vectors
def _one_handshake(engine, sk_i, sk_r, psk, esk_i, esk_r, ts, sid_i, sid_r):
    """one handshake through all four calls: (the initiation, the response, A's key row, B's key row)."""
    pk_i, pk_r = hc.pubkey(sk_i), hc.pubkey(sk_r)
    peers_i, peers_r = hc.peer_rows([(pk_r, psk, hc.mac1_key(pk_r))]), hc.peer_rows([(pk_i, psk, hc.mac1_key(pk_i))])
    b = lambda x: _dev(np.frombuffer(x, np.uint8))  # noqa: E731
    msgs, pending = torch.zeros((1, 160), dtype=torch.uint8, device="cuda"), _fill((1, 128))
    st = [_fill((1,)) for _ in range(4)]
    d_pi, d_pr = _dev(peers_i), _dev(peers_r)
    engine.handshake_initiate_dev(b(sk_i + pk_i), d_pi, _dev(np.zeros(1, np.uint32)), None, b(esk_i), b(ts),
                                  _dev(np.array([sid_i], np.uint32)), None, None, msgs, pending, st[0])
    results, responses = _fill((1, 128)), _fill((1, 96))
    keys_r, keys_i = _fill((1, 64)), _fill((1, 64))
    engine.handshake_init_dev(b(sk_r + pk_r), d_pr, _dev(aead.peer_table(peers_r)),
                              _dev(np.array([(0, 148, 0)], DESC_DTYPE).view(np.uint8)), st[0], msgs, results, st[1])
    engine.handshake_resp_dev(d_pr, results, st[1], b(esk_r), _dev(np.array([sid_r], np.uint32)), None, None, responses,
                              keys_r, st[2])
    pidx, remote, claim = _fill((1,), torch.int32), _fill((1,), torch.int32), _fill((1,), torch.int32)
    engine.handshake_finish_dev(b(sk_i + pk_i), d_pi, _dev(aead.pending_table(np.array([sid_i], np.uint32))), pending,
                                _dev(np.array([(0, 92, 0)], DESC_DTYPE).view(np.uint8)), st[2], responses, keys_i, pidx,
                                remote, claim, st[3])
    torch.cuda.synchronize()
    assert [int(t.item()) for t in st] == [ic.OK] * 4
    assert int(remote.cpu().numpy().view(np.uint32)[0]) == sid_r and pidx.item() == 0
    return (msgs.cpu().numpy().tobytes()[:148], responses.cpu().numpy().tobytes()[:92],
            keys_i.cpu().numpy().tobytes(), keys_r.cpu().numpy().tobytes())


def test_recorded_handshakes_through_both_ends(engine):
    """the crypto crate's test `handshake` (seed 3) through the GPU on both sides gives its empty tag, K1 and
    K2; the core crate's test `snapshot` (seed 1), with the initiator's recovered ephemeral key, gives the
    recorded initiation and response byte for byte."""
    g = load_golden("handshake_full.json")["handshake"]
    init, resp, ki, kr = _one_handshake(engine, *(bytes.fromhex(g[k]) for k in (
        "static_private_i", "static_private_r", "preshared_key", "esk_i", "esk_r", "timestamp")), 0x11, 0x22)
    assert resp[44:60].hex() == g["empty_tag"]
    assert ki.hex() == g["transport_k1"] + g["transport_k2"] and kr.hex() == g["transport_k2"] + g["transport_k1"]
    s = load_golden("handshake_initiator.json").get("snapshot_initiation")
    if s is None:
        return  # the generator could not recover the ephemeral key: no recorded bytes to compare with
    full = load_golden("handshake_full.json")["snapshot"]
    init, resp, ki, kr = _one_handshake(engine, bytes.fromhex(s["static_private_i"]), bytes.fromhex(s["static_private_r"]),
                                        bytes.fromhex(full["preshared_key"]), bytes.fromhex(s["esk_i"]),
                                        bytes.fromhex(full["esk_r"]), bytes.fromhex(s["timestamp"]), s["sender"],
                                        full["session_id"])
    assert init.hex() == s["initiation"] and resp.hex() == full["response"]
    assert ki.hex() == full["recv_key"] + full["send_key"] and kr.hex() == full["send_key"] + full["recv_key"]


# ------------------------------------------------------------------ refusals
def test_initiator_argument_refusals(engine, initiate_world, finish_world):
    """null pointers, misaligned arrays, a pend_cap that is no power of two, n = 2^32, cookies without
    has_cookie: RG_EINVAL with the call named, nothing touched."""
    ini, _, b = initiate_world
    f = finish_world
    L, h = engine.library, engine.handle
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    n = 4
    own, peers = _dev(ini.own), _dev(b["peers"])
    pidx, esk, ts, sids = _dev(b["peer_idx"][:n + 1]), _dev(b["esk"][:n + 1]), _dev(b["ts"][:n + 1]), _dev(b["sids"][:n + 1])
    cookies, has = _dev(b["cookies"][:n + 1]), _dev(b["has_cookie"][:n])
    msgs, pend, status = _fill((n + 1, 160)), _fill((n + 1, 128)), _fill((n,))

    def initiate(own=p(own), peers=p(peers), pidx=p(pidx), esk_p=p(esk), ts_p=p(ts), sid=p(sids), ck=None, hc_=None,
                 out=p(msgs), pe=p(pend), st=p(status), n=n):
        return L.rg_handshake_initiate_batch_dev(h, own, peers, 6, pidx, None, esk_p, ts_p, sid, ck, hc_, n, out, pe, st, s)

    assert initiate(n=0) == 0
    for bad in (dict(own=None), dict(peers=None), dict(pidx=None), dict(esk_p=None), dict(ts_p=None), dict(sid=None),
                dict(out=None), dict(pe=None), dict(st=None), dict(ck=p(cookies)), dict(own=p(own, 8)),
                dict(peers=p(peers, 8)), dict(out=p(msgs, 8)), dict(pe=p(pend, 8)), dict(pidx=p(pidx, 2)),
                dict(esk_p=p(esk, 2)), dict(ts_p=p(ts, 1)), dict(sid=p(sids, 2)), dict(ck=p(cookies, 1), hc_=p(has)),
                dict(n=1 << 32)):
        assert initiate(**bad) == -1, bad
        assert b"handshake initiate" in L.rg_last_error(), bad
    npend, cap = len(f.rows), len(f.table)
    d_pending, (keys, pix, remote, claim, st) = f.pending_dev(), f.outputs()

    def finish(own=p(f.d_own), peers=p(f.d_peers), table=p(f.d_table), cap=cap, pe=p(d_pending), desc=p(f.d_desc),
               buf=p(f.d_buf), tk=p(keys), pi=p(pix), ro=p(remote), cl=p(claim), st_=p(st), n=n):
        return L.rg_handshake_finish_batch_dev(h, own, peers, 5, table, cap, pe, npend, desc, None, n, buf, len(f.buf),
                                               tk, pi, ro, cl, st_, s)

    assert finish(n=0) == 0
    for bad in (dict(own=None), dict(peers=None), dict(table=None), dict(pe=None), dict(desc=None), dict(buf=None),
                dict(tk=None), dict(pi=None), dict(ro=None), dict(cl=None), dict(st_=None), dict(own=p(f.d_own, 8)),
                dict(peers=p(f.d_peers, 4)), dict(pe=p(d_pending, 8)), dict(desc=p(f.d_desc, 8)), dict(tk=p(keys, 8)),
                dict(table=p(f.d_table, 2)), dict(pi=p(pix, 2)), dict(ro=p(remote, 1)), dict(cl=p(claim, 2)),
                dict(cap=cap - 1), dict(cap=0), dict(cap=24), dict(n=1 << 32)):
        assert finish(**bad) == -1, bad
        assert b"handshake finish" in L.rg_last_error(), bad
    torch.cuda.synchronize()
    for t in (msgs, pend, status, keys, st):
        assert (t.cpu().numpy() == FILL).all()
    for t in (pix, remote, claim):  # not even the claim workspace's memset was enqueued
        assert (t.cpu().numpy().view(np.uint32) == 0xA5A5A5A5).all()
    assert np.array_equal(d_pending.cpu().numpy()[:npend], f.rows)
