"""The device-resident peer handshake state on the GPU (rg_peer_ts_batch_dev, rg_peer_cookie_consume_batch_dev,
rg_peer_cookies_batch_dev, rg_peer_mac1_batch_dev) against the in-order Python model (tests/peerstate_cases.py)
and inside the two chains they were made for.  Every output array and every byte of the state table is compared;
nothing is approximate."""
import ctypes

import numpy as np
import pytest

import handshake_cases as hc
import peerstate_cases as pc
from oracle import oracle
from rustyguard_amd import aead
from rustyguard_amd.workloads import DESC_DTYPE

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL = 0xA5
GUARD = 0xA5A5A5A5


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _fill(shape, dtype=torch.uint8):
    if dtype == torch.uint8:
        return torch.full(shape, FILL, dtype=dtype, device="cuda")
    return torch.full(shape, GUARD - (1 << 32), dtype=torch.int32, device="cuda")  # the same bytes


def _rows(t, n):
    return [r.tobytes() for r in t.cpu().numpy()[:n]]


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _same(name, got, want):
    assert len(got) == len(want), name
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (name, len(bad), bad[:8], [(got[i], want[i]) for i in bad[:2]])


def _state_dev(state):
    """the table with one guard row behind it"""
    t = _fill((len(state) + 1, pc.ROW))
    t[:len(state)] = _dev(pc.rows_array(state, pc.ROW))
    return t


def _state_read(t, nrows):
    a = t.cpu().numpy()
    assert (a[nrows:] == FILL).all()
    return [r.tobytes() for r in a[:nrows]]


# --------------------------------------------------------------- timestamps
class TsCall:
    """One rg_peer_ts_batch_dev geometry on the device: the table (npeers of its rows are the call's), the
    in-place arrays with a guard row each, the workspace."""

    def __init__(self, engine, state, n, npeers=None):
        self.engine, self.n, self.nstate = engine, n, len(state)
        self.npeers = len(state) if npeers is None else npeers
        self.state = _state_dev(state)
        self.res, self.st, self.po = _fill((n + 1, 128)), _fill((n + 1,)), _fill((n + 1,), torch.int32)
        self.ws = engine.peer_ts_workspace(n, self.npeers)

    def load(self, results, status):
        n = self.n
        self.res[:n] = _dev(pc.rows_array(results, 128))
        self.st[:n] = _dev(np.array(status, np.uint8))
        self.po.fill_(GUARD - (1 << 32))

    def run(self, stream=None):
        n = self.n
        self.engine.peer_ts_dev(self.state[:self.npeers], self.res[:n], self.st[:n], self.po[:n], workspace=self.ws,
                                stream=stream)

    def read(self):
        torch.cuda.synchronize()
        n = self.n
        res, st, po = self.res.cpu().numpy(), self.st.cpu().numpy(), _u32(self.po)
        assert (res[n:] == FILL).all() and st[n] == FILL and po[n] == GUARD
        return (_state_read(self.state, self.nstate), [r.tobytes() for r in res[:n]], [int(x) for x in st[:n]],
                [int(x) for x in po[:n]])

    def check(self, want):
        for name, g, w in zip(("state", "results", "status", "peers_out"), self.read(), want):
            _same(name, g, w)


def _ts_once(engine, state, results, status, npeers=None):
    c = TsCall(engine, state, len(results), npeers)
    c.load(results, status)
    c.run()
    want = pc.ts_loop(state, results, status, npeers)
    c.check(want)
    return want


@pytest.mark.parametrize("name", [e[0] for e in pc.EDGE_TS])
def test_ts_edge_rows(engine, name):
    """equal to latest passes; timestamps that differ in byte 0 or byte 11 alone; pairs whose order flips under a
    little-endian word comparison; n <= 16"""
    state, results, status, verdicts = pc.edge_ts_case(name)
    assert len(results) <= 16
    want = _ts_once(engine, state, results, status)
    assert want[2] == verdicts


def _trend_batch(rng, n, peer_of, npeers, bad=0.1, far=()):
    """rows whose timestamps rise slowly with the index under noise of a few steps, so that ties, accepted and
    rejected rows all occur and a row's verdict depends on rows far ahead of it"""
    results, status = [], []
    for i in range(n):
        sec = (1 << 62) + 1_700_000_000 + i // 16 + int(rng.integers(-3, 4))
        ts = sec.to_bytes(8, "big") + [0, 1, 1 << 24][int(rng.integers(0, 3))].to_bytes(4, "big")
        p, st = peer_of(i), pc.OK
        if i in far:
            p = [npeers, npeers + 9, pc.PEER_NONE][i % 3]
        elif rng.random() < bad:
            st = [pc.DECRYPT_ERR, pc.INVALID, pc.REJECTED, pc.UNALIGNED, 8][int(rng.integers(0, 5))]
        results.append(pc.result_row(ts, p, 1 + i % 250) if st == pc.OK else pc.ZERO_RESULT)
        status.append(st)
    return results, status


def test_ts_beyond_one_tile(engine):
    """n = 2 * 2048 + 77 over 3 interleaved peers of a 5-row table: peer 0 owns more than 2048 rows, so its group
    spans a tile boundary and the carry runs; peer 2 meets a far-future timestamp early and loses every later
    row, in another tile; about 10 % of the rows are not OK and a few name no peer row; the table's other rows
    keep every byte."""
    rng = np.random.default_rng(41)
    n, npeers = 2 * 2048 + 77, 3
    deal = rng.choice(3, n, p=[0.6, 0.2, 0.2])
    results, status = _trend_batch(rng, n, lambda i: int(deal[i]), npeers, far={7, 2100, 4100, 4172})
    at = next(i for i in range(40, n) if deal[i] == 2)
    results[at], status[at] = pc.result_row(b"\x7f" + bytes(11), 2, 0x33), pc.OK
    rb = lambda k: bytes(rng.integers(0, 256, k, dtype=np.uint8))  # noqa: E731
    first = results[next(i for i in range(n) if status[i] == pc.OK and deal[i] == 0 and i not in (7,))][96:108]
    state = [pc.state_row(first, cookie=rb(16), mac1=rb(16), pad=rb(16)), pc.state_row(), pc.state_row(mac1=rb(16))]
    state += [pc.state_row(rb(12), cookie=rb(16), mac1=rb(16), pad=rb(16)), pc.state_row(rb(12))]
    want = _ts_once(engine, state, results, status, npeers)
    ok0 = [i for i in range(n) if deal[i] == 0 and status[i] == pc.OK and i not in (7, 2100, 4100, 4172)]
    assert len(ok0) > 2048
    st = want[2]
    assert sum(st[i] == pc.REJECTED for i in ok0) > 200 and sum(st[i] == pc.OK for i in ok0) > 200
    later2 = [i for i in range(at + 1, n) if deal[i] == 2 and status[i] == pc.OK and i not in (2100, 4100, 4172)]
    assert len(later2) > 500 and all(st[i] == pc.REJECTED for i in later2)
    assert [st[i] for i in (7, 2100, 4100, 4172)] == [pc.INVALID] * 4
    assert want[0][3:] == state[3:] and want[0][2][:12] == b"\x7f" + bytes(11)


def test_ts_two_radix_passes(engine):
    """300 peers (two 8-bit passes over the peer index), n = 2049 (two tiles)"""
    rng = np.random.default_rng(42)
    npeers, n = 300, 2049
    results, status = pc.random_ts_batch(rng, n, npeers, nts=5)
    pool = sorted({r[96:108] for r, s in zip(results, status) if s == pc.OK})
    state = [pc.state_row(pool[int(rng.integers(0, len(pool)))] if p % 3 else bytes(12), mac1=bytes([p & 255]) * 16)
             for p in range(npeers)]
    want = _ts_once(engine, state, results, status)
    turned = [b for a, b in zip(status, want[2]) if a == pc.OK and b != pc.OK]
    assert turned.count(pc.REJECTED) > 300 and want[2].count(pc.OK) > 300 and turned.count(pc.INVALID) == 3
    assert len({p for p in want[3] if p != pc.PEER_NONE}) > 256


def test_ts_state_carried_between_calls_and_graph_replays(engine):
    """two calls on one table, then the same call captured into a graph and replayed twice: the table carries
    latest_ts from call to call, so the model is applied as often"""
    rng = np.random.default_rng(43)
    n, npeers = 700, 4
    state = [pc.state_row(mac1=bytes([p]) * 16) for p in range(npeers)]
    batches = [_trend_batch(rng, n, lambda i: i % npeers, npeers) for _ in range(2)]
    batches[1] = (batches[1][0][::-1], batches[1][1][::-1])  # mostly falling: many rejections
    c = TsCall(engine, state, n)
    model = state
    for results, status in batches:
        c.load(results, status)
        c.run()
        want = pc.ts_loop(model, results, status)
        c.check(want)
        model = want[0]
    assert model != state
    # captured: the inputs are put back before every replay, the table is not
    results, status = batches[0]
    d_res, d_st = _dev(pc.rows_array(results, 128)), _dev(np.array(status, np.uint8))
    c.state[:npeers] = _dev(pc.rows_array(state, pc.ROW))
    c.load(results, status)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        c.run(stream=s)
    torch.cuda.synchronize()
    c.state[:npeers] = _dev(pc.rows_array(state, pc.ROW))  # whatever the capture did or did not run
    model = state
    for _ in range(2):
        c.res[:n], c.st[:n] = d_res, d_st
        c.po.fill_(GUARD - (1 << 32))
        g.replay()
        want = pc.ts_loop(model, results, status)
        c.check(want)
        model = want[0]
    assert want[2].count(pc.REJECTED) > pc.ts_loop(state, results, status)[2].count(pc.REJECTED)


# ------------------------------------------------------------------ consume
CONSUME_COUNTS = [("valid", 150), ("tag_flipped", 20), ("ct_flipped", 20), ("nonce_flipped", 20), ("stale_mac1", 15),
                  ("unknown_receiver", 15), ("far_peer", 10), ("type4", 10), ("len63", 5), ("len65", 5),
                  ("offset8", 10), ("gated", 10), ("key_skip", 6)]
CONSUME_STATUS = {"valid": pc.OK, "tag_flipped": pc.DECRYPT_ERR, "ct_flipped": pc.DECRYPT_ERR,
                  "nonce_flipped": pc.DECRYPT_ERR, "stale_mac1": pc.DECRYPT_ERR, "unknown_receiver": pc.REJECTED,
                  "far_peer": pc.INVALID, "type4": pc.INVALID, "len63": pc.INVALID, "len65": pc.INVALID,
                  "offset8": pc.UNALIGNED, "gated": pc.REJECTED, "key_skip": pc.REJECTED, "past_buf": pc.INVALID}


class ConsumeWorld:
    """5 peers, four session ids each and one id whose table row names no peer; 300 messages: the mixed kinds
    dealt by a seeded permutation over peers 0-2 (failures over all five), then by hand peer 4's two valid
    messages with different cookies at indices 10 and 290 (two workgroups) and peer 3's valid message at 20
    with a forged one at 295."""

    def __init__(self, seed=77):
        rng = self.rng = np.random.default_rng(seed)
        rb = self.rb = lambda k: bytes(rng.integers(0, 256, k, dtype=np.uint8))
        self.npeers = 5
        self.keys = [pc.cookie_key(rb(32)) for _ in range(self.npeers)]
        self.state = [pc.state_row(rb(12), cookie=rb(16) if p % 2 else None, mac1=rb(16), pad=rb(16))
                      for p in range(self.npeers)]
        ids = (rng.permutation(1 << 20)[:21].astype(np.uint32) + 0x4000_0000)
        self.ids = [int(x) for x in ids]
        self.id_peer = [i % self.npeers for i in range(20)] + [9]
        self.table = dict(zip(self.ids, self.id_peer))
        kinds = [k for k, c in CONSUME_COUNTS for _ in range(c)]
        kinds = [kinds[i] for i in rng.permutation(len(kinds))]
        plan = [(k, int(rng.integers(0, 3 if k == "valid" else 5))) for k in kinds]
        for at, item in ((10, ("valid", 4)), (20, ("valid", 3)), (290, ("valid", 4)), (295, ("tag_flipped", 3))):
            plan.insert(at, item)
        plan += [("past_buf", 0)] * 4
        assert len(plan) == 304
        self.plan = plan
        self.build()

    def message(self, kind, p, i):
        rb = self.rb
        rid = self.ids[p + 5 * (i % 4)]
        mac1 = self.state[p][32:48]
        if kind == "stale_mac1":
            mac1 = rb(16)
        if kind == "unknown_receiver":
            rid = 0x0BAD_0000 + i
        if kind == "far_peer":
            rid = self.ids[20]
        m = bytearray(pc.cookie_message(rid, rb(24), self.keys[p], mac1, rb(16)))
        lo = {"tag_flipped": 48, "ct_flipped": 32, "nonce_flipped": 8}.get(kind)
        if lo is not None:
            m[lo + int(self.rng.integers(0, 24 if lo == 8 else 16))] ^= 1 << int(self.rng.integers(0, 8))
        if kind == "type4":
            m[0:4] = (4).to_bytes(4, "little")
        return bytes(m)

    def build(self):
        rng, n = self.rng, len(self.plan)
        gaps = rng.integers(0, 3, n) * 16
        off, pos = [], 0
        for i in range(n):
            off.append(pos)
            pos += 64 + int(gaps[i])
        self.buf = rng.integers(0, 256, pos, dtype=np.uint8)
        self.desc, self.gate = np.zeros(n, DESC_DTYPE), np.zeros(n, np.uint8)
        self.msgs, self.flags = [], []
        for i, (kind, p) in enumerate(self.plan):
            m = self.message(kind, p, i)
            o, ln, key, kw = off[i], 64, int(rng.integers(0, 1000)), {}
            if kind in ("len63", "len65"):
                ln = int(kind[3:])
                kw = dict(length=ln)
            elif kind == "offset8":
                o, kw = o + 8, dict(aligned=False)
            elif kind == "past_buf":
                o, kw = pos - 48, dict(in_buf=False)  # the last 16-byte boundary from which 64 bytes overrun
            elif kind == "gated":
                self.gate[i], kw = [pc.REJECTED, 7, pc.INVALID, 6][i % 4], dict(gated=True)
            elif kind == "key_skip":
                key, kw = pc.KEY_SKIP, dict(key_skip=True)
            self.buf[off[i]:off[i] + 64] = np.frombuffer(m, np.uint8)
            self.desc[i] = (o, ln, key)
            self.msgs.append(m)
            self.flags.append(kw)


def test_consume_mixed_batch_vs_model(engine):
    """every status, every cookies_out row and every byte of the table against the in-order loop: of two valid
    messages of one peer the higher index stays, a forged message behind a valid one changes nothing; buf is
    never written"""
    w = ConsumeWorld()
    n, npeers = len(w.plan), w.npeers
    want_state, want_st, want_ck = pc.consume_loop(w.state, w.keys, w.table, w.msgs, w.flags)
    for (k, _), s in zip(w.plan, want_st):  # the model agrees with the header's table
        assert s == CONSUME_STATUS[k], k
    assert want_state[4][16:32] == want_ck[290] != want_ck[10] and want_ck[10] != bytes(16)
    assert want_state[3][16:32] == want_ck[20] and want_st[295] == pc.DECRYPT_ERR
    assert all(want_state[p][12:16] == b"\x01\0\0\0" for p in range(npeers))
    d_state = _state_dev(w.state)
    d_keys = _dev(np.frombuffer(b"".join(w.keys), np.uint8))
    d_table = _dev(aead.rx_table(np.array(w.ids, np.uint32), np.array(w.id_peer, np.uint32)))
    d_desc, d_buf, d_gate = _dev(w.desc.view(np.uint8).reshape(-1, 16)), _dev(w.buf), _dev(w.gate)
    ck, claim, st = _fill((n + 1, 16)), _fill((npeers + 1,), torch.int32), _fill((n + 1,))
    engine.peer_cookie_consume_dev(d_state[:npeers], d_keys, d_table, d_desc, d_gate, d_buf, ck[:n], claim[:npeers],
                                   st[:n])
    torch.cuda.synchronize()
    assert (ck.cpu().numpy()[n:] == FILL).all() and st.cpu().numpy()[n] == FILL and _u32(claim)[npeers] == GUARD
    _same("status", [int(x) for x in st.cpu().numpy()[:n]], want_st)
    _same("cookies_out", _rows(ck, n), want_ck)
    _same("state", _state_read(d_state, npeers), want_state)
    assert np.array_equal(d_buf.cpu().numpy(), w.buf)
    assert _u32(claim)[4] == 291 and _u32(claim)[3] == 21
    # a peer without a valid message keeps its row byte for byte: the failures alone, on a fresh table
    fails = [i for i, (k, _) in enumerate(w.plan) if k != "valid"]
    d_state2 = _state_dev(w.state)
    m = len(fails)
    ck2, st2 = _fill((m + 1, 16)), _fill((m + 1,))
    engine.peer_cookie_consume_dev(d_state2[:npeers], d_keys, d_table, _dev(w.desc[fails].view(np.uint8).reshape(-1, 16)),
                                   _dev(w.gate[fails]), d_buf, ck2[:m], claim[:npeers], st2[:m])
    torch.cuda.synchronize()
    assert _state_read(d_state2, npeers) == w.state and (ck2.cpu().numpy()[:m] == 0).all()
    assert [int(x) for x in st2.cpu().numpy()[:m]] == [want_st[i] for i in fails]
    assert (_u32(claim)[:npeers] == 0).all()


# ---------------------------------------------------------- gather / record
def test_gather_and_record_vs_model(engine):
    """duplicates per peer, rows that were not sent, RG_PEER_NONE and rows past the table, over two workgroups;
    both (stride, mac1_offset) pairs of the handshake messages"""
    rng = np.random.default_rng(9)
    rb = lambda k: bytes(rng.integers(0, 256, k, dtype=np.uint8))  # noqa: E731
    npeers, n = 6, 300
    state = [pc.state_row(rb(12), cookie=rb(16) if p in (0, 2, 5) else None, mac1=rb(16), pad=rb(16))
             for p in range(npeers)]
    stale = bytearray(state[3])  # a cookie left behind a cleared has_cookie does not count
    stale[16:32] = rb(16)
    state[3] = bytes(stale)
    peer_idx = [int(x) for x in rng.choice([0, 1, 2, 3, 5, npeers, npeers + 3, pc.PEER_NONE], n)]  # peer 4: absent
    status = [int(x) for x in rng.choice([pc.OK, pc.OK, pc.OK, pc.REJECTED, pc.INVALID, 8], n)]
    d_state, d_pidx = _state_dev(state), _dev(np.array(peer_idx, np.uint32))
    ck, has = _fill((n + 1, 16)), _fill((n + 1,))
    engine.peer_cookies_dev(d_state[:npeers], d_pidx, ck[:n], has[:n])
    torch.cuda.synchronize()
    want_ck, want_has = pc.gather(state, peer_idx)
    assert (ck.cpu().numpy()[n:] == FILL).all() and has.cpu().numpy()[n] == FILL
    _same("cookies", _rows(ck, n), want_ck)
    _same("has_cookie", [int(x) for x in has.cpu().numpy()[:n]], want_has)
    assert _state_read(d_state, npeers) == state and 0 < sum(want_has) < n
    model = state
    for stride, at in ((160, 116), (96, 60)):
        msgs = rng.integers(0, 256, (n, stride), dtype=np.uint8)
        claim = _fill((npeers + 1,), torch.int32)
        engine.peer_mac1_dev(d_state[:npeers], d_pidx, _dev(np.array(status, np.uint8)), _dev(msgs), stride, at,
                             claim[:npeers])
        torch.cuda.synchronize()
        model = pc.record_loop(model, peer_idx, status, [m.tobytes() for m in msgs], at)
        _same("state", _state_read(d_state, npeers), model)
        assert _u32(claim)[npeers] == GUARD and _u32(claim)[4] == 0
        last = max(i for i in range(n) if peer_idx[i] == 0 and status[i] == pc.OK)
        assert _u32(claim)[0] == last + 1 and model[0][32:48] == msgs[last, at:at + 16].tobytes()
    assert model[4] == state[4] and all(a[:32] == b[:32] and a[48:] == b[48:] for a, b in zip(model, state))


# ------------------------------------------------------------ the loop closes
def test_cookie_loop_closes_gpu_to_gpu(engine):
    """64 handshakes of one initiator to a responder under load, one peer row each: cookies -> initiate -> mac1,
    the responder's filter answers every one with a cookie reply, consume opens them all under the recorded
    mac1 and stores BLAKE2s-128(secret, addr), cookies -> initiate again, and now the filter passes them all.
    One stream, no host step between the calls."""
    rng = np.random.default_rng(64)
    rb = lambda k: bytes(rng.integers(0, 256, k, dtype=np.uint8))  # noqa: E731
    n = 64
    sk_a, sk_b = rb(32), rb(32)
    pk_a, pk_b = hc.pubkey(sk_a), hc.pubkey(sk_b)
    peers_a = hc.peer_rows([(pk_b, rb(32), hc.mac1_key(pk_b)) for _ in range(n)])  # one tunnel per row, all to B
    secret = rb(32)
    ck = hc.mac1_key(pk_b) + pc.cookie_key(pk_b) + secret  # B's rg_cookie_keys
    addrs = [aead.encode_src_addr("198.51.100.%d" % i, 7000 + i) for i in range(n)]
    sids = rng.permutation(1 << 20)[:n].astype(np.uint32) + 0x0A00_0000
    desc = np.array([(160 * i, 148, 0) for i in range(n)], DESC_DTYPE)
    rdesc = np.array([(64 * i, 64, 0) for i in range(n)], DESC_DTYPE)
    state0 = [pc.state_row() for _ in range(n)]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_state = _state_dev(state0)
        a_own, a_peers = _dev(np.frombuffer(sk_a + pk_a, np.uint8)), _dev(peers_a)
        pidx, d_sids = _dev(np.arange(n, dtype=np.uint32)), _dev(sids)
        esk = [_dev(rng.integers(0, 256, (n, 32), dtype=np.uint8)) for _ in range(2)]
        ts = _dev(np.frombuffer(b"".join(hc.tai64n(1_900_000_000, i) for i in range(n)), np.uint8).reshape(n, 12))
        d_ck, d_addrs = _dev(np.frombuffer(ck, np.uint8)), _dev(np.frombuffer(b"".join(addrs), np.uint8).reshape(n, 24))
        d_over, d_nonces = _dev(np.ones(n, np.uint8)), _dev(rng.integers(0, 256, (n, 24), dtype=np.uint8))
        d_desc, d_rdesc = _dev(desc.view(np.uint8).reshape(-1, 16)), _dev(rdesc.view(np.uint8).reshape(-1, 16))
        d_ckeys = _dev(np.frombuffer(pc.cookie_key(pk_b) * n, np.uint8))
        d_table = _dev(aead.rx_table(sids, np.arange(n, dtype=np.uint32)))
        msgs = [torch.zeros((n, 160), dtype=torch.uint8, device="cuda") for _ in range(2)]
        pend = [_fill((n, 128)) for _ in range(2)]
        cookies = [_fill((n, 16)) for _ in range(2)]
        has = [_fill((n,)) for _ in range(2)]
        replies = [torch.zeros((n, 64), dtype=torch.uint8, device="cuda") for _ in range(2)]
        got_ck, claim = _fill((n, 16)), _fill((n,), torch.int32)
        st = [_fill((n,)) for _ in range(5)]
    s.synchronize()
    with torch.cuda.stream(s):
        engine.peer_cookies_dev(d_state[:n], pidx, cookies[0], has[0], stream=s)
        engine.handshake_initiate_dev(a_own, a_peers, pidx, None, esk[0], ts, d_sids, cookies[0], has[0], msgs[0],
                                      pend[0], st[0], stream=s)
        engine.peer_mac1_dev(d_state[:n], pidx, st[0], msgs[0], 160, 116, claim, stream=s)
        engine.cookie_reply_dev(d_ck, d_desc, d_addrs, d_over, d_nonces, msgs[0], replies[0], st[1], stream=s)
        engine.peer_cookie_consume_dev(d_state[:n], d_ckeys, d_table, d_rdesc, None, replies[0], got_ck, claim, st[2],
                                       stream=s)
        engine.peer_cookies_dev(d_state[:n], pidx, cookies[1], has[1], stream=s)
        engine.handshake_initiate_dev(a_own, a_peers, pidx, None, esk[1], ts, d_sids, cookies[1], has[1], msgs[1],
                                      pend[1], st[3], stream=s)
        engine.cookie_reply_dev(d_ck, d_desc, d_addrs, d_over, d_nonces, msgs[1], replies[1], st[4], stream=s)
    s.synchronize()
    assert (has[0].cpu().numpy() == 0).all() and (cookies[0].cpu().numpy() == 0).all()
    assert list(st[0].cpu().numpy()) == [pc.OK] * n and list(st[3].cpu().numpy()) == [pc.OK] * n
    assert list(st[1].cpu().numpy()) == [aead.PKT_COOKIE] * n
    assert list(st[2].cpu().numpy()) == [pc.OK] * n
    want_ck = [oracle.blake2s(a[:18], secret, 16) for a in addrs]
    m0, m1 = msgs[0].cpu().numpy(), msgs[1].cpu().numpy()
    assert (m0[:, 132:148] == 0).all()
    want_state = [pc.state_row(cookie=c, mac1=m0[i, 116:132].tobytes()) for i, c in enumerate(want_ck)]
    _same("state", _state_read(d_state, n), want_state)
    _same("cookies_out", _rows(got_ck, n), want_ck)
    _same("gathered", _rows(cookies[1], n), want_ck)
    assert (has[1].cpu().numpy() == 1).all()
    assert all(m1[i, 132:148].tobytes() == oracle.blake2s(m1[i, :132].tobytes(), want_ck[i], 16) for i in range(n))
    assert list(st[4].cpu().numpy()) == [pc.OK] * n  # mac2 under the stored cookie: the filter lets them through
    assert (replies[1].cpu().numpy() == 0).all()


# ------------------------------------------------------------ responder chain
def test_responder_chain_on_one_stream(engine):
    """filter -> init -> ts -> cookies -> resp -> mac1 on one stream against the existing calls stitched together
    on the host with ts_loop, gather and record_loop in between: 44 initiations over 4 peers, one with a broken
    mac1, one of an unknown initiator, and for peer 2 a timestamp of 5 followed by one of 3, which must come out
    RG_PKT_REJECTED with a zero response row."""
    r = hc.Responder(2029, npeers=4, neph=6, nunknown=1)
    rng = r.rng
    rb = lambda k: bytes(rng.integers(0, 256, k, dtype=np.uint8))  # noqa: E731
    n, npeers = 44, 4
    senders = rng.permutation(1 << 20)[:n].astype(np.uint32) + 0x0C00_0000
    # peer 2 (a new peer: a zero row) counts in small numbers: ... 4, 5, 3, 5 ...
    small = {2: 1, 6: 1, 10: 2, 14: 2, 18: 4, 22: 5, 26: 3, 30: 5, 34: 6, 38: 6, 42: 2}
    five, three = 22, 26
    msgs = []
    for i in range(n):
        p = i % npeers
        ts = hc.tai64n(1_700_000_000 + (i // 8), 0)  # runs of equal timestamps per peer
        if i in (13, 31):
            ts = hc.tai64n(1_600_000_000, i)  # older than what the peer sent before
        if p == 2:
            ts = bytes(11) + bytes([small[i]])
        sk = r.sk_unknown[0] if i == 9 else r.sk_i[p]
        m = bytearray(hc.make_initiation(sk, r.pk_r, r.esk_i[i % 6], ts, int(senders[i]))[0])
        if i == 17:
            m[120] ^= 1  # mac1 broken: drops out at the filter
        msgs.append(bytes(m))
    # the table: peer 2 is new (Peer::new), peers 1 and 3 hold a cookie (their responses carry a mac2), peer 0
    # has seen a timestamp newer than its first two of this batch
    state = [pc.state_row(hc.tai64n(1_700_000_001, 0), mac1=rb(16)), pc.state_row(cookie=rb(16)), pc.state_row(),
             pc.state_row(hc.tai64n(1_500_000_000, 0), cookie=rb(16), mac1=rb(16), pad=rb(16))]
    buf = np.zeros(160 * n, np.uint8)
    for i, m in enumerate(msgs):
        buf[160 * i:160 * i + 148] = np.frombuffer(m, np.uint8)
    desc = np.array([(160 * i, 148, 0) for i in range(n)], DESC_DTYPE)
    ck = hc.mac1_key(r.pk_r) + rb(64)
    addrs = np.frombuffer(b"".join(aead.encode_src_addr("192.0.2.%d" % i, 4000 + i) for i in range(n)), np.uint8)
    rows_b = hc.peer_rows(r.peers)
    d_own, d_peers, d_table = _dev(r.own), _dev(rows_b), _dev(aead.peer_table(rows_b))
    d_desc, d_buf = _dev(desc.view(np.uint8).reshape(-1, 16)), _dev(buf)
    d_ck, d_addrs = _dev(np.frombuffer(ck, np.uint8)), _dev(addrs.reshape(n, 24))
    d_over, d_nonces = _dev(np.zeros(n, np.uint8)), _dev(rng.integers(0, 256, (n, 24), dtype=np.uint8))
    d_esk = _dev(rng.integers(0, 256, (n, 32), dtype=np.uint8))
    d_sid = _dev(np.arange(n, dtype=np.uint32) * 7 + 0x0D00)
    replies = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")

    def outputs():
        return dict(results=_fill((n, 128)), responses=torch.zeros((n, 96), dtype=torch.uint8, device="cuda"),
                    keys=torch.zeros((n, 64), dtype=torch.uint8, device="cuda"), st_f=_fill((n,)), st_i=_fill((n,)),
                    st_r=_fill((n,)))

    # the chain
    c = outputs()
    d_state = _state_dev(state)
    po, cookies, has, claim = _fill((n,), torch.int32), _fill((n, 16)), _fill((n,)), _fill((npeers,), torch.int32)
    ws = engine.peer_ts_workspace(n, npeers)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        engine.cookie_reply_dev(d_ck, d_desc, d_addrs, d_over, d_nonces, d_buf, replies, c["st_f"], stream=s)
        engine.handshake_init_dev(d_own, d_peers, d_table, d_desc, c["st_f"], d_buf, c["results"], c["st_i"], stream=s)
        engine.peer_ts_dev(d_state[:npeers], c["results"], c["st_i"], po, workspace=ws, stream=s)
        engine.peer_cookies_dev(d_state[:npeers], po, cookies, has, stream=s)
        engine.handshake_resp_dev(d_peers, c["results"], c["st_i"], d_esk, d_sid, cookies, has, c["responses"],
                                  c["keys"], c["st_r"], stream=s)
        engine.peer_mac1_dev(d_state[:npeers], po, c["st_r"], c["responses"], 96, 60, claim, stream=s)
    s.synchronize()
    # the same with the host in between
    h = outputs()
    engine.cookie_reply_dev(d_ck, d_desc, d_addrs, d_over, d_nonces, d_buf, replies, h["st_f"])
    engine.handshake_init_dev(d_own, d_peers, d_table, d_desc, h["st_f"], d_buf, h["results"], h["st_i"])
    torch.cuda.synchronize()
    res0, st0 = _rows(h["results"], n), [int(x) for x in h["st_i"].cpu().numpy()]
    want_state, res1, st1, want_po = pc.ts_loop(state, res0, st0)
    want_ck, want_has = pc.gather(want_state, want_po)
    h["results"][:] = _dev(pc.rows_array(res1, 128))
    h["st_i"][:] = _dev(np.array(st1, np.uint8))
    engine.handshake_resp_dev(d_peers, h["results"], h["st_i"], d_esk, d_sid, _dev(pc.rows_array(want_ck, 16)),
                              _dev(np.array(want_has, np.uint8)), h["responses"], h["keys"], h["st_r"])
    torch.cuda.synchronize()
    st_r = [int(x) for x in h["st_r"].cpu().numpy()]
    want_state = pc.record_loop(want_state, want_po, st_r, _rows(h["responses"], n), 60)
    # what the host path saw, so that the comparison below means something
    assert st0[17] == pc.REJECTED and st0[9] == pc.REJECTED and st0.count(pc.OK) == n - 2
    assert st1[five] == pc.OK and st1[three] == pc.REJECTED and st1[30] == pc.OK  # 5, 3, then 5 again
    assert [i for i in range(n) if st1[i] != pc.OK] == [0, 4, 9, 13, 17, 26, 31, 42]
    assert st_r == st1
    resp_h = h["responses"].cpu().numpy()
    assert (resp_h[three] == 0).all() and resp_h[five].any()
    assert all(resp_h[i, 76:92].any() == (want_po[i] in (1, 3)) for i in range(n))  # mac2 where the peer has a cookie
    assert want_state[2][:12] == bytes(11) + b"\x06" and want_state[2][32:48] != bytes(16)
    for name in ("st_f", "st_i", "st_r", "results", "responses", "keys"):
        assert torch.equal(c[name], h[name]), name
    _same("peers_out", [int(x) for x in _u32(po)], want_po)
    _same("cookies", _rows(cookies, n), want_ck)
    _same("has_cookie", [int(x) for x in has.cpu().numpy()], want_has)
    _same("state", _state_read(d_state, npeers), want_state)
    assert c["st_r"].cpu().numpy()[three] == pc.REJECTED and (c["responses"].cpu().numpy()[three] == 0).all()


# ------------------------------------------------------------------ refusals
def test_peerstate_argument_refusals(engine):
    """n == 0 is RG_OK; a null required pointer, n = 2^32, a misaligned array, a short workspace, a sess_cap that
    is no power of two and a mac1 field that does not fit its row are RG_EINVAL with the call named, and nothing
    is enqueued: every array keeps its fill, the claim workspaces included."""
    L, h = engine.library, engine.handle
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    n, npeers = 8, 3
    state, res, st, po = _fill((npeers + 1, 64)), _fill((n + 1, 128)), _fill((n,)), _fill((n + 1,), torch.int32)
    need = int(L.rg_peer_ts_workspace_size(n, npeers))
    ws = _fill((need + 16,))

    def ts(state_=p(state), res_=p(res), st_=p(st), po_=p(po), n_=n, ws_=p(ws), wl=need):
        return L.rg_peer_ts_batch_dev(h, state_, npeers, res_, st_, po_, n_, ws_, wl, s)

    assert ts(n_=0) == 0
    for bad in (dict(state_=None), dict(res_=None), dict(st_=None), dict(po_=None), dict(ws_=None),
                dict(state_=p(state, 8)), dict(res_=p(res, 8)), dict(po_=p(po, 2)), dict(ws_=p(ws, 8)),
                dict(wl=need - 1), dict(wl=0), dict(n_=1 << 32)):
        assert ts(**bad) == -1, bad
        assert b"peer ts" in L.rg_last_error(), bad
    keys, table, desc = _fill((npeers, 32)), _fill((8, 8)), _fill((n + 1, 16))
    buf, ck, claim = _fill((64 * n,)), _fill((n + 1, 16)), _fill((npeers + 1,), torch.int32)

    def consume(state_=p(state), keys_=p(keys), table_=p(table), cap=8, desc_=p(desc), buf_=p(buf), ck_=p(ck),
                claim_=p(claim), st_=p(st), n_=n):
        return L.rg_peer_cookie_consume_batch_dev(h, state_, npeers, keys_, table_, cap, desc_, None, n_, buf_, 64 * n,
                                                  ck_, claim_, st_, s)

    assert consume(n_=0) == 0
    for bad in (dict(state_=None), dict(keys_=None), dict(table_=None), dict(desc_=None), dict(buf_=None),
                dict(ck_=None), dict(claim_=None), dict(st_=None), dict(state_=p(state, 8)), dict(keys_=p(keys, 8)),
                dict(desc_=p(desc, 8)), dict(table_=p(table, 2)), dict(ck_=p(ck, 2)), dict(claim_=p(claim, 2)),
                dict(cap=0), dict(cap=6), dict(cap=7), dict(n_=1 << 32)):
        assert consume(**bad) == -1, bad
        assert b"peer cookie consume" in L.rg_last_error(), bad
    pidx, has = _fill((n + 1,), torch.int32), _fill((n,))

    def cookies(state_=p(state), pidx_=p(pidx), ck_=p(ck), has_=p(has), n_=n):
        return L.rg_peer_cookies_batch_dev(h, state_, npeers, pidx_, n_, ck_, has_, s)

    assert cookies(n_=0) == 0
    for bad in (dict(state_=None), dict(pidx_=None), dict(ck_=None), dict(has_=None), dict(state_=p(state, 8)),
                dict(pidx_=p(pidx, 2)), dict(ck_=p(ck, 1)), dict(n_=1 << 32)):
        assert cookies(**bad) == -1, bad
        assert b"peer cookies" in L.rg_last_error(), bad
    msgs = _fill((n, 160))

    def mac1(state_=p(state), pidx_=p(pidx), st_=p(st), msgs_=p(msgs), stride=160, at=116, claim_=p(claim), n_=n):
        return L.rg_peer_mac1_batch_dev(h, state_, npeers, pidx_, st_, msgs_, stride, at, n_, claim_, s)

    assert mac1(n_=0) == 0
    for bad in (dict(state_=None), dict(pidx_=None), dict(st_=None), dict(msgs_=None), dict(claim_=None),
                dict(state_=p(state, 8)), dict(pidx_=p(pidx, 2)), dict(claim_=p(claim, 2)), dict(at=118),
                dict(at=148), dict(stride=96, at=84), dict(stride=8, at=0), dict(n_=1 << 32)):
        assert mac1(**bad) == -1, bad
        assert b"peer mac1" in L.rg_last_error(), bad
    assert mac1(stride=96, at=80) == 0  # the field may end with the row (statuses of 0xA5: no row was sent)
    torch.cuda.synchronize()
    for t in (state, res, st, ws, keys, table, desc, buf, ck, has, msgs):
        assert (t.cpu().numpy() == FILL).all()
    for t in (po, pidx):
        assert (_u32(t) == GUARD).all()
    assert (_u32(claim)[:npeers] == 0).all() and _u32(claim)[npeers] == GUARD  # the one accepted mac1 call zeroed it
