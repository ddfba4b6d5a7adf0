"""Device-resident cryptokey routing: rg_route_batch_dev, rg_route_check_batch_dev and rg_send_batch_dev_routed
against the Python models of route_cases.py (a brute-force longest-prefix match and the per-packet rules restated
over plain integers).  Each test asserts that the verdict classes it is there for occur in its batch."""
import numpy as np
import pytest
import torch

import route_cases as rc
import send_cases as sc
from oracle import oracle
from rustyguard_amd import aead, route
from rustyguard_amd._lib import RgError

pytestmark = pytest.mark.gpu

KEYS = np.random.default_rng(91).integers(0, 256, (rc.NKEYS, 32), dtype=np.uint8)
RECV = np.array([0x1111, 0x3333, 0x5555, 0x7777, 0x9999], np.uint32)  # receiver ids; key row = state row = index
STATE = sc.rows(10, (1 << 32) - 20, 7, 1 << 40, 99)
NOW = sc.T0 + 9


def _u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).cuda()


def _i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()


def _desc(d):
    return torch.from_numpy(np.ascontiguousarray(d).view(np.uint8).reshape(-1, 16).copy()).cuda()


def _np_u32(t):
    return t.cpu().numpy().view(np.uint32)


def _table(rows):
    return _u32(route.build_table(rc.prefix_rows(rows)))


@pytest.fixture(scope="module")
def table():
    return _table(rc.ROWS)


@pytest.fixture(scope="module")
def batches():
    """n -> (desc, buf, kinds, model outputs), computed once."""
    out = {}
    for n in rc.BATCH_SIZES:
        desc, buf, kinds = rc.send_batch(n, 100 + n)
        out[n] = (desc, buf, kinds, rc.route_model(rc.ROWS, rc.peer_slots(), desc, buf))
    return out


def _route(engine, table, peer_slot, desc, buf, with_peers=True):
    n = len(desc)
    db = torch.from_numpy(buf.copy()).cuda()
    peers = torch.full((n,), 0x6E6E6E6E, dtype=torch.int32, device="cuda") if with_peers else None
    slots = torch.full((n,), 0x6E6E6E6E, dtype=torch.int32, device="cuda")
    dout = torch.full((n, 16), 0xEE, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    route.route_batch_dev(engine, table, _u32(peer_slot), _desc(desc), db, slots, dout, st, peers_out=peers)
    torch.cuda.synchronize()
    return (_np_u32(peers) if with_peers else None, _np_u32(slots), dout.cpu().numpy().reshape(-1).view(rc.DESC_DTYPE),
            st.cpu().numpy(), db.cpu().numpy())


ALL_SEND = {rc.OK, rc.INVALID, rc.UNALIGNED, rc.UNROUTABLE, rc.REJECTED}


@pytest.mark.parametrize("n", rc.BATCH_SIZES)
def test_route_matches_model(engine, table, batches, n):
    desc, buf, kinds, (peers, slots, dout, status, want) = batches[n]
    g_peers, g_slots, g_dout, g_st, got = _route(engine, table, rc.peer_slots(), desc, buf)
    assert np.array_equal(g_st, status), [(i, kinds[i], g_st[i], status[i]) for i in np.nonzero(g_st != status)[0][:5]]
    assert np.array_equal(g_peers, peers) and np.array_equal(g_slots, slots)
    assert np.array_equal(g_dout, dout)
    assert np.array_equal(got, want)  # the zeroed padding; every other byte, untouched frames included, as it was
    if n >= 63:
        assert set(status) == ALL_SEND
        assert set(desc["len"]) >= set(rc.INNER_LENGTHS)
        assert not np.array_equal(want, buf) and ((desc["len"] % 16 != 0) & (status == rc.OK)).sum() >= 10
        assert ((desc["len"] % 16 == 0) & (status == rc.OK)).any()
        bad = status != rc.OK
        assert (slots[bad] == rc.SKIP).all() and np.array_equal(dout["len"][bad], desc["len"][bad])
        assert (peers[status == rc.REJECTED] == rc.NO_SESSION).all()  # whom to start a handshake with
        assert {"short", "version", "ihl", "total_long", "total_short", "outside"} <= {kinds[i] for i in
                                                                                     np.nonzero(status == rc.INVALID)[0]}
        assert {"none", "beyond"} == {kinds[i] for i in np.nonzero(status == rc.UNROUTABLE)[0]}
    else:
        assert list(status) == [rc.OK]


def test_route_in_place_descriptors_and_no_peers(engine, table, batches):
    """desc_out may be desc itself, peers_out may be NULL."""
    desc, buf, _, (_, slots, dout, status, want) = batches[65]
    dd, db = _desc(desc), torch.from_numpy(buf.copy()).cuda()
    gs = torch.zeros(65, dtype=torch.int32, device="cuda")
    st = torch.full((65,), 0xEE, dtype=torch.uint8, device="cuda")
    route.route_batch_dev(engine, table, _u32(rc.peer_slots()), dd, db, gs, dd, st)
    torch.cuda.synchronize()
    assert np.array_equal(dd.cpu().numpy().reshape(-1).view(rc.DESC_DTYPE), dout) and np.array_equal(_np_u32(gs), slots)
    assert np.array_equal(st.cpu().numpy(), status) and np.array_equal(db.cpu().numpy(), want)


class Sender:
    def __init__(self, engine, n, state=STATE):
        self.engine = engine
        self.keys = torch.from_numpy(KEYS.copy()).cuda()
        self.recv = _u32(RECV)
        self.state = _i64(np.asarray(state, np.uint64).reshape(-1))
        self.peer_slot = _u32(rc.peer_slots())
        self.ws = route.route_workspace(engine, n, rc.NKEYS)
        self.send_ws = engine.send_workspace(n, rc.NKEYS)
        self.now = _i64(np.array([NOW], np.uint64))

    def rows(self):
        return self.state.cpu().numpy().view(np.uint64).reshape(-1, 3)

    def outputs(self, n):
        return (torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda"),
                torch.full((n,), -1, dtype=torch.int64, device="cuda"),
                torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda"))

    def routed(self, table, desc, buf, stream=None):
        n = len(desc)
        db = torch.from_numpy(buf.copy()).cuda()
        st, ctr, rk = self.outputs(n)
        peers = torch.full((n,), 0x6E6E6E6E, dtype=torch.int32, device="cuda")
        route.send_batch_dev_routed(self.engine, self.keys, self.recv, self.state, table, self.peer_slot, _desc(desc),
                                    db, st, peers_out=peers, counters_out=ctr, rekey_out=rk, now_ns=self.now,
                                    workspace=self.ws, stream=stream)
        torch.cuda.synchronize()
        return st.cpu().numpy(), ctr.cpu().numpy().view(np.uint64), rk.cpu().numpy(), _np_u32(peers), db.cpu().numpy()

    def separate(self, table, desc, buf):
        """rg_route_batch_dev, rg_send_batch_dev_resident over its outputs, the overlay on the host."""
        n = len(desc)
        db = torch.from_numpy(buf.copy()).cuda()
        slots = torch.zeros(n, dtype=torch.int32, device="cuda")
        dout = torch.zeros((n, 16), dtype=torch.uint8, device="cuda")
        rst = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        peers = torch.zeros(n, dtype=torch.int32, device="cuda")
        route.route_batch_dev(self.engine, table, self.peer_slot, _desc(desc), db, slots, dout, rst, peers_out=peers)
        st, ctr, rk = self.outputs(n)
        self.engine.send_batch_dev_resident(self.keys, self.recv, self.state, slots, dout, db, st, ctr, rk, self.now,
                                            workspace=self.send_ws)
        torch.cuda.synchronize()
        r, s = rst.cpu().numpy(), st.cpu().numpy()
        return (np.where(r != rc.OK, r, s).astype(np.uint8), ctr.cpu().numpy().view(np.uint64), rk.cpu().numpy(),
                _np_u32(peers), db.cpu().numpy())


@pytest.mark.parametrize("n", rc.BATCH_SIZES)
def test_routed_send_equals_the_three_calls(engine, table, batches, n):
    desc, buf, _, (peers, slots, dout, status, padded) = batches[n]
    a, b = Sender(engine, n), Sender(engine, n)
    want = a.separate(table, desc, buf)
    got = b.routed(table, desc, buf)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert np.array_equal(a.rows(), b.rows())
    fin, ctr, _, g_peers, frames = got
    assert np.array_equal(g_peers, peers) and np.array_equal(fin, status)  # every routed packet sealed: OK
    assert (ctr[status != rc.OK] == 0).all()
    assert int(b.rows()[:, 0].sum() - STATE[:, 0].sum()) == int((status == rc.OK).sum())  # one counter per routed packet
    # and the frames are the oracle's seal of the padded packets under those counters
    ok = status == rc.OK
    ref = padded.copy()
    oracle.seal_batch(KEYS, RECV, np.ascontiguousarray(dout[ok]), ctr[ok], ref)
    assert np.array_equal(frames, ref)
    ws_desc = b.ws[:16 * n].cpu().numpy().view(rc.DESC_DTYPE)  # the workspace begins with the working descriptors
    assert np.array_equal(ws_desc, dout)
    if n >= 63:
        assert set(fin) == ALL_SEND and len(set(slots[ok])) == rc.NKEYS


def test_routed_send_verdicts_of_the_send_itself(engine, table, batches):
    """A routed packet whose session has run out of counters is the resident send's RG_PKT_REJECTED; the packets
    the route turned away keep the route's verdicts beside it."""
    desc, buf, _, (_, slots, _, status, _) = batches[257]
    state = STATE.copy()
    state[2, 0] = sc.REJECT - 3  # key row 2 has three counters left
    a, b = Sender(engine, 257, state), Sender(engine, 257, state)
    want, got = a.separate(table, desc, buf), b.routed(table, desc, buf)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert np.array_equal(a.rows(), b.rows())
    on2 = np.nonzero((status == rc.OK) & (slots == 2))[0]
    assert len(on2) > 5 and list(got[0][on2[:3]]) == [rc.OK] * 3 and (got[0][on2[3:]] == rc.REJECTED).all()
    rest = np.ones(257, bool)
    rest[on2] = False
    assert np.array_equal(got[0][rest], status[rest]) and set(got[0]) == ALL_SEND


def _receiver(engine, n):
    keys = torch.from_numpy(KEYS.copy()).cuda()
    rx = torch.from_numpy(aead.rx_table(RECV, np.arange(rc.NKEYS, dtype=np.uint32)).view(np.int32).copy()).cuda()
    win = torch.zeros(rc.NKEYS * 33, dtype=torch.int64, device="cuda")
    ws = engine.replay_workspace(n, rc.NKEYS)

    def recv(desc, db):
        st = torch.full((len(desc),), 0xEE, dtype=torch.uint8, device="cuda")
        key = torch.full((len(desc),), -7, dtype=torch.int32, device="cuda")
        engine.recv_batch_dev_resident(keys, rx, win, _desc(desc), db, st, None, key, workspace=ws)
        return st, key

    return recv


def _check(engine, table, slot_peer, desc, key, db, st):
    """-> (status, inner_len) of rg_route_check_batch_dev on a copy of st."""
    st = st.clone()
    inner = torch.full((len(desc),), 0x6E6E6E6E, dtype=torch.int32, device="cuda")
    before = db.clone()
    route.route_check_batch_dev(engine, table, _u32(slot_peer), _desc(desc), key, db, st, inner)
    torch.cuda.synchronize()
    assert torch.equal(db, before)  # buf is only read
    return st.cpu().numpy(), _np_u32(inner)


def test_check_matches_model(engine, table):
    """Sealed frames through rg_recv_batch_dev_resident, then the check on its statuses, key rows and plaintexts."""
    inner = rc.recv_inner(90, 5)
    inner.append((0, inner[0][1].copy(), "forged"))  # one more frame of session 0, its ciphertext then damaged
    rng = np.random.default_rng(6)
    n = len(inner) + 1  # and a replay of frame 0 at the end
    desc = np.zeros(n, rc.DESC_DTYPE)
    ctr, off = [], 0
    per = [0] * rc.NKEYS
    for i, (s, pkt, _) in enumerate(inner):
        desc[i] = (off, len(pkt), s)
        ctr.append(per[s])
        per[s] += 1
        off += (len(pkt) + 32 + 16 + 15) // 16 * 16
    buf = rng.integers(0, 256, off + 96, dtype=np.uint8)
    for d, (_, pkt, _) in zip(desc, inner):
        buf[int(d["offset"]) + 16:int(d["offset"]) + 16 + len(pkt)] = pkt
    oracle.seal_batch(KEYS, RECV, np.ascontiguousarray(desc[:-1]), np.array(ctr, np.uint64), buf)
    desc["len"][:-1] += 32  # frame lengths
    buf[int(desc["offset"][n - 2]) + 20] ^= 1  # statuses the check must leave alone: a bad tag ...
    o, w = int(desc["offset"][0]), int(desc["len"][0])
    assert w <= 96
    desc[n - 1] = (off, w, 0)
    buf[off:off + w] = buf[o:o + w]  # ... and a replayed counter
    db = torch.from_numpy(buf.copy()).cuda()
    st, key = _receiver(engine, n)(desc, db)
    torch.cuda.synchronize()
    st_h, key_h, plain = st.cpu().numpy(), _np_u32(key), db.cpu().numpy()
    kinds = np.array([k for _, _, k in inner] + ["replayed"])
    assert (st_h[:-2] == rc.OK).all() and st_h[-2] == rc.ERR and st_h[-1] == rc.REJECTED
    slot_peer = np.array(rc.SRC_PEER + (3, 4), np.uint32)
    want_st, want_len = rc.check_model(rc.ROWS, slot_peer, desc, key_h, plain, st_h)
    got_st, got_len = _check(engine, table, slot_peer, desc, key, db, st)
    assert np.array_equal(got_st, want_st), [(i, kinds[i]) for i in np.nonzero(got_st != want_st)[0][:5]]
    assert np.array_equal(got_len, want_len)
    # every class, by what the packets were made to be
    assert (want_st[kinds == "own"] == rc.OK).all() and (want_len[kinds == "own"] >= 20).all()
    assert (want_st[kinds == "other"] == rc.UNROUTABLE).all() and (want_st[kinds == "none"] == rc.UNROUTABLE).all()
    assert (want_st[kinds == "keepalive"] == rc.OK).all() and (want_len[kinds == "keepalive"] == 0).all()
    assert (want_st[kinds == "not_ip"] == rc.INVALID).all() and (want_st[kinds == "short_total"] == rc.INVALID).all()
    assert want_st[-2] == rc.ERR and want_st[-1] == rc.REJECTED and (want_len[want_st != rc.OK] == 0).all()
    for k in ("own", "other", "none", "keepalive", "not_ip", "short_total"):
        assert (kinds == k).sum() >= 5, k
    own = kinds == "own"
    assert (want_len[own] < desc["len"][own] - 32).any() and (want_len[own] == desc["len"][own] - 32).any()
    # a key row beyond slot_peer: unroutable, whatever the source
    short_st, short_len = _check(engine, table, slot_peer[:2], desc, key, db, st)
    m_st, m_len = rc.check_model(rc.ROWS, slot_peer[:2], desc, key_h, plain, st_h)
    assert np.array_equal(short_st, m_st) and np.array_equal(short_len, m_len)
    assert (short_st[own & (key_h == 2)] == rc.UNROUTABLE).all() and (own & (key_h == 2)).sum() >= 5
    # inner_len_out is optional
    st2 = st.clone()
    route.route_check_batch_dev(engine, table, _u32(slot_peer), _desc(desc), key, db, st2)
    torch.cuda.synchronize()
    assert np.array_equal(st2.cpu().numpy(), want_st)


def test_round_trip(engine, table, batches):
    """Routed send -> resident receive -> check: exactly the packets the model lets through arrive, and
    inner_len_out trims the padding the sender added."""
    n = 257
    desc, buf, _, (peers, slots, dout, status, padded) = batches[n]
    fin, _, _, _, frames = Sender(engine, n).routed(table, desc, buf)
    assert np.array_equal(fin, status)
    sent = np.nonzero(fin == rc.OK)[0]
    fdesc = np.zeros(len(sent), rc.DESC_DTYPE)
    fdesc["offset"], fdesc["len"] = dout["offset"][sent], dout["len"][sent] + 32
    db = torch.from_numpy(frames.copy()).cuda()
    st, key = _receiver(engine, len(sent))(fdesc, db)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == rc.OK).all() and np.array_equal(_np_u32(key), slots[sent])
    plain = db.cpu().numpy()
    for d in fdesc:  # the plaintexts are back, padding and all (header and tag stay the frame's)
        o, w = int(d["offset"]), int(d["len"])
        assert np.array_equal(plain[o + 16:o + w - 16], padded[o + 16:o + w - 16])
    # the receiving side's view: key row k belongs to the peer the sender routed row k's traffic to first
    slot_peer = np.array([10, 1, 12, 13, 14], np.uint32)
    want_st, want_len = rc.check_model(rc.ROWS, slot_peer, fdesc, slots[sent], plain, np.zeros(len(sent), np.uint8))
    got_st, got_len = _check(engine, table, slot_peer, fdesc, key, db, st)
    assert np.array_equal(got_st, want_st) and np.array_equal(got_len, want_len)
    # every packet's source is peer 10's: only what went out on peer 10's key row comes through
    delivered = got_st == rc.OK
    assert np.array_equal(delivered, slots[sent] == 0) and 10 < delivered.sum() < len(sent)
    assert (got_st[~delivered] == rc.UNROUTABLE).all()
    trimmed = 0
    for j in np.nonzero(delivered)[0]:
        i, o = sent[j], int(fdesc["offset"][j]) + 16
        L = int(desc["len"][i])
        total = int(buf[o + 2]) << 8 | int(buf[o + 3])
        assert got_len[j] == total <= L
        assert np.array_equal(padded[o:o + total], buf[o:o + total])
        trimmed += int(fdesc["len"][j]) - 32 > total
    assert trimmed >= 5


def test_table_switch_between_batches(engine, table, batches):
    desc, buf, _, (_, _, _, status, _) = batches[65]
    other_rows = [(rc.ip(10, 1, 2, 0), 24, 1), (rc.ip(10, 9, 0, 0), 16, rc.NO_SESSION)]
    other = _table(other_rows)
    m_peers, m_slots, m_dout, m_status, m_buf = rc.route_model(other_rows, rc.peer_slots(), desc, buf)
    assert (m_status != status).any() and {rc.OK, rc.UNROUTABLE, rc.REJECTED} <= set(m_status)
    s = Sender(engine, 65)
    first = s.routed(table, desc, buf)
    second = s.routed(other, desc, buf)  # the other pointer from the next batch on; counters carry on
    third = s.routed(table, desc, buf)
    assert np.array_equal(first[0], status) and np.array_equal(second[0], m_status) and np.array_equal(third[0], status)
    assert np.array_equal(second[3], m_peers)
    ok = m_status == rc.OK
    # the second batch's counters on key row 1 carry on behind the first batch's
    start = np.uint64(int(first[1][(status == rc.OK) & (first[3] == 1)].max()) + 1)
    assert (m_slots[ok] == 1).all() and np.array_equal(second[1][ok], start + np.arange(ok.sum(), dtype=np.uint64))


def test_graph_capture(engine, table, batches):
    n = 65
    desc, buf, _, _ = batches[n]
    a, b = Sender(engine, n), Sender(engine, n)
    direct = [a.routed(table, desc, buf), a.routed(table, desc, buf)]  # (also grows the context's buffers)
    assert not np.array_equal(direct[0][4], direct[1][4])  # the second call's counters differ
    dd, db = _desc(desc), torch.from_numpy(buf.copy()).cuda()
    st, ctr, rk = b.outputs(n)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin()
        route.send_batch_dev_routed(engine, b.keys, b.recv, b.state, table, b.peer_slot, dd, db, st, counters_out=ctr,
                                    rekey_out=rk, now_ns=b.now, workspace=b.ws, stream=s)
        g.capture_end()
    torch.cuda.synchronize()
    assert np.array_equal(db.cpu().numpy(), buf) and np.array_equal(b.rows(), STATE)  # captured, not run
    for want in direct:
        db.copy_(torch.from_numpy(buf))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(st.cpu().numpy(), want[0]) and np.array_equal(ctr.cpu().numpy().view(np.uint64), want[1])
        assert np.array_equal(rk.cpu().numpy(), want[2]) and np.array_equal(db.cpu().numpy(), want[4])
    assert np.array_equal(a.rows(), b.rows())


def test_einval_enqueues_nothing(engine, table, batches):
    n = 65
    desc, buf, _, _ = batches[n]
    s = Sender(engine, n)
    dd, db = _desc(desc), torch.from_numpy(buf.copy()).cuda()
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    slots = torch.full((n,), 0x6E6E6E6E, dtype=torch.int32, device="cuda")
    dout = torch.full((n, 16), 0xEE, dtype=torch.uint8, device="cuda")
    key = torch.zeros(n, dtype=torch.int32, device="cuda")
    L, h = engine.library, engine.handle
    p = lambda t: t.data_ptr()  # noqa: E731
    words = table.numel()
    calls = {  # name -> (function, good arguments, indices of the required pointers)
        "route": (L.rg_route_batch_dev, [h, p(table), words, p(s.peer_slot), rc.NPEERS, p(dd), n, p(db), db.numel(), None,
                                         p(slots), p(dout), p(st), None], (1, 3, 5, 7, 10, 11, 12)),
        "check": (L.rg_route_check_batch_dev, [h, p(table), words, p(s.peer_slot), rc.NPEERS, p(dd), p(key), n, p(db),
                                               db.numel(), p(st), None, None], (1, 3, 5, 6, 8, 10)),
        "routed": (L.rg_send_batch_dev_routed, [h, p(s.keys), p(s.recv), rc.NKEYS, p(s.state), p(table), words,
                                                p(s.peer_slot), rc.NPEERS, p(dd), n, p(s.now), p(db), db.numel(), None,
                                                p(st), None, None, p(s.ws), s.ws.numel(), None],
                   (1, 2, 4, 5, 7, 9, 12, 15, 18)),
    }
    # where each call keeps table_words, n and buf
    at = {"route": (2, 6, 7), "check": (2, 7, 8), "routed": (6, 10, 12)}
    tried = 0
    for name, (fn, good, required) in calls.items():
        w_at, n_at, buf_at = at[name]
        edits = [(k, None) for k in required] + [(w_at, 65535), (n_at, 1 << 32), (buf_at, p(db) + 8)]
        if name == "routed":
            edits += [(3, 0), (4, p(s.state) + 4), (18, p(s.ws) + 8), (19, s.ws.numel() - 256), (19, 0)]
        for k, value in edits:
            args = list(good)
            args[k] = value
            assert fn(*args) == -1, (name, k, value)
            assert L.rg_last_error()
            tried += 1
    assert tried == 7 + 3 + 6 + 3 + 9 + 3 + 5
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0xEE).all() and np.array_equal(db.cpu().numpy(), buf)
    assert (_np_u32(slots) == 0x6E6E6E6E).all() and (dout.cpu().numpy() == 0xEE).all()
    assert np.array_equal(s.rows(), STATE)
    with pytest.raises(RgError):  # the wrapper raises
        route.route_batch_dev(engine, table[:65535], s.peer_slot, dd, db, slots, dout, st)
    # n == 0 is RG_OK
    assert L.rg_route_batch_dev(h, None, 0, None, 0, None, 0, None, 0, None, None, None, None, None) == 0
    assert L.rg_route_check_batch_dev(h, None, 0, None, 0, None, None, 0, None, 0, None, None, None) == 0
    assert L.rg_send_batch_dev_routed(h, None, None, 0, None, None, 0, None, 0, None, 0, None, None, 0, None, None, None,
                                      None, None, 0, None) == 0
    # and the good arguments do run
    assert calls["route"][0](*calls["route"][1]) == 0
    torch.cuda.synchronize()
    assert (st.cpu().numpy() != 0xEE).all()
