"""The device-resident pending handshakes on the GPU (rg_pending_install_batch_dev, rg_pending_turn_dev,
rg_pending_index_dev) against the in-order Python model (tests/pending_cases.py), and in the loop they exist for:
a transport turn's rekey list -> the pending turn -> the initiator chain -> the install, the responder's answers ->
finish -> session install -> arm, a lost response retried and an abandoned row reaped, with no host read between
the calls.  Every output array has a guard entry behind it, and every byte of every table array is compared."""
import ctypes

import numpy as np
import pytest

import handshake_cases as hc
import pending_cases as pc
import timer_cases as tc
from conftest import load_golden
from rustyguard_amd import _lib, aead, pending, session, timers
from rustyguard_amd.workloads import DESC_DTYPE

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL = 0xA5
GUARD = 0xA5A5A5A5
NOW = 10**12
OK, INV, REJ, NONE = pc.OK, pc.INVALID, pc.REJECTED, pc.NONE
SIZES = (1, 63, 64, 65, 2047, 2049, 4099)
SEC = 10**9


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _words(values):
    return _dev(np.array(values, np.uint32).view(np.int32))


def _clock(now):
    return _dev(np.array([now], np.uint64).view(np.int64))


def _fill(shape, dtype=torch.uint8):
    if dtype == torch.uint8:
        return torch.full(shape, FILL, dtype=dtype, device="cuda")
    return torch.full(shape, GUARD - (1 << 32), dtype=torch.int32, device="cuda")  # the same bytes


def _u32(t):
    return [int(x) for x in t.cpu().numpy().view(np.uint32).reshape(-1)]


def _u8(t):
    return [int(x) for x in t.cpu().numpy().reshape(-1)]


def _same(name, got, want):
    assert len(got) == len(want), name
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (name, len(bad), bad[:8], [(got[i], want[i]) for i in bad[:2]])


def _rows_dev(rows):
    return _dev(np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), pc.ROW))


def _rows(t):
    a = t.cpu().numpy().reshape(-1, pc.ROW)
    return [r.tobytes() for r in a]


def put_table(engine, t, pend_cap=None):
    """the model's table on the device; pend_table holds stale bytes, which every call replaces"""
    npeers = len(t["pending"])
    T = pending.PendingTables(engine, npeers, pend_cap)
    if npeers:
        T.pending[:] = _rows_dev(t["pending"])
        T.timers[:] = _dev(np.array(t["timers"], np.uint64).reshape(npeers, 2).view(np.uint8).reshape(npeers, 16))
        T.hs_ids[:] = _words(t["hs_ids"])
    T.pend_table.fill_(0x01020304)
    return T


def get_table(T):
    tm = T.timers.cpu().numpy().view(np.uint64).reshape(-1, 2)
    return {"pending": _rows(T.pending), "timers": [(int(a), int(b)) for a, b in tm], "hs_ids": _u32(T.hs_ids)}


def check_table(T, want, gone=()):
    """every byte of pending, timers and hs_ids; pend_table through its lookup: every live id answers its peer, every
    id in `gone` (dead, replaced or never installed) answers nothing, and the table holds nothing else"""
    got = get_table(T)
    for name in ("pending", "timers", "hs_ids"):
        _same(name, got[name], want[name])
    table = np.ascontiguousarray(T.pend_table.cpu().numpy().view(np.uint32).reshape(-1, 2))
    find = _lib.lib().rg_rx_table_find
    ptr = table.ctypes.data_as(ctypes.c_void_p)
    live = pc.lookup(want)
    for ident, p in live.items():
        assert find(ptr, T.pend_cap, ident) == p, (hex(ident), p)
    for ident in gone:
        if ident not in live:
            assert find(ptr, T.pend_cap, ident) == -1, hex(ident)
    used = table[table[:, 1] != NONE]
    assert sorted((int(a), int(b)) for a, b in used) == sorted(live.items())
    assert (table[table[:, 1] == NONE, 0] == NONE).all()


class Outputs:
    """the turn's four output arrays with a guard entry behind each"""

    def __init__(self, npeers):
        self.npeers = npeers
        self.init, self.gate = _fill((npeers + 1,), torch.int32), _fill((npeers + 1,))
        self.expired, self.counts = _fill((npeers + 1,)), _fill((3,), torch.int32)

    def turn(self, engine, T, d_now, start_peers=None, start_status=None, match=OK, ws=None, stream=None, expired=True):
        p = self.npeers
        return pending.turn_dev(engine, T, d_now, self.init[:p], self.gate[:p], self.counts[:2], start_peers=start_peers,
                                start_status=start_status, start_match=match,
                                expired_out=self.expired[:p] if expired else None, workspace=ws, stream=stream)

    def read(self):
        torch.cuda.synchronize()
        p = self.npeers
        init, gate, expired, counts = _u32(self.init), _u8(self.gate), _u8(self.expired), _u32(self.counts)
        assert init[p] == GUARD and gate[p] == FILL and expired[p] == FILL and counts[2] == GUARD
        return init[:p], gate[:p], expired[:p], counts[:2]


def turn_vs_model(engine, t, now, peers=(), status=None, match=OK):
    T, out = put_table(engine, t), Outputs(len(t["pending"]))
    out.turn(engine, T, _clock(now), _words(peers) if len(peers) else None,
             None if status is None else _dev(np.array(status, np.uint8)), match)
    want = pc.turn_loop(t, now, peers, status, match)
    for name, g, w in zip(("init_peers_out", "init_gate_out", "expired_out", "counts_out"), out.read(), want[1:]):
        _same(name, g, w)
    check_table(T, want[0], [pc.row_sender(r) for r in t["pending"]])
    return want, T, out


# -------------------------------------------------------------------- turn
@pytest.mark.parametrize("npeers", SIZES)
def test_turn_sizes_against_the_model(engine, npeers):
    """wave edges, the scan-tile edge and more than two tiles; live, dead, expiring and retrying rows with times one
    below, at and one above each deadline; request lists of every length with duplicates, padding and entries past
    the table, with and without a status to match"""
    for m in (0, 1, 65, 2049):
        t = pc.random_table(npeers, 100 * npeers + m, NOW)
        peers, status = pc.request_list(npeers, m, 7 * npeers + m)
        for st in (None, status):
            want = turn_vs_model(engine, t, NOW, peers, st, REJ)[0]
        if npeers >= 2047:
            assert want[4][0] > 0 and want[4][1] > 0


def test_turn_same_clock_twice_and_no_expired_array(engine):
    """the list is padded with RG_PEER_NONE and the gate with RG_PKT_REJECTED over the full npeers; a second turn at
    the same clock lists nothing and changes no byte; expired_out may be NULL"""
    npeers = 2049
    t = pc.random_table(npeers, 77, NOW)
    want, T, out = turn_vs_model(engine, t, NOW)
    k, nexp = want[4]
    assert 0 < k < npeers and 0 < nexp < npeers
    assert want[1][:k] == sorted(want[1][:k]) and want[1][k:] == [NONE] * (npeers - k)
    assert want[2] == [OK] * k + [REJ] * (npeers - k)
    out.turn(engine, T, _clock(NOW))
    assert out.read() == ([NONE] * npeers, [REJ] * npeers, [0] * npeers, [0, 0])
    check_table(T, want[0])
    T2, out2 = put_table(engine, t), Outputs(npeers)
    out2.turn(engine, T2, _clock(NOW), expired=False)
    got = out2.read()
    assert got[0] == want[1] and got[1] == want[2] and got[2] == [FILL] * npeers and got[3] == want[4]
    check_table(T2, want[0])
    # no peers: the counts alone
    T0, out0 = pending.PendingTables(engine, 0), Outputs(0)
    assert T0.pend_cap == 2
    out0.turn(engine, T0, _clock(NOW), _words([0, 1]))
    assert out0.read() == ([], [], [], [0, 0]) and _u32(T0.pend_table) == [NONE] * 4


# ----------------------------------------------------------------- install
@pytest.mark.parametrize("npeers", (5, 4099))
@pytest.mark.parametrize("n", (1, 64, 65, 2049))
def test_install_against_the_model(engine, n, npeers):
    """synthetic rows: a gate with holes, peers past the table, rows of one peer on both sides of a wave edge and of
    a tile edge; the consumed batch is all wiped, a retry keeps `started`, the replaced ids answer nothing"""
    t = pc.random_table(npeers, 31 * n + npeers, NOW - 6 * SEC)
    batch, gate = pc.install_batch(n, npeers, n + npeers)
    for g in ((gate, None) if n == 65 else (gate,)):
        T = put_table(engine, t)
        d_batch, status, installed = _fill((n + 1, pc.ROW)), _fill((n + 1,)), _fill((n + 1,), torch.int32)
        d_batch[:n] = _rows_dev(batch)
        pending.install_dev(engine, T, d_batch[:n], None if g is None else _dev(np.array(g, np.uint8)), _clock(NOW),
                            status[:n], installed[:n])
        torch.cuda.synchronize()
        want, w_batch, w_status, w_installed = pc.install_loop(t, batch, g, NOW)
        got_st, got_in, got_batch = _u8(status), _u32(installed), _rows(d_batch)
        assert got_st[n] == FILL and got_in[n] == GUARD and got_batch[n] == bytes([FILL]) * pc.ROW
        _same("status", got_st[:n], w_status)
        _same("installed_out", got_in[:n], w_installed)
        _same("batch", got_batch[:n], w_batch)
        assert all(b == pc.EMPTY for b, s in zip(w_batch, w_status) if s != REJ)
        check_table(T, want, [pc.row_sender(r) for r in batch + t["pending"]])
        kept = [p for p in range(npeers) if pc.is_live(t, p) and pc.row_peer(want["pending"][p]) == p
                and want["pending"][p] != t["pending"][p]]
        if n >= 64:
            assert kept and all(want["timers"][p] == (t["timers"][p][0], NOW) for p in kept)


# ------------------------------------------------------------------- index
def test_index_with_every_id_in_one_home_slot(engine):
    """pend_cap = 2 npeers rounded up to a power of two; 65 live ids with one home slot: the probe runs the whole
    cluster and finds every one; a row wiped as the finish call wipes it leaves the table at the next rebuild"""
    npeers = 65
    assert pending.PendingTables(engine, npeers).pend_cap == 256 and pending.PendingTables(engine, 64).pend_cap == 128
    ids = pc.colliding_ids(npeers, 256)
    rng = np.random.default_rng(5)
    t = pc.empty_table(npeers)
    t["pending"] = [pc.make_row(p, ids[p], rng) for p in range(npeers)]
    T = put_table(engine, t)
    pending.index_dev(engine, T)
    torch.cuda.synchronize()
    check_table(T, t)
    table = T.pend_table.cpu().numpy().view(np.uint32).reshape(-1, 2)
    assert sorted(int(x) for x in np.flatnonzero(table[:, 1] != NONE)) == list(range(5, 5 + npeers))
    T.pending[7] = _rows_dev([pc.EMPTY])[0]
    t["pending"][7] = pc.EMPTY
    pending.index_dev(engine, T)
    torch.cuda.synchronize()
    check_table(T, t, [ids[7]])
    with pytest.raises(_lib.RgError, match="pend_cap"):
        pending.index_dev(engine, put_table(engine, t, pend_cap=128))


# -------------------------------------------------------------- fail closed
def test_short_workspace_enqueues_nothing(engine):
    npeers, n = 65, 9
    t = pc.random_table(npeers, 3, NOW)
    T, out = put_table(engine, t), Outputs(npeers)
    need = pending.workspace_size(engine, n, 4, npeers)
    ws = _fill((need,))
    with pytest.raises(_lib.RgError, match="pending turn"):
        out.turn(engine, T, _clock(NOW), _words([1, 2, 3, 4]), ws=ws[:need - 1])
    batch, status, installed = _fill((n, pc.ROW)), _fill((n,)), _fill((n,), torch.int32)
    with pytest.raises(_lib.RgError, match="pending install"):
        pending.install_dev(engine, T, batch, None, _clock(NOW), status, installed, workspace=ws[:need - 1])
    assert out.read() == ([GUARD] * npeers, [FILL] * npeers, [FILL] * npeers, [GUARD] * 2)
    assert _u8(status) == [FILL] * n and _u32(installed) == [GUARD] * n and (batch.cpu().numpy() == FILL).all()
    assert (ws.cpu().numpy() == FILL).all() and _u32(T.pend_table) == [0x01020304] * (2 * T.pend_cap)
    got = get_table(T)
    assert got == t


# ------------------------------------------------------- the loop it is for
NP, LISTED = 8, (0, 3, 5)


class World:
    """A, the initiator with the recorded static key of golden/handshake_full.json, and its eight peers, of which
    peers 0, 3 and 5 are responders that answer (peer 0 the recorded one); every array the chain takes, allocated
    once, so that the same calls can be captured."""

    def __init__(self, engine, seed):
        g = load_golden("handshake_full.json")["handshake"]
        rng = np.random.default_rng(seed)
        self.rb = rb = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
        sk_a = bytes.fromhex(g["static_private_i"])
        pk_a = hc.pubkey(sk_a)
        sk = {p: bytes.fromhex(g["static_private_r"]) if p == 0 else rb(32) for p in LISTED}
        psk = [bytes.fromhex(g["preshared_key"]) if p == 0 else rb(32) for p in range(NP)]
        pk = [hc.pubkey(sk[p]) if p in sk else hc.pubkey(rb(32)) for p in range(NP)]
        self.engine = engine
        self.a_own = _dev(np.frombuffer(sk_a + pk_a, np.uint8))
        self.a_peers = _dev(hc.peer_rows([(pk[p], psk[p], hc.mac1_key(pk[p])) for p in range(NP)]))
        self.b = {}
        for p in LISTED:
            rows = hc.peer_rows([(pk_a, psk[p], hc.mac1_key(pk_a))])
            self.b[p] = (_dev(np.frombuffer(sk[p] + pk[p], np.uint8)), _dev(rows), _dev(aead.peer_table(rows)))
        self.state_a = torch.zeros((NP, 64), dtype=torch.uint8, device="cuda")  # rg_hs_peer_state
        self.PT, self.out = pending.PendingTables(engine, NP), Outputs(NP)
        self.ws = pending.pending_workspace(engine, NP, NP, NP)
        self.d_ts = _dev(np.frombuffer(bytes.fromhex(g["timestamp"]) * NP, np.uint8).reshape(NP, 12))
        self.desc_i = _dev(np.array([(160 * i, 148, 0) for i in range(NP)], DESC_DTYPE).view(np.uint8).reshape(-1, 16))
        self.desc_r = _dev(np.array([(96 * i, 92, 0) for i in range(NP)], DESC_DTYPE).view(np.uint8).reshape(-1, 16))
        self.esk, self.sids = torch.zeros((NP, 32), dtype=torch.uint8, device="cuda"), _words([0] * NP)
        self.msgs, self.batch = torch.zeros((NP, 160), dtype=torch.uint8, device="cuda"), _fill((NP, pc.ROW))
        self.cookies, self.has_cookie, self.claim_a = _fill((NP, 16)), _fill((NP,)), _fill((NP,), torch.int32)
        self.st_init, self.st_inst, self.installed = _fill((NP,)), _fill((NP,)), _fill((NP,), torch.int32)

    def fresh(self, attempt):
        """the caller's part of an attempt: ephemeral keys and session ids, one per row of the list"""
        self.esk.copy_(_dev(np.frombuffer(self.rb(32 * NP), np.uint8).reshape(NP, 32)))
        ids = [0xA000 + 0x100 * attempt + k for k in range(NP)]
        self.sids.copy_(_words(ids))
        return ids

    def chain(self, d_now, start_peers=None, start_status=None, stream=None):
        """rg_pending_turn_dev -> cookies -> initiate -> mac1 -> rg_pending_install_batch_dev, each with n = NP"""
        e, o = self.engine, self.out
        o.turn(e, self.PT, d_now, start_peers, start_status, OK, ws=self.ws, stream=stream)
        e.peer_cookies_dev(self.state_a, o.init[:NP], self.cookies, self.has_cookie, stream=stream)
        e.handshake_initiate_dev(self.a_own, self.a_peers, o.init[:NP], o.gate[:NP], self.esk, self.d_ts, self.sids,
                                 self.cookies, self.has_cookie, self.msgs, self.batch, self.st_init, stream=stream)
        e.peer_mac1_dev(self.state_a, o.init[:NP], self.st_init, self.msgs, 160, 116, self.claim_a, stream=stream)
        pending.install_dev(e, self.PT, self.batch, self.st_init, d_now, self.st_inst, self.installed,
                            workspace=self.ws, stream=stream)

    def respond(self, answering, attempt):
        """the responder calls of every answering peer over the whole message array, merged on the device by their
        statuses -> (responses [NP][96], gate [NP], {peer: its transport keys [NP][64]})"""
        e = self.engine
        merged, gate, keys = torch.zeros((NP, 96), dtype=torch.uint8, device="cuda"), _dev(np.full(NP, REJ, np.uint8)), {}
        for p in answering:
            own, peers, table = self.b[p]
            results, responses, keys[p] = _fill((NP, 128)), _fill((NP, 96)), _fill((NP, 64))
            st1, st2 = _fill((NP,)), _fill((NP,))
            esk_b = _dev(np.frombuffer(self.rb(32 * NP), np.uint8).reshape(NP, 32))
            sid_b = _words([0xB000 + 0x100 * attempt + 0x10 * p + k for k in range(NP)])
            e.handshake_init_dev(own, peers, table, self.desc_i, None, self.msgs, results, st1)
            e.handshake_resp_dev(peers, results, st1, esk_b, sid_b, None, None, responses, keys[p], st2)
            ok = st2 == OK
            merged, gate = torch.where(ok[:, None], responses, merged), torch.where(ok, st2, gate)
        return merged, gate, keys

    def snapshot(self):
        torch.cuda.synchronize()
        return (get_table(self.PT), _u32(self.PT.pend_table), self.out.read(), _u8(self.st_init), _u8(self.st_inst),
                _u32(self.installed), _rows(self.batch), self.msgs.cpu().numpy().tobytes(),
                self.state_a.cpu().numpy().tobytes())


def test_rekey_retry_finish_and_expiry_with_no_host_read(engine):
    """Part 1: a transport table whose turn lists peers 0, 3 and 5 for a rekey -> the pending turn -> cookies ->
    initiate -> mac1 -> install.  Part 3 (before part 2, on the same rows): the responses are dropped, the clock
    moves 6 s and the turn lists exactly those peers again; the second install keeps `started`, moves `sent` and
    replaces the ids, and a response to the first attempt is RG_PKT_REJECTED.  Part 2: the responders' answers to
    the second attempt -> finish on tables.pending -> session install with hs_ids -> arm; both ends hold the same
    keys and the finished rows are dead.  Peer 5's answer is lost: 91 s after its last attempt the row expires."""
    w = World(engine, 2032)
    NK, t0 = 16, 500 * SEC
    TA, tm_a = session.SessionTables(engine, NK, NP), timers.timer_rows(engine, NK)
    old = np.zeros((NK, 3), np.uint64)
    old[:NP] = [(3, t0 - tc.REKEY_NS - 9 if p in LISTED else t0 - 9, t0 - 9) for p in range(NP)]
    TA.send_state[:] = _dev(old.view(np.uint8).reshape(NK, 24))
    TA.slot_peer[:NP], TA.peer_slot[:] = _words(range(NP)), _words(range(NP))
    TA.local_ids[:NP] = _words([0x900 + r for r in range(NP)])
    session.index_dev(engine, TA)
    tm = np.zeros((NK, 2), np.uint64)
    tm[:NP, 0] = [t0 - 1 if p in LISTED else t0 + tc.REKEY_NS for p in range(NP)]
    tm_a[:] = _dev(tm.view(np.uint8).reshape(NK, 16))
    ka, rk, rk_gate, rk_counts = _fill((NP,), torch.int32), _fill((NP,), torch.int32), _fill((NP,)), _fill((2,), torch.int32)
    d_now = _clock(t0)
    pad = [NONE] * (NP - len(LISTED))

    # ---- part 1
    timers.turn_dev(engine, TA, tm_a, d_now, ka, rk, rk_gate, rk_counts)
    ids0 = w.fresh(0)
    w.chain(d_now, rk, rk_gate)
    resp0, gate0, _ = w.respond(LISTED, 0)  # answers that will never arrive in time
    first = w.snapshot()
    assert _u32(rk) == list(LISTED) + pad and first[2] == (list(LISTED) + pad, [OK] * 3 + [REJ] * 5, [0] * NP, [3, 0])
    assert first[3] == first[4] == [OK] * 3 + [REJ] * 5 and first[5] == list(LISTED) + pad
    assert first[6][:3] == [pc.EMPTY] * 3 and first[6][3:] == [bytes([FILL]) * pc.ROW] * 5
    t1 = first[0]
    assert [pc.is_live(t1, p) for p in range(NP)] == [p in LISTED for p in range(NP)]
    assert [t1["timers"][p] for p in LISTED] == [(t0, t0)] * 3 and [t1["hs_ids"][p] for p in LISTED] == ids0[:3]
    assert pc.lookup(t1) == {ids0[k]: p for k, p in enumerate(LISTED)} and _u8(gate0) == [OK] * 3 + [REJ] * 5
    esk0 = w.esk.cpu().numpy()
    assert [t1["pending"][p][64:96] for p in LISTED] == [esk0[k].tobytes() for k in range(3)]

    # ---- part 3: nothing arrived; +3 s nothing is due, +6 s the same peers again
    d_now.copy_(_clock(t0 + 3 * SEC))
    timers.turn_dev(engine, TA, tm_a, d_now, ka, rk, rk_gate, rk_counts)
    w.out.turn(engine, w.PT, d_now, rk, rk_gate, OK, ws=w.ws)
    assert _u32(rk) == [NONE] * NP and w.out.read() == ([NONE] * NP, [REJ] * NP, [0] * NP, [0, 0])
    t_retry = t0 + 6 * SEC
    d_now.copy_(_clock(t_retry))
    ids1 = w.fresh(1)
    w.chain(d_now, _words(list(LISTED) + [7, 7, NONE]))  # a request for the live rows changes nothing; peer 7 starts
    second = w.snapshot()
    assert second[2] == ([0, 3, 5, 7] + [NONE] * 4, [OK] * 4 + [REJ] * 4, [0] * NP, [4, 0])
    t2 = second[0]
    assert [t2["timers"][p] for p in (0, 3, 5, 7)] == [(t0, t_retry)] * 3 + [(t_retry, t_retry)]
    assert [t2["hs_ids"][p] for p in (0, 3, 5, 7)] == ids1[:4] and pc.lookup(t2) == dict(zip(ids1[:4], (0, 3, 5, 7)))
    assert all(t2["pending"][p] != t1["pending"][p] for p in LISTED)

    def finish(responses, gate):
        keys_a, pidx, remote = _fill((NP, 64)), _fill((NP,), torch.int32), _fill((NP,), torch.int32)
        claim, st_fin, st_sess, rows_a = _fill((NP,), torch.int32), _fill((NP,)), _fill((NP,)), _fill((NP,), torch.int32)
        engine.handshake_finish_dev(w.a_own, w.a_peers, w.PT.pend_table, w.PT.pending, w.desc_r, gate,
                                    responses.reshape(-1), keys_a, pidx, remote, claim, st_fin)
        session.install_finish_batch_dev(engine, TA, st_fin, pidx, remote, w.PT.hs_ids, w.PT.peers, keys_a, st_sess,
                                         rows_a, now_ns=d_now)
        timers.arm_batch_dev(engine, tm_a, rows_a, st_sess, d_now, tc.REKEY_NS)
        torch.cuda.synchronize()
        return _u8(st_fin), _u32(pidx), _u8(st_sess), _u32(rows_a)

    st_fin, pidx, st_sess, rows_a = finish(resp0, gate0)  # the first attempt's answers: their ids are gone
    assert st_fin == [REJ] * NP and pidx == [NONE] * NP and st_sess == [REJ] * NP and rows_a == [NONE] * NP
    assert get_table(w.PT) == t2

    # ---- part 2: peers 0 and 3 answer the second attempt; peer 5's answer is lost
    resp1, gate1, keys_b = w.respond((0, 3), 1)
    st_fin, pidx, st_sess, rows_a = finish(resp1, gate1)
    assert st_fin == [OK, OK] + [REJ] * 6 and pidx == [0, 3] + [NONE] * 6
    assert st_sess == [OK, OK] + [REJ] * 6 and rows_a == [8, 9] + [NONE] * 6
    t3 = get_table(w.PT)
    assert t3["pending"][0] == t3["pending"][3] == pc.EMPTY and pc.is_live(t3, 5) and pc.is_live(t3, 7)
    assert t3["hs_ids"] == t2["hs_ids"] and t3["timers"] == t2["timers"]  # the wipe is all that ends a row
    assert _u32(TA.peer_slot) == [8, 1, 2, 9, 4, 5, 6, 7] and _u32(TA.local_ids)[8:10] == [ids1[0], ids1[1]]
    send_a, recv_a = TA.send_keys.cpu().numpy(), TA.recv_keys.cpu().numpy()
    for k, p in enumerate((0, 3)):
        kb = keys_b[p].cpu().numpy()[k]
        assert send_a[8 + k].tobytes() == kb[32:].tobytes() != bytes(32) and recv_a[8 + k].tobytes() == kb[:32].tobytes()
    tma = tm_a.cpu().numpy().view(np.uint64).reshape(NK, 2)
    assert [int(x) for x in tma[8:10, 0]] == [t_retry + tc.REKEY_NS] * 2

    # ---- 91 s past the last attempt: the abandoned rows are reaped, and a request starts them afresh
    d_now.copy_(_clock(t_retry + 91 * SEC))
    w.out.turn(engine, w.PT, d_now, ws=w.ws)
    assert w.out.read() == ([NONE] * NP, [REJ] * NP, [0, 0, 0, 0, 0, 1, 0, 1], [0, 2])
    t4 = get_table(w.PT)
    assert t4["pending"] == [pc.EMPTY] * NP and t4["hs_ids"] == t2["hs_ids"]
    # an expired row's timers are cleared; a finished row's are left as they were and mean nothing
    assert t4["timers"] == [(t0, t_retry) if p in (0, 3) else (0, 0) for p in range(NP)]
    assert _u32(w.PT.pend_table) == [NONE] * (2 * w.PT.pend_cap)


def test_turn_chain_and_install_captured(engine):
    """turn -> cookies -> initiate -> mac1 -> install captured once and replayed at two clocks, against the same
    calls uncaptured from the same start: at the first clock two requested peers start, 6 s later they retry"""
    w = World(engine, 2033)
    t0 = 40 * SEC
    d_now, req = _clock(t0), _words([6, 2, NONE, 6])
    w.fresh(0)
    start = [t.clone() for t in (w.PT.pending, w.PT.timers, w.PT.hs_ids, w.PT.pend_table, w.state_a)]

    def reset():
        for dst, src in zip((w.PT.pending, w.PT.timers, w.PT.hs_ids, w.PT.pend_table, w.state_a), start):
            dst.copy_(src)
        for t_ in (w.batch, w.cookies, w.has_cookie, w.st_init, w.st_inst):
            t_.fill_(FILL)
        w.msgs.zero_()

    want = []
    for now in (t0, t0 + 6 * SEC):
        d_now.copy_(_clock(now))
        w.chain(d_now, req)
        want.append(w.snapshot())
    assert want[0][2] == ([2, 6] + [NONE] * 6, [OK] * 2 + [REJ] * 6, [0] * NP, [2, 0]) and want[1][2] == want[0][2]
    assert [want[1][0]["timers"][p] for p in (2, 6)] == [(t0, t0 + 6 * SEC)] * 2
    reset()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        w.chain(d_now, req, stream=s)
    torch.cuda.synchronize()
    reset()  # whatever the capture did or did not run
    for k, now in enumerate((t0, t0 + 6 * SEC)):
        d_now.copy_(_clock(now))
        g.replay()
        got = w.snapshot()
        for name, a, b in zip(("tables", "pend_table", "outputs", "initiate status", "install status", "installed_out",
                               "batch", "messages", "peer state"), got, want[k]):
            assert a == b, (name, k)
