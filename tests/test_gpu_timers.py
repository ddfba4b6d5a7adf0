"""The device-resident session timers on the GPU (rg_timer_arm_batch_dev, rg_timer_note_send_batch_dev,
rg_timer_note_recv_batch_dev, rg_timer_turn_dev) against the in-order Python model (tests/timer_cases.py), and
between the calls they were made to join: install -> arm, receive -> note -> turn -> the padded keepalive send, the
turn's rekey list through the initiator chain, expiry.  Every output array over its full length and every byte of
the timers and of the tables the turn reads are compared."""
import ctypes

import numpy as np
import pytest

import handshake_cases as hc
import route_cases as rc
import timer_cases as tc
from conftest import load_golden
from rustyguard_amd import aead, route, session, timers
from rustyguard_amd.workloads import DESC_DTYPE

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL = 0xA5
GUARD = 0xA5A5A5A5
NOW = 10**12
OK, REJ, SKIP, NONE = tc.OK, tc.REJECTED, tc.SKIP, tc.NONE
SIZES = (1, 63, 64, 65, 2047, 2049, 4099)


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


def put_timers(tm):
    """(rekey_at_ns, flags, pad) rows -> uint8 [nkeys][16] on the device"""
    a = np.array([(at, flags | (pad << 32)) for at, flags, pad in tm], np.uint64).reshape(len(tm), 2)
    return _dev(a.view(np.uint8).reshape(len(tm), 16))


def get_timers(d):
    a = d.cpu().numpy().view(np.uint64).reshape(-1, 2)
    return [(int(at), int(w) & 0xFFFFFFFF, int(w) >> 32) for at, w in a]


def put_tables(engine, t):
    """the arrays the timer calls read (slot_peer, send_state, peer_slot) on the device, the others empty"""
    nkeys, npeers = len(t["slot_peer"]), len(t["peer_slot"])
    T = session.SessionTables(engine, nkeys, npeers)
    T.send_state[:] = _dev(np.array(t["send_state"], np.uint64).reshape(nkeys, 3).view(np.uint8).reshape(nkeys, 24))
    T.slot_peer[:] = _words(t["slot_peer"])
    T.peer_slot[:] = _words(t["peer_slot"])
    return T


def get_state(T):
    return [tuple(int(x) for x in r) for r in T.send_state.cpu().numpy().view(np.uint64).reshape(-1, 3)]


def check_read_only(T, t):
    _same("send_state", get_state(T), [tuple(s) for s in t["send_state"]])
    _same("slot_peer", _u32(T.slot_peer), t["slot_peer"])
    _same("peer_slot", _u32(T.peer_slot), t["peer_slot"])


class Outputs:
    """the turn's four output arrays with a guard entry behind each"""

    def __init__(self, npeers):
        self.npeers = npeers
        self.ka, self.rk = _fill((npeers + 1,), torch.int32), _fill((npeers + 1,), torch.int32)
        self.gate, self.counts = _fill((npeers + 1,)), _fill((3,), torch.int32)

    def turn(self, engine, T, d_timers, d_now, ws=None, stream=None):
        p = self.npeers
        return timers.turn_dev(engine, T, d_timers, d_now, self.ka[:p], self.rk[:p], self.gate[:p], self.counts[:2],
                               workspace=ws, stream=stream)

    def read(self):
        torch.cuda.synchronize()
        p = self.npeers
        ka, rk, gate, counts = _u32(self.ka), _u32(self.rk), _u8(self.gate), _u32(self.counts)
        assert ka[p] == GUARD and rk[p] == GUARD and gate[p] == FILL and counts[2] == GUARD
        return ka[:p], rk[:p], gate[:p], counts[:2]


def turn_vs_model(engine, t, tm, now):
    """one turn over the model's table -> (the model's result, the device arrays): every output and every byte of
    timers against the model, the tables unchanged"""
    T, d_timers, out = put_tables(engine, t), put_timers(tm), Outputs(len(t["peer_slot"]))
    out.turn(engine, T, d_timers, _clock(now))
    want = tc.turn_loop(t, tm, now)
    for name, g, w in zip(("ka_slots_out", "rekey_peers_out", "rekey_gate_out", "counts_out"), out.read(), want[1:]):
        _same(name, g, w)
    _same("timers", get_timers(d_timers), want[0])
    check_read_only(T, t)
    return want, T, d_timers, out


# -------------------------------------------------------------------- turn
@pytest.mark.parametrize("nkeys", SIZES)
def test_turn_sizes_against_the_model(engine, nkeys):
    """nkeys and npeers independently over a wave edge, a scan-tile edge and two carries; random live and free rows,
    times from one below, at and one above each deadline, counters from the edge values"""
    for npeers in SIZES:
        t, tm = tc.random_case(nkeys, npeers, 1000 * nkeys + npeers, NOW)
        want = turn_vs_model(engine, t, tm, NOW)[0]
        if nkeys >= 2047 and npeers >= 63:
            assert want[4][0] > 0 and want[4][1] > 0


def test_turn_few_peers_and_one_row_per_peer(engine):
    """4099 rows on 3 peers: every row of a peer stores the same want word; then one row per peer, all due: the
    lists are full and nothing is padding"""
    t, tm = tc.due_case(4099, 3, 0.5, NOW)
    want = turn_vs_model(engine, t, tm, NOW)[0]
    assert want[1:] == ([4098, 4096, 4097], [0, 1, 2], [OK] * 3, [3, 3])
    t, tm = tc.due_case(4099, 4099, 1.0, NOW)
    want = turn_vs_model(engine, t, tm, NOW)[0]
    assert want[1] == list(range(4099)) and want[2] == list(range(4099)) and want[4] == [4099, 4099]


def test_turn_same_clock_twice_and_padding(engine):
    """the lists are padded with RG_KEY_SKIP / RG_PEER_NONE and the gate with RG_PKT_REJECTED over the full npeers;
    a second turn at the same clock returns empty lists and changes no byte"""
    t, tm = tc.random_case(2049, 2049, 77, NOW)
    want, T, d_timers, out = turn_vs_model(engine, t, tm, NOW)
    nka, nrk = want[4]
    assert 0 < nka < 2049 and 0 < nrk < 2049
    assert want[1][nka:] == [SKIP] * (2049 - nka) and SKIP not in want[1][:nka]
    assert want[2][nrk:] == [NONE] * (2049 - nrk) and want[2][:nrk] == sorted(want[2][:nrk])
    assert want[3] == [OK] * nrk + [REJ] * (2049 - nrk)
    out.turn(engine, T, d_timers, _clock(NOW))
    assert out.read() == ([SKIP] * 2049, [NONE] * 2049, [REJ] * 2049, [0, 0])
    _same("timers", get_timers(d_timers), want[0])
    check_read_only(T, t)
    assert tc.turn_loop(t, want[0], NOW)[0] == want[0]
    # no peers: the counts alone, no row touched
    t0 = tc.tables([(NONE, 0, 0, 0), (5, 0, 5, 5)], [])
    want0 = turn_vs_model(engine, t0, [(1, 1, 0)] * 2, NOW)[0]
    assert want0 == ([(1, 1, 0)] * 2, [], [], [], [0, 0])


# ------------------------------------------------------------------- notes
def test_arm_and_note_calls_against_the_model(engine):
    """duplicates of one row within a batch (every lane stores the same value, the flag is an atomicOr), statuses
    that are not RG_PKT_OK, RG_KEY_SKIP and rows past the table; the arrays the calls read keep their bytes"""
    nkeys, n = 65, 4099
    t, tm = tc.random_case(nkeys, 7, 9, NOW)
    rows, status, rekey = tc.note_batch(nkeys, n, 10)
    assert max(rows.count(r) for r in set(rows) if r < nkeys) > 400 and SKIP in rows
    d_rows, d_status, d_rekey = _words(rows), _dev(np.array(status, np.uint8)), _dev(np.array(rekey, np.uint8))
    T, d_now = put_tables(engine, t), _clock(NOW)

    d = put_timers(tm)
    timers.arm_batch_dev(engine, d, d_rows, d_status, d_now, tc.REKEY_NS)
    _same("arm", get_timers(d), tc.arm_loop(tm, rows, status, NOW, tc.REKEY_NS))
    timers.arm_batch_dev(engine, d, d_rows, None, None, 0)  # no gate, no clock: a responder's sessions
    want = tc.arm_loop(tc.arm_loop(tm, rows, status, NOW, tc.REKEY_NS), rows, None, NOW, 0)
    _same("arm 0", get_timers(d), want)
    assert [want[r] for r in sorted(set(rows)) if r < nkeys] == [(0, 0, 0)] * len({r for r in rows if r < nkeys})

    d = put_timers(tm)
    timers.note_send_batch_dev(engine, d, d_rows, d_status, d_rekey, d_now)
    want = tc.note_send_loop(tm, rows, status, rekey, NOW)
    _same("note_send", get_timers(d), want)
    assert 0 < sum(a != b for a, b in zip(tm, want)) < nkeys
    timers.note_send_batch_dev(engine, d, d_rows, d_status, d_rekey, _clock(0))  # a clock of 0 arms nothing
    _same("note_send 0", get_timers(d), tc.note_send_loop(want, rows, status, rekey, 0))

    d = put_timers(tm)
    timers.note_recv_batch_dev(engine, d, T.send_state, d_rows, d_status, d_now)
    want = tc.note_recv_loop(tm, t["send_state"], rows, status, NOW)
    _same("note_recv", get_timers(d), want)
    assert 0 < sum(a != b for a, b in zip(tm, want)) < nkeys
    check_read_only(T, t)
    assert _u32(d_rows) == rows and _u8(d_status) == status and _u8(d_rekey) == rekey


# ------------------------------------------------------------------ capture
def test_note_turn_and_send_captured(engine):
    """note_recv -> turn -> the padded keepalive send on one stream, captured into a graph and replayed with the
    clock word changed between replays: at +5 s nothing is due, at +11 s rows 0 and 2 are flagged and their peers'
    current rows send (sent_ns moves), at +121 s they are silent again and row 1's rekey entry fires"""
    t0 = 7 * 10**9
    rows = [(0, 0, t0, t0), (1, 0, t0, t0), (2, 0, t0, t0), (2, 0, t0 - 9, t0 - 9), (NONE, 0, 0, 0)]
    t = tc.tables(rows, [0, 1, 2])
    tm = [(0, 0, 0), (t0 + tc.REKEY_NS, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)]
    nkeys, npeers = 5, 3
    T, d_timers, out = put_tables(engine, t), put_timers(tm), Outputs(npeers)
    T.send_keys[:] = _dev(np.random.default_rng(4).integers(0, 256, (nkeys, 32), dtype=np.uint8))
    T.receivers[:] = _words([0x900 + r for r in range(nkeys)])
    seen, seen_st = _words([0, 3, 2, 3, SKIP, 9]), _dev(np.array([OK, OK, OK, REJ, OK, OK], np.uint8))
    desc = _dev(np.array([(32 * k, 0, 0) for k in range(npeers)], DESC_DTYPE).view(np.uint8).reshape(-1, 16))
    buf, st, d_now = torch.zeros(32 * npeers, dtype=torch.uint8, device="cuda"), _fill((npeers,)), _clock(t0)
    ws_t, ws_s = timers.timer_workspace(engine, nkeys, npeers), engine.send_workspace(npeers, nkeys)
    skip = _words([SKIP] * npeers)
    engine.send_batch_dev_resident(T.send_keys, T.receivers, T.send_state, skip, desc, buf, st, now_ns=d_now,
                                   workspace=ws_s)  # the shape once, outside the capture; it takes no counter
    torch.cuda.synchronize()
    check_read_only(T, t)
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        timers.note_recv_batch_dev(engine, d_timers, T.send_state, seen, seen_st, d_now, stream=s)
        out.turn(engine, T, d_timers, d_now, ws=ws_t, stream=s)
        engine.send_batch_dev_resident(T.send_keys, T.receivers, T.send_state, out.ka[:npeers], desc, buf, st,
                                       now_ns=d_now, workspace=ws_s, stream=s)
    torch.cuda.synchronize()
    T.send_state[:] = put_tables(engine, t).send_state  # whatever the capture did or did not run
    d_timers.copy_(put_timers(tm))
    state, model = [tuple(r[1:]) for r in rows], tm
    expect = {5: ([SKIP] * 3, [NONE] * 3, [0, 0]), 11: ([0, 2, SKIP], [NONE] * 3, [2, 0]),
              121: ([0, 2, SKIP], [1, NONE, NONE], [2, 1])}
    for secs, (ka, rk, counts) in expect.items():
        now = t0 + secs * 10**9
        d_now.copy_(_clock(now))
        g.replay()
        torch.cuda.synchronize()
        cur = dict(t, send_state=state)
        model = tc.note_recv_loop(model, state, _u32(seen), _u8(seen_st), now)
        model, w_ka, w_rk, w_gate, w_counts = tc.turn_loop(cur, model, now)
        assert (w_ka, w_rk, w_counts) == (ka, rk, counts), secs
        for name, got, want in zip(("ka_slots_out", "rekey_peers_out", "rekey_gate_out", "counts_out"), out.read(),
                                   (w_ka, w_rk, w_gate, w_counts)):
            _same(f"{name} at +{secs} s", got, want)
        _same("timers", get_timers(d_timers), model)
        state = [(c + 1, started, now) if r in ka else (c, started, sent) for r, (c, started, sent) in enumerate(state)]
        _same("send_state", get_state(T), state)
        assert _u8(st) == [OK] * counts[0] + [REJ] * (npeers - counts[0]), secs
    frames = buf.cpu().numpy().reshape(npeers, 32)
    assert frames[0, :16].tobytes() == (4).to_bytes(4, "little") + (0x900).to_bytes(4, "little") + (1).to_bytes(8, "little")


# --------------------------------------------------------------- end to end
def test_keepalive_rekey_and_expiry_gpu_to_gpu(engine):
    """A initiates to B with the recorded keys of golden/handshake_full.json; both install and arm.  After 11 s of
    silence from B, A's data makes B owe a keepalive: note_recv -> turn -> the padded send, which A opens as an
    empty packet.  At +121 s A's turn lists B for a rekey; the list goes through the initiator chain and the
    responder calls as it is, and the second session becomes both ends' current row.  At +181 s the first session
    expires and a stale entry on its row lists nothing."""
    g = load_golden("handshake_full.json")["handshake"]
    rng = np.random.default_rng(2031)
    rb = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
    sk_a, sk_b, psk = (bytes.fromhex(g[k]) for k in ("static_private_i", "static_private_r", "preshared_key"))
    pk_a, pk_b = hc.pubkey(sk_a), hc.pubkey(sk_b)
    other = [hc.pubkey(rb(32)) for _ in range(3)]
    peers_a = hc.peer_rows([(pk_b, psk, hc.mac1_key(pk_b)), (other[2], rb(32), hc.mac1_key(other[2]))])
    rows_b = hc.peer_rows([(other[0], rb(32), hc.mac1_key(other[0])), (other[1], rb(32), hc.mac1_key(other[1])),
                           (pk_a, psk, hc.mac1_key(pk_a))])
    NA, NB, NK = 2, 3, 4  # A's peers (B is 0), B's peers (A is 2), rows of both tables
    table_a = _dev(route.build_table([("10.9.0.0/24", 0)]))
    table_b = _dev(route.build_table([("10.0.0.0/16", 2)]))
    TA, TB = session.SessionTables(engine, NK, NA), session.SessionTables(engine, NK, NB)
    tm_a, tm_b = timers.timer_rows(engine, NK), timers.timer_rows(engine, NK)
    tm_a.fill_(FILL), tm_b.fill_(FILL)  # stale rows: the arm behind the install clears them
    out_a, out_b = Outputs(NA), Outputs(NB)
    a_own, a_peers = _dev(np.frombuffer(sk_a + pk_a, np.uint8)), _dev(peers_a)
    b_own, b_peers, b_ptable = _dev(np.frombuffer(sk_b + pk_b, np.uint8)), _dev(rows_b), _dev(aead.peer_table(rows_b))
    state_a = torch.zeros((NA, 64), dtype=torch.uint8, device="cuda")  # rg_hs_peer_state
    t0 = 5 * 10**9
    d_now = _clock(t0)
    ts = bytes.fromhex(g["timestamp"])

    def handshake(peer_idx, gate, esk_a, esk_b, sid_a, sid_b):
        """n rows of the initiator chain on A, the responder calls on B, finish on A; install and arm on both.
        -> (statuses of the eight calls, A's rows, B's rows)"""
        n = len(sid_a)
        d_sid_a, d_sid_b = _words(sid_a), _words(sid_b)
        desc_i = _dev(np.array([(160 * i, 148, 0) for i in range(n)], DESC_DTYPE).view(np.uint8).reshape(-1, 16))
        desc_r = _dev(np.array([(96 * i, 92, 0) for i in range(n)], DESC_DTYPE).view(np.uint8).reshape(-1, 16))
        msgs, pending = torch.zeros((n, 160), dtype=torch.uint8, device="cuda"), _fill((n, 128))
        results, responses, keys_b, keys_a = _fill((n, 128)), _fill((n, 96)), _fill((n, 64)), _fill((n, 64))
        cookies, has_cookie, claim_a = _fill((n, 16)), _fill((n,)), _fill((NA,), torch.int32)
        st = [_fill((n,)) for _ in range(6)]
        pidx, remote, claim = (_fill((n,), torch.int32) for _ in range(3))
        rows_a, rows_bt = _fill((n,), torch.int32), _fill((n,), torch.int32)
        pend_table = _dev(aead.pending_table(np.array(sid_a, np.uint32)))
        d_ts = _dev(np.frombuffer(ts * n, np.uint8).reshape(n, 12))
        engine.peer_cookies_dev(state_a, peer_idx, cookies, has_cookie)
        engine.handshake_initiate_dev(a_own, a_peers, peer_idx, gate, _dev(esk_a), d_ts, d_sid_a, cookies, has_cookie,
                                      msgs, pending, st[0])
        engine.peer_mac1_dev(state_a, peer_idx, st[0], msgs, 160, 116, claim_a)
        engine.handshake_init_dev(b_own, b_peers, b_ptable, desc_i, st[0], msgs, results, st[1])
        engine.handshake_resp_dev(b_peers, results, st[1], _dev(esk_b), d_sid_b, None, None, responses, keys_b, st[2])
        session.install_resp_batch_dev(engine, TB, st[2], d_sid_b, results, keys_b, st[3], rows_bt, now_ns=d_now)
        timers.arm_batch_dev(engine, tm_b, rows_bt, st[3], None, 0)
        engine.handshake_finish_dev(a_own, a_peers, pend_table, pending, desc_r, st[2], responses, keys_a, pidx, remote,
                                    claim, st[4])
        session.install_finish_batch_dev(engine, TA, st[4], pidx, remote, d_sid_a, peer_idx, keys_a, st[5], rows_a,
                                         now_ns=d_now)
        timers.arm_batch_dev(engine, tm_a, rows_a, st[5], d_now, tc.REKEY_NS)
        torch.cuda.synchronize()
        mac1 = msgs.cpu().numpy()[0, 116:132].tobytes()
        assert state_a.cpu().numpy()[0, 32:48].tobytes() == mac1 != bytes(16)  # last_sent_mac1 of peer 0
        return [_u8(s) for s in st], _u32(rows_a), _u32(rows_bt)

    esk = lambda first, n: np.frombuffer(first + rb(32 * (n - 1)), np.uint8).reshape(n, 32)  # noqa: E731
    # ---- finish -> install -> arm
    st, rows_a, rows_bt = handshake(_words([0]), None, esk(bytes.fromhex(g["esk_i"]), 1), esk(bytes.fromhex(g["esk_r"]), 1),
                                    [0x0A10], [0x0B07])
    assert st == [[OK]] * 6 and rows_a == [0] and rows_bt == [0]
    assert TA.send_keys.cpu().numpy()[0].tobytes() == bytes.fromhex(g["transport_k1"])
    assert get_timers(tm_a)[0] == (t0 + tc.REKEY_NS, 0, 0) and get_timers(tm_b)[0] == (0, 0, 0)
    assert get_timers(tm_a)[1] == (0xA5A5A5A5A5A5A5A5, GUARD, GUARD)  # the other rows are the caller's
    tm_a[1:].zero_(), tm_b[1:].zero_()

    # ---- +11 s: A -> B data, B owes a keepalive
    t1 = t0 + 11 * 10**9
    d_now.copy_(_clock(t1))
    pkt = rc.ipv4(64, rc.ip(10, 0, 0, 1), rc.ip(10, 9, 0, 7), rng)
    data = np.zeros(96, np.uint8)
    data[16:80] = pkt
    d_data = _dev(data)
    d_desc = _dev(np.array([(0, 64, 0)], DESC_DTYPE).view(np.uint8).reshape(-1, 16))
    slots, desc_out, st1, st2, rekey = _fill((1,), torch.int32), _fill((1, 16)), _fill((1,)), _fill((1,)), _fill((1,))
    route.route_batch_dev(engine, table_a, TA.peer_slot, d_desc, d_data, slots, desc_out, st1)
    engine.send_batch_dev_resident(TA.send_keys, TA.receivers, TA.send_state, slots, desc_out, d_data, st2,
                                   rekey_out=rekey, now_ns=d_now)
    timers.note_send_batch_dev(engine, tm_a, slots, st2, rekey, d_now)
    wire = _dev(np.array([(0, 96, 0)], DESC_DTYPE).view(np.uint8).reshape(-1, 16))
    st3, key_idx, inner = _fill((1,)), _fill((1,), torch.int32), _fill((1,), torch.int32)
    engine.recv_batch_dev_resident(TB.recv_keys, TB.rx_table, TB.windows, wire, d_data, st3, key_idx_out=key_idx)
    timers.note_recv_batch_dev(engine, tm_b, TB.send_state, key_idx, st3, d_now)
    route.route_check_batch_dev(engine, table_b, TB.slot_peer, wire, key_idx, d_data, st3, inner)
    out_b.turn(engine, TB, tm_b, d_now)
    ka_desc = _dev(np.array([(32 * k, 0, 0) for k in range(NB)], DESC_DTYPE).view(np.uint8).reshape(-1, 16))
    ka_buf, st4 = torch.zeros(32 * NB, dtype=torch.uint8, device="cuda"), _fill((NB,))
    engine.send_batch_dev_resident(TB.send_keys, TB.receivers, TB.send_state, out_b.ka[:NB], ka_desc, ka_buf, st4,
                                   now_ns=d_now)
    torch.cuda.synchronize()
    assert _u8(st1) == _u8(st2) == _u8(st3) == [OK] and _u8(rekey) == [0] and _u32(inner) == [64]
    assert np.array_equal(d_data.cpu().numpy()[16:80], pkt)
    assert get_timers(tm_a)[0] == (t0 + tc.REKEY_NS, 0, 0)
    assert out_b.read() == ([0, SKIP, SKIP], [NONE] * 3, [REJ] * 3, [1, 0])
    assert get_timers(tm_b) == [(0, 0, 0)] * NK  # the flag was set and taken
    assert _u8(st4) == [OK, REJ, REJ] and get_state(TB)[0] == (1, t0, t1)
    assert not ka_buf.cpu().numpy()[32:].any()  # the padding rows' frames are untouched
    ka_wire = _dev(np.array([(32 * k, 32, 0) for k in range(NB)], DESC_DTYPE).view(np.uint8).reshape(-1, 16))
    st5, key_idx5, inner5 = _fill((NB,)), _fill((NB,), torch.int32), _fill((NB,), torch.int32)
    engine.recv_batch_dev_resident(TA.recv_keys, TA.rx_table, TA.windows, ka_wire, ka_buf, st5, key_idx_out=key_idx5)
    timers.note_recv_batch_dev(engine, tm_a, TA.send_state, key_idx5, st5, d_now)
    route.route_check_batch_dev(engine, table_a, TA.slot_peer, ka_wire, key_idx5, ka_buf, st5, inner5)
    out_a.turn(engine, TA, tm_a, d_now)
    torch.cuda.synchronize()
    assert _u8(st5)[0] == OK and OK not in _u8(st5)[1:] and _u32(key_idx5)[0] == 0 and _u32(inner5) == [0] * NB
    assert out_a.read() == ([SKIP] * 2, [NONE] * 2, [REJ] * 2, [0, 0])  # A sent a second ago and is not yet due
    assert get_timers(tm_a)[0] == (t0 + tc.REKEY_NS, 0, 0)

    # ---- +121 s: A's turn lists B; the list through the initiator chain and the responder calls
    t2 = t0 + 121 * 10**9
    d_now.copy_(_clock(t2))
    out_a.turn(engine, TA, tm_a, d_now)
    assert out_a.read() == ([SKIP] * 2, [0, NONE], [OK, REJ], [0, 1])
    assert get_timers(tm_a)[0] == (0, 0, 0)
    st, rows_a, rows_bt = handshake(out_a.rk[:NA], out_a.gate[:NA], esk(rb(32), NA), esk(rb(32), NA), [0x0A25, 0x0A3A],
                                    [0x0B19, 0x0B2B])
    assert st == [[OK, REJ]] * 6 and rows_a == [1, SKIP] and rows_bt == [1, SKIP]
    assert _u32(TA.peer_slot) == [1, SKIP] and _u32(TB.peer_slot) == [SKIP, SKIP, 1]
    assert _u32(TA.slot_peer) == [0, 0, NONE, NONE] and _u32(TB.slot_peer) == [2, 2, NONE, NONE]
    assert get_timers(tm_a)[:2] == [(0, 0, 0), (t2 + tc.REKEY_NS, 0, 0)] and get_state(TA)[1] == (0, t2, t2)
    assert TA.send_keys.cpu().numpy()[1].tobytes() == TB.recv_keys.cpu().numpy()[1].tobytes() != bytes(32)

    # ---- +181 s: the first session expires; a stale entry on its row lists nothing
    t3 = t0 + 181 * 10**9
    d_now.copy_(_clock(t3))
    timers.note_send_batch_dev(engine, tm_a, _words([0]), _dev(np.array([OK], np.uint8)), _dev(np.array([1], np.uint8)),
                               d_now)
    expired = _fill((NK,))
    session.expire_batch_dev(engine, TA, d_now, None, expired)
    d_now.copy_(_clock(t3 + 1))
    out_a.turn(engine, TA, tm_a, d_now)
    assert _u8(expired) == [1, 0, 0, 0] and _u32(TA.slot_peer) == [NONE, 0, NONE, NONE] and _u32(TA.peer_slot) == [1, SKIP]
    assert out_a.read() == ([SKIP] * 2, [NONE] * 2, [REJ] * 2, [0, 0])
    assert get_timers(tm_a)[:2] == [(t3, 0, 0), (t2 + tc.REKEY_NS, 0, 0)]  # a free row is not touched


# ------------------------------------------------------------------ refusals
def test_timer_argument_refusals(engine):
    """n == 0 is RG_OK; a null required pointer, n = 2^32, a misaligned array and a short workspace are RG_EINVAL
    with the call named, and nothing is enqueued: every array keeps its fill"""
    L, h = engine.library, engine.handle
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    n, nkeys, npeers = 4, 4, 2
    T = session.SessionTables(engine, nkeys, npeers)
    for name in session.ARRAYS:
        getattr(T, name).fill_(FILL if getattr(T, name).dtype == torch.uint8 else GUARD - (1 << 32))
    tm, rows, st, rk, now = _fill((nkeys + 1, 16)), _fill((n + 1,), torch.int32), _fill((n,)), _fill((n,)), _fill((16,))
    ka, rkp, gate, counts = _fill((npeers + 1,), torch.int32), _fill((npeers + 1,), torch.int32), _fill((npeers,)), \
        _fill((3,), torch.int32)
    need = int(L.rg_timer_workspace_size(nkeys, npeers))
    ws = _fill((need + 16,))

    def arm(tm_=p(tm), rows_=p(rows), n_=n, now_=p(now), after=5):
        return L.rg_timer_arm_batch_dev(h, tm_, nkeys, rows_, None, n_, now_, after, s)

    def note_send(tm_=p(tm), rows_=p(rows), st_=p(st), rk_=p(rk), n_=n, now_=p(now)):
        return L.rg_timer_note_send_batch_dev(h, tm_, nkeys, rows_, st_, rk_, n_, now_, s)

    def note_recv(tm_=p(tm), ss=p(T.send_state), rows_=p(rows), st_=p(st), n_=n, now_=p(now)):
        return L.rg_timer_note_recv_batch_dev(h, tm_, ss, nkeys, rows_, st_, n_, now_, s)

    def turn(tables=None, tm_=p(tm), now_=p(now), ka_=p(ka), rkp_=p(rkp), gate_=p(gate), counts_=p(counts), ws_=p(ws),
             wl=need, **fields):
        t = T.struct()
        for k, v in fields.items():
            setattr(t, k, v)
        return L.rg_timer_turn_dev(h, None if tables == "null" else ctypes.byref(t), tm_, now_, ka_, rkp_, gate_, counts_,
                                   ws_, wl, s)

    assert arm(n_=0) == 0 and note_send(n_=0) == 0 and note_recv(n_=0) == 0
    common = (dict(tm_=None), dict(rows_=None), dict(now_=None), dict(n_=1 << 32), dict(tm_=p(tm, 4)), dict(rows_=p(rows, 2)),
              dict(now_=p(now, 4)))
    for call, name, more in ((arm, b"timer arm", ()), (note_send, b"timer note send", (dict(st_=None), dict(rk_=None))),
                             (note_recv, b"timer note recv", (dict(st_=None), dict(ss=None), dict(ss=p(T.send_state, 4))))):
        for bad in common + more:
            assert call(**bad) == -1, (name, bad)
            assert name in L.rg_last_error(), (name, bad)
    for bad in (dict(tables="null"), dict(tm_=None), dict(now_=None), dict(ka_=None), dict(rkp_=None), dict(gate_=None),
                dict(counts_=None), dict(ws_=None), dict(tm_=p(tm, 4)), dict(now_=p(now, 4)), dict(ka_=p(ka, 2)),
                dict(rkp_=p(rkp, 2)), dict(counts_=p(counts, 2)), dict(ws_=p(ws, 8)), dict(wl=need - 1), dict(wl=0),
                dict(slot_peer=None), dict(send_state=None), dict(peer_slot=None),
                dict(send_state=T.send_state.data_ptr() + 4), dict(slot_peer=T.slot_peer.data_ptr() + 2),
                dict(peer_slot=T.peer_slot.data_ptr() + 2)):
        assert turn(**bad) == -1, bad
        assert b"timer turn" in L.rg_last_error(), bad
    torch.cuda.synchronize()
    for t_ in (tm, st, rk, now, gate, ws) + tuple(getattr(T, name) for name in session.ARRAYS
                                                   if getattr(T, name).dtype == torch.uint8):
        assert (t_.cpu().numpy() == FILL).all()
    for t_ in (rows, ka, rkp, counts, T.receivers, T.local_ids, T.slot_peer, T.rx_table, T.peer_slot):
        assert all(x == GUARD for x in _u32(t_))
