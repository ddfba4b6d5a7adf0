"""The device-resident session table on the GPU (rg_session_install_batch_dev and its two wrappers,
rg_session_expire_batch_dev, rg_session_index_dev) against the in-order Python model (tests/session_cases.py) and
between the handshake calls and the resident transport calls it was made to join.  Every output array and every
table array is compared byte for byte; the receiver table is compared through its lookup."""
import ctypes

import numpy as np
import pytest

import handshake_cases as hc
import route_cases as rc
import session_cases as sc
from conftest import load_golden
from oracle import oracle
from rustyguard_amd import aead, route, session
from rustyguard_amd.workloads import DESC_DTYPE

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL = 0xA5
GUARD = 0xA5A5A5A5


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _words(values):
    """uint32 values -> a device tensor (int32 holding the same bits)"""
    return _dev(np.array(values, np.uint32).view(np.int32))


def _fill(shape, dtype=torch.uint8):
    if dtype == torch.uint8:
        return torch.full(shape, FILL, dtype=dtype, device="cuda")
    return torch.full(shape, GUARD - (1 << 32), dtype=torch.int32, device="cuda")  # the same bytes


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _same(name, got, want):
    assert len(got) == len(want), name
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (name, len(bad), bad[:8], [(got[i], want[i]) for i in bad[:2]])


def upload(engine, t, rx_cap=None):
    """the model's table on the device, its receiver table built by rg_session_index_dev as for a caller that
    seeded the rows itself"""
    nkeys, npeers = len(t["slot_peer"]), len(t["peer_slot"])
    T = session.SessionTables(engine, nkeys, npeers, rx_cap)
    if nkeys:
        T.send_keys[:] = _dev(np.frombuffer(b"".join(t["send_keys"]), np.uint8).reshape(nkeys, 32))
        T.recv_keys[:] = _dev(np.frombuffer(b"".join(t["recv_keys"]), np.uint8).reshape(nkeys, 32))
        T.windows[:] = _dev(np.frombuffer(b"".join(t["windows"]), np.uint8).reshape(nkeys, sc.WINDOW))
        T.send_state[:] = _dev(np.array(t["send_state"], np.uint64).view(np.uint8).reshape(nkeys, 24))
        for name in ("receivers", "local_ids", "slot_peer"):
            getattr(T, name)[:] = _words(t[name])
    if npeers:
        T.peer_slot[:] = _words(t["peer_slot"])
    session.index_dev(engine, T)
    return T


def download(T):
    torch.cuda.synchronize()
    t = {name: [r.tobytes() for r in getattr(T, name).cpu().numpy()] for name in ("send_keys", "recv_keys", "windows")}
    t["send_state"] = [tuple(int(x) for x in r) for r in T.send_state.cpu().numpy().view(np.uint64).reshape(-1, 3)]
    for name in ("receivers", "local_ids", "slot_peer", "peer_slot"):
        t[name] = [int(x) for x in _u32(getattr(T, name))]
    return t


def check_tables(T, want, gone=(), never=(0xDEAD0001, 0, 0xFFFFFFFF, 0x7FFFFFFF)):
    """every array against the model; the receiver table through rg_rx_table_find: every live id finds its row,
    every id in `gone` and `never` finds none, and there is one occupied entry per live row"""
    got = download(T)
    for name in sc.ROW_ARRAYS + ("peer_slot",):
        _same(name, got[name], want[name])
    table = np.ascontiguousarray(_u32(T.rx_table).reshape(-1, 2))
    pairs = sc.rx_pairs(want)
    for lid, r in pairs.items():
        assert aead.rx_find(table, lid) == r, (hex(lid), r)
    for lid in list(gone) + list(never):
        if lid not in pairs:
            assert aead.rx_find(table, lid) == -1, hex(lid)
    assert int((table[:, 1] != sc.SKIP).sum()) == len(pairs)
    assert (table[table[:, 1] == sc.SKIP] == 0xFFFFFFFF).all()


def run_install(engine, T, b, now=None, gate=True, stream=None, ws=None):
    """one rg_session_install_batch_dev over the batch dict b -> (status, rows_out, key rows), guards checked"""
    n = len(b["local_ids"])
    st, rows, keys = _fill((n + 1,)), _fill((n + 1,), torch.int32), _fill((n + 1, 64))
    keys[:n] = _dev(np.frombuffer(b"".join(b["keys"]), np.uint8).reshape(n, 64))
    d_now = None if now is None else _dev(np.array([now], np.uint64).view(np.int64))
    session.install_batch_dev(engine, T, _dev(np.array(b["gate"], np.uint8)) if gate else None, _words(b["local_ids"]),
                              _words(b["remote_ids"]), _words(b["peers"]), keys[:n], st[:n], rows[:n], now_ns=d_now,
                              workspace=ws, stream=stream)
    torch.cuda.synchronize()
    s, r, k = st.cpu().numpy(), _u32(rows), keys.cpu().numpy()
    assert s[n] == FILL and r[n] == GUARD and (k[n] == FILL).all()
    return [int(x) for x in s[:n]], [int(x) for x in r[:n]], [x.tobytes() for x in k[:n]]


def install_vs_model(engine, t, b, now=None, gate=True, rx_cap=None):
    T = upload(engine, t, rx_cap)
    check_tables(T, t)  # the seeded table indexes as the model says
    got = run_install(engine, T, b, now, gate)
    want = sc.install_loop(t, b["gate"] if gate else None, b["local_ids"], b["remote_ids"], b["peers"], b["keys"], now)
    for name, g, w in zip(("status", "rows_out", "transport_keys"), got, want[1:]):
        _same(name, g, w)
    check_tables(T, want[0])
    return T, want


# ------------------------------------------------------------------ install
def test_install_every_rule_once(engine):
    """nkeys = 8, npeers = 4, n = 12 (session_cases.every_rule_case): gated rows between OK rows, a peer past the
    table, a duplicate of a live id, a duplicate whose first holder is itself RG_PKT_FULL, the free list running
    out mid-batch, two handshakes of one peer, two ids with one home slot"""
    t, b, now, status, rows_out, peer_slot = sc.every_rule_case()
    T, want = install_vs_model(engine, t, b, now)
    assert want[1] == status and want[2] == rows_out and want[0]["peer_slot"] == peer_slot
    # without a gate the gated rows are judged like any other
    install_vs_model(engine, t, b, now, gate=False)


def _edge(nkeys, npeers, live, n, seed):
    rng = np.random.default_rng(seed)
    t = sc.empty_tables(nkeys, npeers)
    for r in live:
        sc.seed_row(t, r, 0x600 + r, 0x700 + r, r % npeers, rng, started=3)
    rows = [(sc.OK, 0x800 + i, 0x900 + i, i % npeers) for i in range(n)]
    return t, sc.batch(rows, rng)


@pytest.mark.parametrize("name,nkeys,live,n,now", [
    ("nkeys_1", 1, (), 3, 5), ("no_free_row", 4, (0, 1, 2, 3), 3, 5), ("all_free", 5, (), 4, 5),
    ("n_1", 4, (1,), 1, 5), ("now_null", 4, (2,), 2, None)])
def test_install_edges(engine, name, nkeys, live, n, now):
    """nkeys = 1; a table with no free row; a table all free; n = 1; now_ns NULL"""
    t, b = _edge(nkeys, 2, live, n, 31)
    T, want = install_vs_model(engine, t, b, now)
    free = nkeys - len(live)
    assert want[1] == [sc.OK] * min(n, free) + [sc.FULL] * max(0, n - free)
    if name == "now_null":
        assert want[0]["send_state"][0] == (0, 0, 0) and want[0]["slot_peer"][0] == 0


def test_install_beyond_one_scan_tile(engine):
    """the scans run by tiles of 2048 rows (session_cases.TILE = kGroupTile): n = nkeys = 2 * 2048 + 3, every third
    row live and every third handshake not eligible, five more eligible handshakes than free rows"""
    assert sc.TILE == 2048
    n = nkeys = 2 * sc.TILE + 3
    t = sc.scattered_tables(nkeys, 5, 21, extra_live=(1, 2, 4, 5, 7))
    b = sc.scattered_batch(n, 5, 22)
    T, want = install_vs_model(engine, t, b, 7)
    assert want[1].count(sc.FULL) == 5 and want[1].count(sc.OK) == sum(p == sc.NONE for p in t["slot_peer"])


@pytest.mark.parametrize("n,nkeys", [(2 * sc.TILE + 3, sc.TILE - 5), (70, 2 * sc.TILE + 3)],
                         ids=["batch_3_tiles_table_1", "batch_1_tile_table_3"])
def test_install_batch_and_table_on_different_tile_counts(engine, n, nkeys):
    """the scan over the batch is bounded by n and the scan over the table by nkeys: three tiles of handshakes into
    one tile of rows (the free rows run out, most answers RG_PKT_FULL), and one tile of handshakes into three tiles
    of rows (the free list spans them, every eligible handshake gets a row)"""
    t = sc.scattered_tables(nkeys, 5, 23)
    b = sc.scattered_batch(n, 5, 24)
    T, want = install_vs_model(engine, t, b, 7)
    status, free = want[1], sum(p == sc.NONE for p in t["slot_peer"])
    dup = [i for i in range(0, n, 3) if (i // 3) % 4 == 3]  # the id of an earlier row of the batch
    assert dup and all(status[i] == sc.REJECTED for i in dup)
    eligible = n - len(range(0, n, 3))
    assert status.count(sc.OK) == min(free, eligible) > 0 and status.count(sc.FULL) == eligible - min(free, eligible)
    assert (status.count(sc.FULL) > n // 3) == (n > nkeys)


# ------------------------------------------------------------------- expiry
def test_expiry(engine):
    """started_ns + 180e9 == now stays, one below goes, a started_ns near 2^64 wraps; the list names a live row, a
    free row and indices >= nkeys; peer_slot is cleared only where it names the removed row; removed rows are
    zero; the next install takes the lowest freed rows"""
    t, now, rows, expired, peer_slot = sc.expiry_case()
    nkeys = len(expired)
    T = upload(engine, t)
    d_now, d_rows = _dev(np.array([now], np.uint64).view(np.int64)), _words(rows)
    out = _fill((nkeys + 1,))
    session.expire_batch_dev(engine, T, d_now, d_rows, out[:nkeys])
    want, want_exp = sc.expire_loop(t, now, rows)
    assert want_exp == expired and want["peer_slot"] == peer_slot
    torch.cuda.synchronize()
    assert [int(x) for x in out.cpu().numpy()] == expired + [FILL]
    gone = [t["local_ids"][r] for r in range(nkeys) if expired[r]]
    check_tables(T, want, gone=gone)
    for r in range(nkeys):
        if expired[r]:
            assert want["send_keys"][r] == bytes(32) and want["windows"][r] == bytes(264)
    b = sc.batch([(sc.OK, 0x900 + i, 1, i % 4) for i in range(3)], np.random.default_rng(5))
    got = run_install(engine, T, b, now)
    want2 = sc.install_loop(want, b["gate"], b["local_ids"], b["remote_ids"], b["peers"], b["keys"], now)
    assert got[1] == want2[2] == [1, 2, 3]
    check_tables(T, want2[0], gone=gone)
    # the list alone (now_ns NULL), no expired_out; then the clock alone
    T = upload(engine, t)
    session.expire_batch_dev(engine, T, None, d_rows, None)
    want, want_exp = sc.expire_loop(t, None, rows)
    assert want_exp == [0, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    check_tables(T, want, gone=[t["local_ids"][3]])
    session.expire_batch_dev(engine, T, d_now, None, out[:nkeys])
    want, want_exp = sc.expire_loop(want, now, ())
    torch.cuda.synchronize()
    assert [int(x) for x in out.cpu().numpy()[:nkeys]] == want_exp == [0, 1, 1, 0, 0, 0, 1, 0, 0, 0]
    check_tables(T, want, gone=gone)


# ------------------------------------------------------------------ capture
def test_install_then_expire_captured(engine):
    """install followed by expire on one stream, captured into a graph and replayed once with another *now_ns:
    the tables equal the model applied twice.  The first pass installs three sessions at now = 10^12 and expires
    nothing new; the replay at 10^12 + 200 s finds their ids live (every row REJECTED) and expires them all."""
    t, now, rows, _, _ = sc.expiry_case()
    nkeys = len(t["slot_peer"])
    b = sc.batch([(sc.OK, 0xA00 + i, 0xB00 + i, i % 4) for i in range(3)], np.random.default_rng(6))
    n = 3
    T = upload(engine, t)
    key_rows = _dev(np.frombuffer(b"".join(b["keys"]), np.uint8).reshape(n, 64))
    st, rows_out, keys, out = _fill((n,)), _fill((n,), torch.int32), _fill((n, 64)), _fill((nkeys,))
    d_now = _dev(np.array([now], np.uint64).view(np.int64))
    args = [_dev(np.array(b["gate"], np.uint8)), _words(b["local_ids"]), _words(b["remote_ids"]), _words(b["peers"])]
    ws = session.session_workspace(engine, n, nkeys, 4)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        session.install_batch_dev(engine, T, *args, keys, st, rows_out, now_ns=d_now, workspace=ws, stream=s)
        session.expire_batch_dev(engine, T, d_now, None, out, workspace=ws, stream=s)
    torch.cuda.synchronize()
    T2 = upload(engine, t)  # whatever the capture did or did not run, start from the case's table
    for name in session.ARRAYS:
        getattr(T, name).copy_(getattr(T2, name))
    model = t
    for k, clock in enumerate((now, now + 200 * 10**9)):
        keys.copy_(key_rows)
        d_now.copy_(_dev(np.array([clock], np.uint64).view(np.int64)))
        g.replay()
        torch.cuda.synchronize()
        m1 = sc.install_loop(model, b["gate"], b["local_ids"], b["remote_ids"], b["peers"], b["keys"], clock)
        model, want_exp = sc.expire_loop(m1[0], clock, ())
        assert [int(x) for x in st.cpu().numpy()] == m1[1] == ([sc.OK] * 3 if k == 0 else [sc.REJECTED] * 3)
        assert [int(x) for x in _u32(rows_out)] == m1[2]
        assert (keys.cpu().numpy() == 0).all()
        assert [int(x) for x in out.cpu().numpy()] == want_exp
        check_tables(T, model, gone=b["local_ids"] + t["local_ids"])
    assert sc.rx_pairs(model) == {} and sum(want_exp) == 6  # rows 0, 3 and 4 of the case and the three installed ones


# --------------------------------------------------------------- end to end
def _frames(rng, pairs):
    """IPv4 packets of 64 and 80 bytes, one frame of headroom each: (desc with the inner lengths, buf, plaintexts)"""
    desc, pkts, off = np.zeros(len(pairs), DESC_DTYPE), [], 0
    for i, (src, dst) in enumerate(pairs):
        L = (64, 80)[i % 2]
        pkts.append(rc.ipv4(L, src, dst, rng))
        desc[i] = (off, L, 0)
        off += 16 + L + 16
    buf = rng.integers(1, 256, off, dtype=np.uint8)
    for d, p in zip(desc, pkts):
        buf[int(d["offset"]) + 16:int(d["offset"]) + 16 + len(p)] = p
    return desc, buf, pkts


def _send(engine, T, table, desc, buf, now):
    n = len(desc)
    d_desc, d_buf = _dev(desc.view(np.uint8).reshape(-1, 16)), _dev(buf)
    slots, desc_out, st = _fill((n,), torch.int32), _fill((n, 16)), _fill((n,))
    route.route_batch_dev(engine, table, T.peer_slot, d_desc, d_buf, slots, desc_out, st)
    torch.cuda.synchronize()
    assert list(st.cpu().numpy()) == [sc.OK] * n
    st2 = _fill((n,))
    engine.send_batch_dev_resident(T.send_keys, T.receivers, T.send_state, slots, desc_out, d_buf, st2, now_ns=now)
    torch.cuda.synchronize()
    assert list(st2.cpu().numpy()) == [sc.OK] * n
    return [int(x) for x in _u32(slots)], d_buf


def _recv(engine, T, table, desc, d_buf):
    n = len(desc)
    wire = desc.copy()
    wire["len"] += 32
    d_wire = _dev(wire.view(np.uint8).reshape(-1, 16))
    st, key_idx, inner = _fill((n,)), _fill((n,), torch.int32), _fill((n,), torch.int32)
    engine.recv_batch_dev_resident(T.recv_keys, T.rx_table, T.windows, d_wire, d_buf, st, key_idx_out=key_idx)
    route.route_check_batch_dev(engine, table, T.slot_peer, d_wire, key_idx, d_buf, st, inner)
    torch.cuda.synchronize()
    return [int(x) for x in st.cpu().numpy()], [int(x) for x in _u32(key_idx)], [int(x) for x in _u32(inner)], wire


def test_handshake_to_transport_gpu_to_gpu(engine):
    """Three handshakes between A and B, the first with the recorded static, ephemeral and preshared keys of
    golden/handshake_full.json: initiate -> init -> resp -> install_resp on B's tables, finish -> install_finish
    on A's, one stream, the key rows never read back.  A's three peer rows are three tunnels to B; B knows A as
    its row 2.  Then A routes and sends two packets per tunnel, B receives and checks their sources; the first
    tunnel's frames also open under the recorded transport keys in the CPU oracle; then the reverse direction;
    then B's rows expire and the next frame of the same session is RG_PKT_REJECTED, its bytes untouched."""
    g = load_golden("handshake_full.json")["handshake"]
    rng = np.random.default_rng(2030)
    rb = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
    n = 3
    sk_a, sk_b, psk = (bytes.fromhex(g[k]) for k in ("static_private_i", "static_private_r", "preshared_key"))
    pk_a, pk_b = hc.pubkey(sk_a), hc.pubkey(sk_b)
    other = [hc.pubkey(rb(32)) for _ in range(2)]
    peers_a = hc.peer_rows([(pk_b, psk, hc.mac1_key(pk_b))] * n)
    rows_b = hc.peer_rows([(other[0], rb(32), hc.mac1_key(other[0])), (other[1], rb(32), hc.mac1_key(other[1])),
                           (pk_a, psk, hc.mac1_key(pk_a))])
    esk_a = np.frombuffer(bytes.fromhex(g["esk_i"]) + rb(64), np.uint8).reshape(n, 32)
    esk_b = np.frombuffer(bytes.fromhex(g["esk_r"]) + rb(64), np.uint8).reshape(n, 32)
    ts = np.frombuffer(bytes.fromhex(g["timestamp"]) * n, np.uint8).reshape(n, 12)
    sid_a = np.array([0x0A10, 0x0A25, 0x0A3A], np.uint32)
    sid_b = np.array([0x0B07, 0x0B19, 0x0B2B], np.uint32)
    desc_i = np.array([(160 * i, 148, 0) for i in range(n)], DESC_DTYPE)
    desc_r = np.array([(96 * i, 92, 0) for i in range(n)], DESC_DTYPE)
    # A: peer p owns 10.0.p.0/24; B: A (its peer 2) owns 10.0.0.0/16, B's own hosts are 10.9.0.0/16 behind A's peers
    table_a = _dev(route.build_table([("10.9.%d.0/24" % p, p) for p in range(n)]))
    table_b = _dev(route.build_table([("10.0.0.0/16", 2), ("10.7.0.0/16", 0)]))
    TA, TB = session.SessionTables(engine, 8, n), session.SessionTables(engine, 8, 3)
    now = 5 * 10**9
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a_own, a_peers = _dev(np.frombuffer(sk_a + pk_a, np.uint8)), _dev(peers_a)
        b_own, b_peers, b_ptable = _dev(np.frombuffer(sk_b + pk_b, np.uint8)), _dev(rows_b), _dev(aead.peer_table(rows_b))
        a_pidx, a_sid, b_sid = _words(np.arange(n)), _words(sid_a), _words(sid_b)
        a_pend_table = _dev(aead.pending_table(sid_a))
        d_desc_i, d_desc_r = _dev(desc_i.view(np.uint8).reshape(-1, 16)), _dev(desc_r.view(np.uint8).reshape(-1, 16))
        msgs, pending = torch.zeros((n, 160), dtype=torch.uint8, device="cuda"), _fill((n, 128))
        results, responses, keys_b, keys_a = _fill((n, 128)), _fill((n, 96)), _fill((n, 64)), _fill((n, 64))
        st = [_fill((n,)) for _ in range(6)]
        pidx, remote, claim = (_fill((n,), torch.int32) for _ in range(3))
        rows_a, rows_bt = _fill((n,), torch.int32), _fill((n,), torch.int32)
        d_now = _dev(np.array([now], np.uint64).view(np.int64))
        ws_a, ws_b = session.session_workspace(engine, n, 8, n), session.session_workspace(engine, n, 8, 3)
        d_esk_a, d_esk_b, d_ts = _dev(esk_a), _dev(esk_b), _dev(ts)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        engine.handshake_initiate_dev(a_own, a_peers, a_pidx, None, d_esk_a, d_ts, a_sid, None, None, msgs, pending, st[0],
                                      stream=s)
        engine.handshake_init_dev(b_own, b_peers, b_ptable, d_desc_i, st[0], msgs, results, st[1], stream=s)
        engine.handshake_resp_dev(b_peers, results, st[1], d_esk_b, b_sid, None, None, responses, keys_b, st[2], stream=s)
        session.install_resp_batch_dev(engine, TB, st[2], b_sid, results, keys_b, st[3], rows_bt, now_ns=d_now,
                                       workspace=ws_b, stream=s)
        engine.handshake_finish_dev(a_own, a_peers, a_pend_table, pending, d_desc_r, st[2], responses, keys_a, pidx,
                                    remote, claim, st[4], stream=s)
        session.install_finish_batch_dev(engine, TA, st[4], pidx, remote, a_sid, a_pidx, keys_a, st[5], rows_a,
                                         now_ns=d_now, workspace=ws_a, stream=s)
    s.synchronize()
    for t_ in st:
        assert list(t_.cpu().numpy()) == [sc.OK] * n
    assert (keys_a.cpu().numpy() == 0).all() and (keys_b.cpu().numpy() == 0).all()  # consumed on the device
    assert list(_u32(rows_a)) == [0, 1, 2] and list(_u32(rows_bt)) == [0, 1, 2]
    k1, k2 = bytes.fromhex(g["transport_k1"]), bytes.fromhex(g["transport_k2"])
    a, b = download(TA), download(TB)
    assert (a["send_keys"][0], a["recv_keys"][0]) == (k1, k2) and (b["send_keys"][0], b["recv_keys"][0]) == (k2, k1)
    for i in range(n):
        assert a["send_keys"][i] == b["recv_keys"][i] and a["recv_keys"][i] == b["send_keys"][i] and a["send_keys"][i] != bytes(32)
    assert len({a["send_keys"][i] for i in range(n)}) == n
    assert a["receivers"][:n] == list(sid_b) == b["local_ids"][:n] and b["receivers"][:n] == list(sid_a) == a["local_ids"][:n]
    assert a["slot_peer"][:n + 1] == [0, 1, 2, sc.NONE] and a["peer_slot"] == [0, 1, 2]
    assert b["slot_peer"][:n + 1] == [2, 2, 2, sc.NONE] and b["peer_slot"] == [sc.SKIP, sc.SKIP, 2]
    assert a["send_state"][:n] == [(0, now, now)] * n
    # A -> B: two packets per tunnel
    pairs = [(rc.ip(10, 0, p, 1 + j), rc.ip(10, 9, p, 7)) for p in range(n) for j in range(2)]
    desc, buf, pkts = _frames(rng, pairs)
    slots, d_buf = _send(engine, TA, table_a, desc, buf, d_now)
    assert slots == [0, 0, 1, 1, 2, 2]
    sealed = d_buf.cpu().numpy().copy()
    st_r, key_idx, inner, wire = _recv(engine, TB, table_b, desc, d_buf)
    assert st_r == [sc.OK] * 6 and key_idx == [0, 0, 1, 1, 2, 2] and inner == [64, 80] * 3
    plain = d_buf.cpu().numpy()
    for d, p in zip(desc, pkts):
        assert np.array_equal(plain[int(d["offset"]) + 16:int(d["offset"]) + 16 + len(p)], p)
    # the first tunnel's frames under the recorded keys, in the CPU oracle
    first = wire[:2].copy()
    first["key_idx"] = 0
    obuf = sealed.copy()
    ost, octr = oracle.open_batch(np.frombuffer(k1, np.uint8).reshape(1, 32), first, obuf)
    assert list(ost) == [sc.OK] * 2 and list(octr) == [0, 1]
    for d, p in zip(desc[:2], pkts[:2]):
        assert np.array_equal(obuf[int(d["offset"]) + 16:int(d["offset"]) + 16 + len(p)], p)
    # B -> A: B's peer 2 is A; its current row is the last one installed
    back = [(rc.ip(10, 9, 2, 7), rc.ip(10, 0, 3, 4 + j)) for j in range(3)]
    desc2, buf2, pkts2 = _frames(rng, back)
    slots2, d_buf2 = _send(engine, TB, table_b, desc2, buf2, d_now)
    assert slots2 == [2, 2, 2]
    st_r2, key_idx2, inner2, _ = _recv(engine, TA, table_a, desc2, d_buf2)
    assert st_r2 == [sc.OK] * 3 and key_idx2 == [2, 2, 2] and inner2 == [64, 80, 64]
    plain2 = d_buf2.cpu().numpy()
    for d, p in zip(desc2, pkts2):
        assert np.array_equal(plain2[int(d["offset"]) + 16:int(d["offset"]) + 16 + len(p)], p)
    # B's sessions pass their lifetime: the next frame of tunnel 0 finds no session there
    desc3, buf3, _ = _frames(rng, pairs[:1])
    _, d_buf3 = _send(engine, TA, table_a, desc3, buf3, d_now)
    sealed3 = d_buf3.cpu().numpy().copy()
    later = _dev(np.array([now + sc.REJECT_AFTER_NS + 1], np.uint64).view(np.int64))
    out = _fill((8,))
    session.expire_batch_dev(engine, TB, later, None, out)
    torch.cuda.synchronize()
    assert list(out.cpu().numpy()) == [1, 1, 1, 0, 0, 0, 0, 0]
    check_tables(TB, sc.empty_tables(8, 3), gone=list(sid_b))
    st_r3, key_idx3, inner3, _ = _recv(engine, TB, table_b, desc3, d_buf3)
    assert st_r3 == [sc.REJECTED] and key_idx3 == [sc.SKIP] and inner3 == [0]
    assert np.array_equal(d_buf3.cpu().numpy(), sealed3)


def test_install_finish_refuses_a_pending_row_that_does_not_exist(engine):
    """the finish wrapper against the model behind its gather: pend_idx_out >= npending on a row whose gate is OK
    is RG_PKT_INVALID (its key row consumed), on a gated row nothing is read"""
    rng = np.random.default_rng(8)
    t = sc.empty_tables(4, 3)
    gate, pend_idx, remote = [sc.OK, sc.OK, sc.REJECTED, sc.OK], [1, 2, sc.NONE, 0], [0x71, 0x72, 0, 0x73]
    pend_sids, pend_peers = [0x500, 0x501], [2, 0]
    keys = sc.key_rows(rng, 4)
    lids, rids, peers = sc.gather_finish(gate, pend_idx, remote, pend_sids, pend_peers)
    want = sc.install_loop(t, gate, lids, rids, peers, keys, 9)
    assert want[1] == [sc.OK, sc.INVALID, sc.REJECTED, sc.OK] and want[0]["peer_slot"] == [0, sc.SKIP, 1]
    T = upload(engine, t)
    d_keys, st, rows = _dev(np.frombuffer(b"".join(keys), np.uint8).reshape(4, 64)), _fill((4,)), _fill((4,), torch.int32)
    session.install_finish_batch_dev(engine, T, _dev(np.array(gate, np.uint8)), _words(pend_idx), _words(remote),
                                     _words(pend_sids), _words(pend_peers), d_keys, st, rows,
                                     now_ns=_dev(np.array([9], np.int64)))
    torch.cuda.synchronize()
    assert [int(x) for x in st.cpu().numpy()] == want[1] and [int(x) for x in _u32(rows)] == want[2]
    assert [k.tobytes() for k in d_keys.cpu().numpy()] == want[3]
    check_tables(T, want[0])


# ------------------------------------------------------------------ refusals
def test_session_argument_refusals(engine):
    """n == 0 is RG_OK; a null required pointer, n = 2^32, a misaligned array, an rx_cap that is no power of two or
    below 2 nkeys and a short workspace are RG_EINVAL with the call named, and nothing is enqueued: every array
    keeps its fill"""
    L, h = engine.library, engine.handle
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    n, nkeys, npeers = 4, 4, 2
    T = session.SessionTables(engine, nkeys, npeers)
    for name in session.ARRAYS:
        getattr(T, name).fill_(FILL if getattr(T, name).dtype == torch.uint8 else GUARD - (1 << 32))
    ids, keys, st, rows = _fill((3, n + 1), torch.int32), _fill((n + 1, 64)), _fill((n,)), _fill((n + 1,), torch.int32)
    need = int(L.rg_session_workspace_size(n, nkeys, npeers))
    ws = _fill((need + 16,))

    def install(tables=None, lid=p(ids[0]), rid=p(ids[1]), peer=p(ids[2]), tk=p(keys), n_=n, now=None, st_=p(st),
                ro=p(rows), ws_=p(ws), wl=need, **fields):
        t = T.struct()
        for k, v in fields.items():
            setattr(t, k, v)
        return L.rg_session_install_batch_dev(h, None if tables == "null" else ctypes.byref(t), None, lid, rid, peer, tk,
                                              n_, now, st_, ro, ws_, wl, s)

    assert install(n_=0) == 0
    for bad in (dict(tables="null"), dict(lid=None), dict(rid=None), dict(peer=None), dict(tk=None), dict(st_=None),
                dict(ro=None), dict(ws_=None), dict(n_=1 << 32), dict(tk=p(keys, 8)), dict(ro=p(rows, 2)),
                dict(lid=p(ids[0], 2)), dict(now=p(ids, 4)), dict(ws_=p(ws, 8)), dict(wl=need - 1), dict(wl=0),
                dict(rx_cap=0), dict(rx_cap=12), dict(rx_cap=4), dict(send_keys=None), dict(rx_table=None),
                dict(peer_slot=None), dict(send_keys=T.send_keys.data_ptr() + 8),
                dict(windows=T.windows.data_ptr() + 4), dict(rx_table=T.rx_table.data_ptr() + 4),
                dict(local_ids=T.local_ids.data_ptr() + 2)):
        assert install(**bad) == -1, bad
        assert b"session install" in L.rg_last_error(), bad
    out = _fill((nkeys,))

    def expire(rows_=None, m=0, ws_=p(ws), wl=need, **fields):
        t = T.struct()
        for k, v in fields.items():
            setattr(t, k, v)
        return L.rg_session_expire_batch_dev(h, ctypes.byref(t), None, rows_, m, p(out), ws_, wl, s)

    for bad in (dict(m=2), dict(rows_=p(ids[0]), m=1 << 32), dict(rows_=p(ids[0], 2), m=1), dict(ws_=None),
                dict(ws_=p(ws, 8)), dict(wl=int(L.rg_session_workspace_size(0, nkeys, npeers)) - 1), dict(rx_cap=24),
                dict(slot_peer=None)):
        assert expire(**bad) == -1, bad
        assert b"session expire" in L.rg_last_error(), bad
    t = T.struct()
    t.rx_cap = 6
    assert L.rg_session_index_dev(h, ctypes.byref(t), s) == -1 and b"session index" in L.rg_last_error()
    assert L.rg_session_index_dev(h, None, s) == -1
    torch.cuda.synchronize()
    for t_ in (keys, st, ws, out) + tuple(getattr(T, name) for name in session.ARRAYS if getattr(T, name).dtype == torch.uint8):
        assert (t_.cpu().numpy() == FILL).all()
    for t_ in (ids, rows, T.receivers, T.local_ids, T.slot_peer, T.rx_table, T.peer_slot):
        assert (_u32(t_) == GUARD).all()
