"""rg_handshake_init_batch_dev and rg_handshake_resp_batch_dev on the GPU against the Python model
(tests/handshake_cases.py) and the reference's recorded handshake (tests/golden/handshake_full.json):
decrypt_handshake_init + Config::get_peer_idx, then encrypt_handshake_resp + split(false), for a batch.
Every status, every byte of every result, response and key row is compared; nothing is approximate."""
import ctypes

import numpy as np
import pytest

import handshake_cases as hc
from conftest import load_golden
from oracle import oracle
from rustyguard_amd import aead
from rustyguard_amd.workloads import DESC_DTYPE

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL = 0xA5
COUNTS = [("valid", 120), ("unknown_static", 20), ("static_ct_flipped", 20), ("ts_tag_flipped", 20),
          ("ts_tag_flipped_unknown", 10), ("eph_zero", 10), ("eph_one", 10), ("static_low_order", 14), ("type2", 12),
          ("len92", 12), ("offset8", 12), ("past_buf", 10), ("gated", 20), ("key_skip", 10)]
WANT = {"valid": hc.OK, "unknown_static": hc.REJECTED, "static_ct_flipped": hc.DECRYPT_ERR,
        "ts_tag_flipped": hc.DECRYPT_ERR, "ts_tag_flipped_unknown": hc.DECRYPT_ERR, "eph_zero": hc.KEYEXCHANGE,
        "eph_one": hc.KEYEXCHANGE, "static_low_order": hc.KEYEXCHANGE, "type2": hc.INVALID, "len92": hc.INVALID,
        "offset8": hc.UNALIGNED, "past_buf": hc.INVALID, "gated": hc.REJECTED, "key_skip": hc.REJECTED}


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


class World:
    """One responder, its device tables and one batch of initiations with the model's verdicts."""

    def __init__(self, seed, kinds):
        self.r = hc.Responder(seed)
        self.kinds = kinds
        (self.desc, self.gate, self.buf, self.msgs, self.want_st, self.want_rows) = hc.init_batch(self.r, kinds,
                                                                                                  DESC_DTYPE)
        self.peers = hc.peer_rows(self.r.peers)
        self.table = aead.peer_table(self.peers)
        self.d_own, self.d_peers, self.d_table = _dev(self.r.own), _dev(self.peers), _dev(self.table)
        self.d_desc, self.d_buf = _dev(self.desc.view(np.uint8).reshape(-1, 16)), _dev(self.buf)

    def init(self, engine, gate, stream=None):
        n = len(self.kinds)
        results = torch.full((n + 2, 128), FILL, dtype=torch.uint8, device="cuda")
        status = torch.full((n + 2,), FILL, dtype=torch.uint8, device="cuda")
        engine.handshake_init_dev(self.d_own, self.d_peers, self.d_table, self.d_desc, gate, self.d_buf, results[:n],
                                  status[:n], stream=stream)
        return results, status


def _kinds(counts, seed):
    kinds = [k for k, c in counts for _ in range(c)]
    order = np.random.default_rng(seed).permutation(len(kinds))
    return [kinds[i] for i in order]


@pytest.fixture(scope="module")
def world():
    return World(2025, _kinds(COUNTS, 11))


def _check_init(w, results, status):
    n = len(w.kinds)
    res, st = results.cpu().numpy(), status.cpu().numpy()
    assert (res[n:] == FILL).all() and (st[n:] == FILL).all()
    assert np.array_equal(w.d_buf.cpu().numpy(), w.buf)  # buf is never written
    return res[:n], st[:n]


def test_init_mixed_batch_vs_model(engine, world):
    """300 messages over 5 peers and 8 ephemeral keys in fourteen categories, dealt by a seeded permutation
    with 0 / 16 / 32-byte gaps: every status and every byte of every result row (a zero row with peer =
    RG_PEER_NONE for every failure), buf untouched; gate = NULL equals a gate of all RG_PKT_OK."""
    w = world
    for k, s in zip(w.kinds, w.want_st):  # the model agrees with the header's table
        assert s == WANT[k], k
    results, status = w.init(engine, _dev(w.gate))
    torch.cuda.synchronize()
    res, st = _check_init(w, results, status)
    assert list(st) == list(w.want_st)
    diff = np.argwhere(res != w.want_rows)
    assert len(diff) == 0, (len(diff), sorted(set(diff[:, 1]))[:40], [w.kinds[i] for i in sorted(set(diff[:, 0]))[:5]])
    ok = st == hc.OK
    assert (res[~ok] == np.frombuffer(hc.ZERO_ROW, np.uint8)).all()
    assert set(np.ascontiguousarray(res[ok][:, 108:112]).view(np.uint32).ravel()) == set(range(5))
    # without a gate the gated messages are judged like any other: here they are valid
    r_none, s_none = w.init(engine, None)
    r_zero, s_zero = w.init(engine, _dev(np.zeros(len(w.kinds), np.uint8)))
    torch.cuda.synchronize()
    res_n, st_n = _check_init(w, r_none, s_none)
    res_z, st_z = _check_init(w, r_zero, s_zero)
    assert np.array_equal(st_n, st_z) and np.array_equal(res_n, res_z)
    gated = np.array([k == "gated" for k in w.kinds])
    assert np.array_equal(st_n[~gated], w.want_st[~gated]) and np.array_equal(res_n[~gated], w.want_rows[~gated])
    for i in np.flatnonzero(gated):
        assert (int(st_n[i]), res_n[i].tobytes()) == hc.consume_initiation(w.msgs[i], w.r.sk_r, w.r.peer_keys)
        assert st_n[i] == hc.OK


@pytest.mark.parametrize("n", [1, 65])
def test_init_small_batches(engine, n):
    counts = [("valid", 1)] if n == 1 else [("valid", 40), ("unknown_static", 5), ("static_ct_flipped", 5),
                                            ("ts_tag_flipped", 5), ("eph_zero", 3), ("static_low_order", 3),
                                            ("gated", 2), ("past_buf", 2)]
    w = World(2025, _kinds(counts, 5))
    assert len(w.kinds) == n
    results, status = w.init(engine, _dev(w.gate))
    torch.cuda.synchronize()
    res, st = _check_init(w, results, status)
    assert list(st) == list(w.want_st) and np.array_equal(res, w.want_rows)


def _resp(engine, w, rows, gate, esk, sids, cookies, has_cookie, stream=None):
    n = len(rows)
    d_rows = _dev(rows)
    responses = torch.full((n + 1, 96), FILL, dtype=torch.uint8, device="cuda")
    keys = torch.full((n + 1, 64), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((n + 1,), FILL, dtype=torch.uint8, device="cuda")
    engine.handshake_resp_dev(w.d_peers, d_rows, None if gate is None else _dev(gate), _dev(esk), _dev(sids),
                              None if cookies is None else _dev(cookies),
                              None if has_cookie is None else _dev(has_cookie), responses[:n], keys[:n], status[:n],
                              stream=stream)
    torch.cuda.synchronize()
    out = (d_rows.cpu().numpy(), responses.cpu().numpy(), keys.cpu().numpy(), status.cpu().numpy())
    assert (out[1][n:] == FILL).all() and (out[2][n:] == FILL).all() and (out[3][n:] == FILL).all()
    return out[0], out[1][:n], out[2][:n], out[3][:n]


def test_response_vs_model(engine, world):
    """the response call over the valid rows: half with cookies, some gated off (untouched), one row with
    peer = npeers (RG_PKT_INVALID), one with a zero ephemeral key (RG_PKT_KEYEXCHANGE): responses, key rows
    and statuses against the model; consumed rows lose their chain and hash."""
    w = world
    rng = np.random.default_rng(77)
    rows = w.want_rows[w.want_st == hc.OK].copy()
    n = len(rows)
    assert n == 120
    rows[5, 108:112] = np.frombuffer((5).to_bytes(4, "little"), np.uint8)  # peer = npeers
    rows[9, 64:96] = 0  # an ephemeral key of small order: ee is all zero
    gate = np.zeros(n, np.uint8)
    gate[[3, 17, 64, 119]] = [hc.REJECTED, hc.DECRYPT_ERR, 6, 7]
    esk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    sids = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    cookies = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    has_cookie = (np.arange(n) % 2).astype(np.uint8)
    after, resp, keys, st = _resp(engine, w, rows, gate, esk, sids, cookies, has_cookie)
    for i in range(n):
        if gate[i]:
            assert st[i] == hc.REJECTED and np.array_equal(after[i], rows[i]), i
            assert (resp[i] == FILL).all() and (keys[i] == FILL).all(), i
            continue
        want_st, want_resp, want_keys = hc.build_response(rows[i].tobytes(), w.r.peers, esk[i].tobytes(), int(sids[i]),
                                                          cookies[i].tobytes() if has_cookie[i] else None)
        assert st[i] == want_st, i
        assert resp[i].tobytes() == want_resp + bytes(4), i
        assert keys[i].tobytes() == want_keys, i
        assert (after[i, :64] == 0).all() and np.array_equal(after[i, 64:], rows[i, 64:]), i
    assert st[5] == hc.INVALID and st[9] == hc.KEYEXCHANGE and (st == hc.OK).sum() == n - 6
    # cookies = NULL: every mac2 is zero
    after, resp, keys, st = _resp(engine, w, rows[:3], None, esk[:3], sids[:3], None, None)
    for i in range(3):
        assert (int(st[i]), resp[i].tobytes()[:92], keys[i].tobytes()) == hc.build_response(
            rows[i].tobytes(), w.r.peers, esk[i].tobytes(), int(sids[i]), None)


def test_recorded_handshake_through_both_calls(engine):
    """the reference's recorded initiation goes in, its recorded response and the receive key 5c1ba029...
    come out."""
    g = load_golden("handshake_full.json")["snapshot"]
    sk_i, sk_r = bytes.fromhex(g["static_private_i"]), bytes.fromhex(g["static_private_r"])
    pk_i = hc.pubkey(sk_i)
    peers = hc.peer_rows([(pk_i, bytes.fromhex(g["preshared_key"]), hc.mac1_key(pk_i))])
    own = np.frombuffer(sk_r + hc.pubkey(sk_r), np.uint8)
    buf = np.zeros(160, np.uint8)
    buf[:148] = np.frombuffer(bytes.fromhex(g["initiation"]), np.uint8)
    desc = np.array([(0, 148, 0)], DESC_DTYPE)
    results = torch.zeros((1, 128), dtype=torch.uint8, device="cuda")
    status = torch.full((1,), FILL, dtype=torch.uint8, device="cuda")
    d_peers = _dev(peers)
    engine.handshake_init_dev(_dev(own), d_peers, _dev(aead.peer_table(peers)), _dev(desc.view(np.uint8)), None,
                              _dev(buf), results, status)
    responses = torch.zeros((1, 96), dtype=torch.uint8, device="cuda")
    keys = torch.zeros((1, 64), dtype=torch.uint8, device="cuda")
    st2 = torch.full((1,), FILL, dtype=torch.uint8, device="cuda")
    row_before = results.clone()
    engine.handshake_resp_dev(d_peers, results, status, _dev(np.frombuffer(bytes.fromhex(g["esk_r"]), np.uint8)),
                              _dev(np.array([g["session_id"]], np.uint32)), None, None, responses, keys, st2)
    torch.cuda.synchronize()
    assert status.item() == hc.OK and st2.item() == hc.OK
    assert row_before.cpu().numpy().tobytes().hex() == g["result_row"]
    assert responses.cpu().numpy().tobytes()[:92].hex() == g["response"]
    k = keys.cpu().numpy().tobytes()
    assert k[:32].hex() == g["send_key"] and k[32:].hex() == g["recv_key"]
    assert g["recv_key"].startswith("5c1ba029")


def test_filter_init_response_chain_and_sessions(engine, world):
    """one round trip on one stream with no host step between the filter and the init call:
    rg_cookie_reply_batch_dev's status is the init call's gate; then the response, whose mac1 passes
    rg_mac_verify_batch_dev, and whose key row, inserted with rg_sessions_insert, opens a transport packet that
    the model's initiator sealed."""
    r = world.r
    rng = np.random.default_rng(5)
    n = 6
    made = [hc.make_initiation(r.sk_i[i % 5], r.pk_r, r.esk_i[i], hc.tai64n(1_800_000_000, i), 1000 + i) for i in range(n)]
    msgs = [bytearray(m[0]) for m in made]
    msgs[2][120] ^= 1  # mac1 broken: the filter rejects it and the gate keeps it out of the handshake
    buf = np.zeros(160 * n, np.uint8)
    for i, m in enumerate(msgs):
        buf[160 * i:160 * i + 148] = np.frombuffer(bytes(m), np.uint8)
    desc = np.array([(160 * i, 148, 0) for i in range(n)], DESC_DTYPE)
    ck = hc.mac1_key(r.pk_r) + rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
    addrs = np.frombuffer(b"".join(aead.encode_src_addr("192.0.2.%d" % i, 4000 + i) for i in range(n)), np.uint8)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_desc, d_buf = _dev(desc.view(np.uint8).reshape(-1, 16)), _dev(buf)
        d_ck, d_addrs = _dev(np.frombuffer(ck, np.uint8)), _dev(addrs.reshape(n, 24))
        d_over, d_nonces = _dev(np.zeros(n, np.uint8)), _dev(rng.integers(0, 256, (n, 24), dtype=np.uint8))
        replies = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
        gate = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
        results = torch.zeros((n, 128), dtype=torch.uint8, device="cuda")
        status = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
        esk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        sids = np.arange(n, dtype=np.uint32) + 0x100
        d_esk, d_sids = _dev(esk), _dev(sids)
        responses = torch.zeros((n, 96), dtype=torch.uint8, device="cuda")
        keys = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
        st2 = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    s.synchronize()
    engine.cookie_reply_dev(d_ck, d_desc, d_addrs, d_over, d_nonces, d_buf, replies, gate, stream=s)
    engine.handshake_init_dev(world.d_own, world.d_peers, world.d_table, d_desc, gate, d_buf, results, status, stream=s)
    engine.handshake_resp_dev(world.d_peers, results, status, d_esk, d_sids, None, None, responses, keys, st2, stream=s)
    s.synchronize()
    want = [hc.OK] * n
    want[2] = hc.REJECTED
    assert list(gate.cpu().numpy()) == want and list(status.cpu().numpy()) == want
    assert list(st2.cpu().numpy()) == want
    resp, keys = responses.cpu().numpy(), keys.cpu().numpy()
    assert (resp[2] == 0).all() and (keys[2] == 0).all()
    # mac1 of every response under its peer's mac1 key
    live = [i for i in range(n) if i != 2]
    mdesc = np.array([(96 * i, 92, i % 5) for i in live], DESC_DTYPE)
    mst = torch.full((len(live),), FILL, dtype=torch.uint8, device="cuda")
    engine.mac_verify_dev(_dev(np.ascontiguousarray(world.peers[:, 64:96])), 1, _dev(mdesc.view(np.uint8).reshape(-1, 16)),
                          responses, mst)
    torch.cuda.synchronize()
    assert list(mst.cpu().numpy()) == [hc.OK] * len(live)
    # the initiator finishes the handshake with the model and seals a packet; the responder's session opens it
    sessions = aead.Sessions(engine, 16)
    for i in live:
        fin = hc.finish_initiator(resp[i].tobytes()[:92], made[i][1], r.sk_i[i % 5], r.esk_i[i], r.peers[i % 5][1])
        assert fin is not None, i
        send_i, recv_i = fin
        assert keys[i].tobytes() == recv_i + send_i, i
        sessions.insert(int(sids[i]), 1000 + i, keys[i, :32].tobytes(), keys[i, 32:].tobytes())
    frames = np.zeros(64 * len(live), np.uint8)
    fdesc = np.array([(64 * j, 64, 0) for j in range(len(live))], DESC_DTYPE)
    plain = []
    for j, i in enumerate(live):
        pt = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
        plain.append(pt)
        ct, tag = oracle.aead_seal(keys[i, 32:].tobytes(), oracle.wg_nonce(0), b"", pt)
        hdr = (4).to_bytes(4, "little") + int(sids[i]).to_bytes(4, "little") + (0).to_bytes(8, "little")
        frames[64 * j:64 * j + 64] = np.frombuffer(hdr + ct + tag, np.uint8)
    st, _ = sessions.recv_batch(fdesc, frames)
    assert list(st) == [hc.OK] * len(live)
    for j, pt in enumerate(plain):
        assert frames[64 * j + 16:64 * j + 48].tobytes() == pt


def test_argument_refusals(engine, world):
    """null pointers, misaligned arrays and a cap that is no power of two: RG_EINVAL, nothing touched."""
    w = world
    L, h = engine.library, engine.handle
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = 4
    results = torch.full((n + 1, 128), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    cap = len(w.table)

    def init(own=p(w.d_own), peers=p(w.d_peers), table=p(w.d_table), cap=cap, desc=p(w.d_desc), buf=p(w.d_buf),
             res=p(results), st=p(status), n=n):
        return L.rg_handshake_init_batch_dev(h, own, peers, 5, table, cap, desc, None, n, buf, len(w.buf), res, st, s)

    assert init(n=0) == 0
    for bad in (dict(own=None), dict(peers=None), dict(table=None), dict(desc=None), dict(buf=None), dict(res=None),
                dict(st=None), dict(own=p(w.d_own, 8)), dict(peers=p(w.d_peers, 4)), dict(res=p(results, 8)),
                dict(desc=p(w.d_desc, 8)), dict(table=p(w.d_table, 2)), dict(cap=cap - 1), dict(cap=0), dict(cap=24),
                dict(n=1 << 32)):
        assert init(**bad) == -1, bad
    assert b"handshake init" in L.rg_last_error()
    responses = torch.full((n + 1, 96), FILL, dtype=torch.uint8, device="cuda")
    keys = torch.full((n + 1, 64), FILL, dtype=torch.uint8, device="cuda")
    esk = torch.zeros((n + 1, 32), dtype=torch.uint8, device="cuda")
    sids = torch.zeros((n + 1,), dtype=torch.int32, device="cuda")
    cookies = torch.zeros((n + 1, 16), dtype=torch.uint8, device="cuda")
    has = torch.zeros((n,), dtype=torch.uint8, device="cuda")

    def resp(peers=p(w.d_peers), res=p(results), esk_p=p(esk), sid=p(sids), ck=None, hc_=None, out=p(responses),
             tk=p(keys), st=p(status), n=n):
        return L.rg_handshake_resp_batch_dev(h, peers, 5, res, None, esk_p, sid, ck, hc_, n, out, tk, st, s)

    assert resp(n=0) == 0
    for bad in (dict(peers=None), dict(res=None), dict(esk_p=None), dict(sid=None), dict(out=None), dict(tk=None),
                dict(st=None), dict(ck=p(cookies)), dict(peers=p(w.d_peers, 8)), dict(res=p(results, 4)),
                dict(out=p(responses, 8)), dict(tk=p(keys, 8)), dict(esk_p=p(esk, 2)), dict(sid=p(sids, 2)),
                dict(ck=p(cookies, 1), hc_=p(has)), dict(n=1 << 32)):
        assert resp(**bad) == -1, bad
    assert b"handshake resp" in L.rg_last_error()
    torch.cuda.synchronize()
    for t in (results, status, responses, keys):
        assert (t.cpu().numpy() == FILL).all()
