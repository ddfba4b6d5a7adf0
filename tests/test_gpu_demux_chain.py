"""The inbound demultiplexer composed with the chains it feeds.  One node S receives one mixed batch from a peer P:
valid initiations, valid responses to its own pending handshakes, cookie replies to its own initiations, data frames
with a keepalive, a forged frame and replays, forged messages of every kind and junk, a wave and one lane of each
class.  Every message is made on the GPU by the calls a peer would run.  The batch goes two ways:
  (a) rg_demux_batch_dev, the existing calls on the lists exactly as the demux left them (inert rows and all: the
      rate count, the filter under its flags, init, finish, consume, the resident receive, the endpoint note), then
      rg_demux_verdict_batch_dev: no host step from the descriptor array to the final statuses;
  (b) the lists split on the host into dense arrays, the same calls on those with the gates gathered on the host, and
      the way back computed on the host.
Final statuses and every chain output (results, transport keys, pending rows, peer state, cookies, replies, windows,
decrypted frames, endpoints) are compared between the two."""
import numpy as np
import pytest

import demux_cases as dc
import handshake_cases as hc
import peerstate_cases as pc
from rustyguard_amd import aead, demux, endpoint, ratelimit
from rustyguard_amd.workloads import DESC_DTYPE

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K = 4        # valid messages of each handshake kind, and S's pending rows
PER = 65     # datagrams of each class: one wave and one lane
SLOT = 160   # bytes of buf a datagram owns
PAY = 64
IDS = ((0x1A0, 0x2A0), (0x1B0, 0x2B0))  # (S's id, P's id) of two transport sessions; only the first carries traffic


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _words(values):
    return _dev(np.array(values, np.uint32).view(np.int32))


def _desc(rows):
    return _dev(np.array(rows, DESC_DTYPE).view(np.uint8).reshape(-1, 16))


def _zeros(*shape, dtype=torch.uint8):
    return torch.zeros(shape, dtype=dtype, device="cuda")


class Node:
    """S's configuration and everything P sent it, made once"""

    def __init__(self, engine):
        rng = self.rng = np.random.default_rng(404)
        rb = lambda k: bytes(rng.integers(0, 256, k, dtype=np.uint8))  # noqa: E731
        self.engine = e = engine
        sk_s, sk_p, psk, self.secret = rb(32), rb(32), rb(32), rb(32)
        pk_s, pk_p = hc.pubkey(sk_s), hc.pubkey(sk_p)
        b = lambda x: _dev(np.frombuffer(x, np.uint8))  # noqa: E731
        own_p = b(sk_p + pk_p)
        self.own = b(sk_s + pk_s)
        row_s, row_p = (pk_s, psk, hc.mac1_key(pk_s)), (pk_p, psk, hc.mac1_key(pk_p))
        pidx = _words(range(K))
        ts = _dev(np.frombuffer(b"".join(hc.tai64n(1_900_000_000, i) for i in range(K)), np.uint8).reshape(K, 12))
        st = [_zeros(K) for _ in range(6)]
        # P initiates to S, one tunnel per row of P's table
        self.inits, pend_p = _zeros(K, 160), _zeros(K, 128)
        e.handshake_initiate_dev(own_p, _dev(hc.peer_rows([row_s] * K)), pidx, None, _dev(rng.integers(0, 256, (K, 32), dtype=np.uint8)),
                                 ts, _words(range(0x0C00, 0x0C00 + K)), None, None, self.inits, pend_p, st[0])
        # S initiates to P: S's pending rows, and the mac1 its cookie replies are opened under
        self.sids = np.arange(0x0A11, 0x0A11 + K, dtype=np.uint32)
        self.peers_i = _dev(hc.peer_rows([row_p] * K))
        msgs_s, self.pending = _zeros(K, 160), _zeros(K, 128)
        e.handshake_initiate_dev(self.own, self.peers_i, pidx, None, _dev(rng.integers(0, 256, (K, 32), dtype=np.uint8)), ts,
                                 _dev(self.sids), None, None, msgs_s, self.pending, st[1])
        self.state = _zeros(K, pc.ROW)
        e.peer_mac1_dev(self.state, pidx, st[1], msgs_s, 160, 116, _zeros(K, dtype=torch.int32))
        # P answers S's initiations, and -- under load -- also sends a cookie reply for each
        peers_p = _dev(hc.peer_rows([row_s]))
        desc_s = _desc([(160 * i, 148, 0) for i in range(K)])
        results, keys_p = _zeros(K, 128), _zeros(K, 64)
        self.responses, self.cookie_msgs = _zeros(K, 96), _zeros(K, 64)
        e.handshake_init_dev(own_p, peers_p, _dev(aead.peer_table(hc.peer_rows([row_s]))), desc_s, None, msgs_s, results, st[2])
        e.handshake_resp_dev(peers_p, results, st[2], _dev(rng.integers(0, 256, (K, 32), dtype=np.uint8)),
                             _words(range(0x0B22, 0x0B22 + K)), None, None, self.responses, keys_p, st[3])
        ck_p = hc.mac1_key(pk_p) + pc.cookie_key(pk_p) + rb(32)
        addr_s = np.frombuffer(aead.encode_src_addr("192.0.2.7", 51820) * K, np.uint8).reshape(K, 24)
        e.cookie_reply_dev(b(ck_p), desc_s, _dev(addr_s), None, _dev(rng.integers(0, 256, (K, 24), dtype=np.uint8)), msgs_s,
                           self.cookie_msgs, st[4])
        torch.cuda.synchronize()
        assert [list(s.cpu().numpy()) for s in st[:5]] == [[dc.OK] * K] * 4 + [[dc.COOKIE] * K]
        # S's side of the receive chains
        self.cookie_keys = b(hc.mac1_key(pk_s) + pc.cookie_key(pk_s) + self.secret)  # rg_cookie_keys of the filter
        peers_r = hc.peer_rows([row_p])
        self.peers_r, self.table_r = _dev(peers_r), _dev(aead.peer_table(peers_r))
        self.pend_table = _dev(aead.pending_table(self.sids))
        self.peer_cookie_keys = b(pc.cookie_key(pk_p) * K)
        self.sess_table = _dev(aead.rx_table(self.sids, np.arange(K, dtype=np.uint32)))
        # transport: P's end is a host session table that seals real frames; counter 5 is a keepalive
        k = [rb(32) for _ in range(4)]
        remote = aead.Sessions(engine, 4)
        ra = remote.insert(IDS[0][1], IDS[0][0], k[0], k[1])
        pays = [PAY, PAY, PAY, PAY, PAY, 0, PAY]
        sdesc = np.array([(SLOT * i, p, 0) for i, p in enumerate(pays)], DESC_DTYPE)
        sbuf = np.zeros(SLOT * len(pays), np.uint8)
        sbuf.reshape(-1, SLOT)[:, 16:16 + PAY] = rng.integers(0, 256, (len(pays), PAY), dtype=np.uint8)
        sst, _ = remote.send_batch([ra] * len(pays), sdesc, sbuf)
        assert (sst == dc.OK).all()
        self.frames = [sbuf[SLOT * i:SLOT * i + p + 32].copy() for i, p in enumerate(pays)]
        self.recv_keys = _dev(np.frombuffer(k[0] + k[2], np.uint8).reshape(2, 32))
        self.rx_table = _dev(aead.rx_table([IDS[0][0], IDS[1][0]], [0, 1]))
        self.slot_peer = _words([0, 1])
        self.batch()

    def batch(self):
        """the mixed batch: PER datagrams of each class and PER of junk, in strict turn; every datagram owns a slot"""
        rng = self.rng
        flip = lambda m, at: np.concatenate([m[:at], m[at:at + 1] ^ 1, m[at + 1:]])  # noqa: E731
        inits = [m[:148] for m in self.inits.cpu().numpy()]
        resps = [m[:92] for m in self.responses.cpu().numpy()]
        cks = list(self.cookie_msgs.cpu().numpy())
        fr = self.frames
        hs = inits + resps + [flip(inits[0], 120), flip(inits[1], 50), flip(resps[0], 70), flip(resps[1], 20)] + inits[:2] + resps
        ck = cks + [flip(cks[0], 40), flip(cks[1], 9)] + cks[:2]
        data = [fr[0], fr[1], fr[5], flip(fr[6], 60), fr[2], fr[1], fr[3], fr[4], fr[0], flip(fr[2], 17)]
        junk = [(np.zeros(64, np.uint8), {}), (inits[2], dict(len=92)), (resps[2], dict(len=148)), (cks[2], dict(len=80)),
                (fr[3], dict(key=dc.SKIP)), (fr[3], dict(shift=8)), (fr[3], dict(len=3)), (flip(inits[3], 1), {}),
                (np.full(32, 5, np.uint8), {})]
        n = 4 * PER
        buf, desc = rng.integers(0, 256, n * SLOT, dtype=np.uint8), np.zeros(n, DESC_DTYPE)
        for i in range(n):
            j, kind = i // 4, i % 4
            m, how = [(hs[j % len(hs)], {}), (ck[j % len(ck)], {}), (data[j % len(data)], {}), junk[j % len(junk)]][kind]
            buf[SLOT * i:SLOT * i + len(m)] = m
            desc[i] = (SLOT * i + how.get("shift", 0), how.get("len", len(m)), how.get("key", int(rng.integers(0, 1 << 31))))
        self.n, self.buf, self.desc = n, buf, desc
        self.addrs = rng.integers(0, 256, (n, 24), dtype=np.uint8)
        self.addrs[:, 18:] = 0  # the callers of the dense path hand over what the socket gave them: no pad bytes
        self.caps = (PER + 1, PER + 1, PER + 1)
        # the handshake messages come from three sources in turn: the rate count lets the first ten of each through
        # (every valid message passes at least once) and flags the rest, which the filter answers with a cookie reply
        hs_at = np.arange(0, n, 4)
        self.addrs[hs_at, :16] = 0
        self.addrs[hs_at, :4] = np.stack([np.full(PER, 10), np.zeros(PER), np.zeros(PER), np.arange(PER) % 3], axis=1)
        self.seeds = rng.integers(0, 256, (ratelimit.RATE_DEPTH, 16), dtype=np.uint8)
        self.nonces = rng.integers(0, 256, (self.caps[0], 24), dtype=np.uint8)

    def chains(self, lists, gates=None):
        """the existing calls over `lists` (hs_desc, hs_addrs, init_desc, resp_desc, ck_desc, data_desc, data_addrs);
        gates = (init gate, finish gate) or None: the filter's status array as it is.  -> every output, on the host"""
        e = self.engine
        hs_desc, hs_addrs, init_desc, resp_desc, ck_desc, data_desc, data_addrs = lists
        nh, ni, nr, nc, nd = (len(x) for x in (hs_desc, init_desc, resp_desc, ck_desc, data_desc))
        buf, pending, state = _dev(self.buf), self.pending.clone(), self.state.clone()
        windows, T = _zeros(2, 264), endpoint.EndpointTable(e, 2)
        replies, results, tkeys = _zeros(nh, 64), _zeros(ni, 128), _zeros(nr, 64)
        pidx, remote = _zeros(nr, dtype=torch.int32), _zeros(nr, dtype=torch.int32)
        cookies, kidx = _zeros(nc, 16), _zeros(nd, dtype=torch.int32)
        st = {k: torch.full((m,), 0xA5, dtype=torch.uint8, device="cuda")
              for k, m in (("filter", nh), ("init", ni), ("finish", nr), ("cookie", nc), ("data", nd))}
        R = ratelimit.RateTables(e)
        R.seeds.copy_(_dev(self.seeds))
        over, counts = torch.full((nh,), 0xA5, dtype=torch.uint8, device="cuda"), _zeros(nh, dtype=torch.int32)
        ratelimit.count_dev(e, R, hs_desc, hs_addrs, buf, over, counts_out=counts)
        e.cookie_reply_dev(self.cookie_keys, hs_desc, hs_addrs, over, _dev(self.nonces[:nh]), buf, replies, st["filter"])
        if gates is None:
            g_init = g_fin = st["filter"]
        else:
            torch.cuda.synchronize()  # the host step of the dense path
            f = st["filter"].cpu().numpy()
            g_init, g_fin = _dev(f[gates[0]]), _dev(f[gates[1]])
        e.handshake_init_dev(self.own, self.peers_r, self.table_r, init_desc, g_init, buf, results, st["init"])
        e.handshake_finish_dev(self.own, self.peers_i, self.pend_table, pending, resp_desc, g_fin, buf, tkeys, pidx, remote,
                               _zeros(K, dtype=torch.int32), st["finish"])
        e.peer_cookie_consume_dev(state, self.peer_cookie_keys, self.sess_table, ck_desc, None, buf, cookies,
                                  _zeros(K, dtype=torch.int32), st["cookie"])
        e.recv_batch_dev_resident(self.recv_keys, self.rx_table, windows, data_desc, buf, st["data"], key_idx_out=kidx,
                                  workspace=e.replay_workspace(nd, 2))
        T.note_recv_batch_dev(self.slot_peer, kidx, st["data"], data_addrs)
        return st, dict(replies=replies, results=results, tkeys=tkeys, pidx=pidx, remote=remote, cookies=cookies, kidx=kidx,
                        buf=buf, pending=pending, state=state, windows=windows, endpoints=T.endpoints, over=over,
                        counts=counts, buckets=R.buckets)


@pytest.fixture(scope="module")
def node(engine):
    return Node(engine)


def test_demux_chains_verdict_against_the_host_split(engine, node):
    w = node
    n, caps = w.n, w.caps
    model = dc.demux_model(w.desc, w.addrs, w.buf, caps)
    rank = [int(x) for x in model["counts"][:3]]
    assert rank == [PER] * 3 == [int(x) for x in model["counts"][3:]] and int((model["cls"] == 0).sum()) == PER
    # (a) on the device, end to end
    D = demux.Demux(engine, n, *caps)
    D.batch_dev(_desc(w.desc), _dev(w.addrs), _dev(w.buf))
    st_a, out_a = w.chains((D.hs_desc, D.hs_addrs, D.init_desc, D.resp_desc, D.ck_desc, D.data_desc, D.data_addrs))
    D.verdict_batch_dev(n, st_a["filter"], st_a["init"], st_a["finish"], st_a["cookie"], st_a["data"])
    torch.cuda.synchronize()
    final_a = D.status.cpu().numpy()
    # (b) split on the host into dense lists
    rows = lambda a: _dev(np.ascontiguousarray(a).view(np.uint8).reshape(-1, 16))  # noqa: E731
    hs = model["hs_desc"][:rank[0]]
    ki = np.nonzero(model["init_desc"][:rank[0]] != dc.INERT)[0]
    kr = np.nonzero(model["resp_desc"][:rank[0]] != dc.INERT)[0]
    assert len(ki) + len(kr) == rank[0] and len(ki) > K and len(kr) > K
    st_b, out_b = w.chains((rows(hs), _dev(model["hs_addrs"][:rank[0]]), rows(hs[ki]), rows(hs[kr]),
                            rows(model["ck_desc"][:rank[1]]), rows(model["data_desc"][:rank[2]]),
                            _dev(model["data_addrs"][:rank[2]])), gates=(ki, kr))
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy()  # noqa: E731
    full = {"filter": np.full(caps[0], dc.PENDING, np.uint8), "init": np.full(caps[0], dc.PENDING, np.uint8),
            "finish": np.full(caps[0], dc.PENDING, np.uint8), "cookie": host(st_b["cookie"]), "data": host(st_b["data"])}
    full["filter"][:rank[0]] = host(st_b["filter"])
    full["init"][ki], full["finish"][kr] = host(st_b["init"]), host(st_b["finish"])
    final_b = dc.verdict_model(model["status"], model["cls"], model["pos"], caps, full)
    assert np.array_equal(final_a, final_b), np.nonzero(final_a != final_b)[0][:8]
    # the batch exercised what it was built for
    assert not (final_a == dc.PENDING).any()
    by_cls = {c: set(int(x) for x in final_a[model["cls"] == c]) for c in range(5)}
    assert by_cls[0] == {dc.INVALID, dc.REJECTED, dc.UNALIGNED}
    assert {dc.OK, dc.COOKIE, dc.REJECTED} <= by_cls[1] and {dc.OK, dc.REJECTED} <= by_cls[2]
    assert {dc.OK, dc.REJECTED} <= by_cls[3] or {dc.OK, dc.DECRYPT_ERR} <= by_cls[3]
    assert by_cls[4] == {dc.OK, dc.DECRYPT_ERR, dc.REJECTED}
    # the chain statuses over the padded lists: what (b) saw at the rows that are real, RG_PKT_INVALID at the inert rows
    fa = host(st_a["filter"])
    assert np.array_equal(fa[:rank[0]], host(st_b["filter"])) and (fa[rank[0]:] == dc.INVALID).all()
    for name, real in (("init", ki), ("finish", kr)):
        sa = host(st_a[name])
        inert = np.ones(caps[0], bool)
        inert[real] = False
        assert np.array_equal(sa[real], host(st_b[name])) and (sa[inert] == dc.INVALID).all(), name
    for name, r in (("cookie", rank[1]), ("data", rank[2])):
        sa = host(st_a[name])
        assert np.array_equal(sa[:r], host(st_b[name])) and (sa[r:] == dc.INVALID).all(), name
    # every chain output
    ok_i, ok_r = host(st_b["init"]) == dc.OK, host(st_b["finish"]) == dc.OK
    assert ok_i.sum() >= K and ok_r.sum() == K  # a replayed response finds its pending row gone
    assert np.array_equal(host(out_a["results"])[ki][ok_i], host(out_b["results"])[ok_i])
    for k in ("tkeys", "pidx", "remote"):
        assert np.array_equal(host(out_a[k])[kr][ok_r], host(out_b[k])[ok_r]), k
    # the rate count over the padded list: the inert row is not counted, the sketch ends the same
    assert not host(out_a["over"])[rank[0]:].any() and not host(out_a["counts"])[rank[0]:].any()
    assert set(host(out_b["over"])) == {0, 1} and host(out_a["buckets"]).any()
    for k, r in (("over", rank[0]), ("counts", rank[0]), ("replies", rank[0]), ("cookies", rank[1]), ("kidx", rank[2])):
        assert np.array_equal(host(out_a[k])[:r], host(out_b[k])), k
    for k in ("buf", "pending", "state", "windows", "endpoints", "buckets"):
        assert np.array_equal(host(out_a[k]), host(out_b[k])), k
    assert not np.array_equal(host(out_a["pending"]), host(w.pending)) and not np.array_equal(host(out_a["state"]), host(w.state))
    assert host(out_a["windows"])[0].any() and host(out_a["endpoints"])[0, 18] == 1 and not host(out_a["endpoints"])[1].any()
