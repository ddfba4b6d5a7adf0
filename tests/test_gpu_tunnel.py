"""Four complete nodes (A and its three responders B, B3 and B5) on one GPU, every state table device-resident, talking to each other through the chains
of INTEGRATION.md §4 tick by tick, against the model nodes of tests/tunnel_cases.py that run the same ticks in plain
Python.  `DeviceNode` has one method per chain: it stages the chain's inputs in arrays allocated once, then enqueues
that chain's line call by call with no host read in between; frames and handshake messages go from node to node as
device copies.  After every chain every byte of every output array and of every table of every node is compared with
the model.  Two tables are compared by meaning, because include/rg_aead.h leaves their layout to arrival order
(rg_session_tables, "rx_table is rebuilt ... depends on arrival"; rg_pending_index_dev): rx_table and pend_table,
through a lookup of every live id and the set of occupied entries; pend_table may besides keep an entry that names a
row the finish call wiped, until its next rebuild (rg_pending_tables: "a stale pend_table entry that names a wiped
row is harmless").  The claim arrays of rg_handshake_finish_batch_dev, rg_peer_cookie_consume_batch_dev and
rg_peer_mac1_batch_dev are, in the header's words, "a workspace of the call" that the call itself initialises; they
hold no state between calls and are not compared.  The endpoint claim words, which every call must leave zero, are."""
import ctypes
import copy

import numpy as np
import pytest

import timer_cases as tc
import tunnel_cases as tn
from rustyguard_amd import _lib, aead, endpoint, pending, ratelimit, route, session, timers

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NP, NK, NB, FILL = tn.NP, tn.NK, tn.NB, tn.FILL
FILL32 = int.from_bytes(bytes([FILL]) * 4, "little") - (1 << 32)
FILL64 = int.from_bytes(bytes([FILL]) * 8, "little") - (1 << 64)


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _bytes_dev(b, *shape):
    t = _dev(np.frombuffer(bytes(b), np.uint8))
    return t.reshape(*shape) if shape else t


def _words(values):
    return _dev(np.array(values, np.uint32).view(np.int32))


def _u8(*shape):
    return torch.full(shape, FILL, dtype=torch.uint8, device="cuda")


def _i32(n):
    return torch.full((n,), FILL32, dtype=torch.int32, device="cuda")


def _i64(n):
    return torch.full((n,), FILL64, dtype=torch.int64, device="cuda")


def _host(t):
    return t.cpu().numpy().tobytes()


class DeviceNode:
    def __init__(self, name, cfg, engine):
        e = self.engine = engine
        self.name, self.cfg = name, cfg
        self.own = _bytes_dev(cfg.sk + cfg.pk)
        rows = np.frombuffer(b"".join(a + b + c for a, b, c in cfg.peers), np.uint8).reshape(NP, 96).copy()
        self.peers, self.peer_table = _dev(rows), _dev(aead.peer_table(rows))
        self.ck = _bytes_dev(cfg.cookie_keys)
        self.peer_cookie_keys = _bytes_dev(b"".join(cfg.peer_cookie_keys), NP, 32)
        self.rtable = _dev(route.build_table(route.prefixes([((int(net).to_bytes(4, "big"), plen), peer)
                                                              for net, plen, peer in cfg.routes])))
        self.pstate = torch.zeros((NP, 64), dtype=torch.uint8, device="cuda")
        self.ST, self.tm = session.SessionTables(e, NK, NP), timers.timer_rows(e, NK)
        self.PT, self.EP, self.RT = pending.PendingTables(e, NP), endpoint.EndpointTable(e, NP), ratelimit.RateTables(e)
        self.EP.endpoints.copy_(_dev(cfg.endpoint_rows()))
        self.arr = {k: _u8(v) for k, v in tn.SIZES.items()}
        self.now = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.ws_r, self.ws_s = e.replay_workspace(NB, NK), e.send_workspace(NB, NK)
        self.ws_sess, self.ws_t = session.session_workspace(e, NP, NK, NP), timers.timer_workspace(e, NK, NP)
        self.ws_p, self.ws_ts = pending.pending_workspace(e, NP, NB, NP), e.peer_ts_workspace(NP, NP)
        self.ws_rate = ratelimit.rate_workspace(e, NP)
        self.claim = [_i32(NP) for _ in range(3)]        # workspaces of the mac1, consume and finish calls
        self.zero_overload = torch.zeros(NP, dtype=torch.uint8, device="cuda")
        self.zero_nonces = torch.zeros((NP, 24), dtype=torch.uint8, device="cuda")
        self.ka_desc = _dev(tn.desc_rows([(32 * k, 0, 0) for k in range(NP)]).view(np.uint8).reshape(-1, 16))
        # every output array, once
        o = self.o = {}
        o["peers_out"], o["slots_out"], o["gated_slots"] = _i32(NB), _i32(NB), _i32(NB)
        o["desc_out"], o["route_status"], o["send_dst"] = _u8(NB, 16), _u8(NB), _u8(NB, 24)
        o["send_status"], o["counters"], o["rekey"] = _u8(NB), _i64(NB), _u8(NB)
        o["status"], o["rcounters"], o["key_idx"], o["inner_len"] = _u8(NB), _i64(NB), _i32(NB), _i32(NB)
        o["ka_slots"], o["rekey_peers"], o["rekey_gate"], o["timer_counts"] = _i32(NP), _i32(NP), _u8(NP), _i32(2)
        o["ka_dst"], o["ka_status"], o["ka_counters"], o["ka_rekey"] = _u8(NP, 24), _u8(NP), _i64(NP), _u8(NP)
        o["init_peers"], o["init_gate"], o["expired"], o["turn_counts"] = _i32(NP), _u8(NP), _u8(NP), _i32(2)
        o["dst"], o["cookies"], o["has_cookie"], o["initiate_status"] = _u8(NP, 24), _u8(NP, 16), _u8(NP), _u8(NP)
        o["batch"], o["install_status"], o["installed"] = _u8(NP, 128), _u8(NP), _i32(NP)
        o["consume_status"], o["cookies_out"], o["filter_status"], o["finish_status"] = _u8(NP), _u8(NP, 16), _u8(NP), _u8(NP)
        o["pend_idx"], o["remote"], o["transport_keys"], o["rows_out"] = _i32(NP), _i32(NP), _u8(NP, 64), _i32(NP)
        o["reset"], o["rate_counts"], o["overload"] = _i32(1), _i32(NP), _u8(NP)
        o["init_status"], o["results"], o["resp_status"] = _u8(NP), _u8(NP, 128), _u8(NP)
        o["session_expired"], o["scratch_replies"], o["peers_out_hs"] = _u8(NK), _u8(NP, 64), _i32(NP)
        # every input a chain takes from its caller, staged here before the chain
        z = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device="cuda")  # noqa: E731
        self.i = dict(desc=z(NB, 16), sdesc=z(NB, 16), src=z(NB, 24), hdesc=z(NP, 16), cdesc=z(NP, 16), addrs=z(NP, 24), esk=z(NP, 32),
                      ts=z(NP, 12), sids=torch.zeros(NP, dtype=torch.int32, device="cuda"), nonces=z(NP, 24),
                      seeds=z(tn.rl.DEPTH, 16))

    # -- the network's three moves, on the device
    def copy_from(self, dst, doff, node, src, soff, length):
        self.arr[dst][doff:doff + length].copy_(node.arr[src][soff:soff + length])

    def xor(self, name, off, value):
        self.arr[name][off:off + 1] ^= value

    def put(self, name, off, data):
        self.arr[name][off:off + len(data)].copy_(_bytes_dev(data))

    def stage(self, **values):
        """the caller's inputs of a chain -> their arrays on the device (the first rows of each)"""
        for k, v in values.items():
            if k in ("esk", "ts", "nonces"):
                v = np.frombuffer(b"".join(v), np.uint8)
            elif k == "sids":
                v = np.array(v, np.uint32).view(np.int32)
            elif k == "seeds":
                v = np.array(v, np.uint64).view(np.uint8)
            else:
                v = np.ascontiguousarray(v).view(np.uint8)
            t = self.i[k]
            t.view(-1)[:v.size].copy_(_dev(v.reshape(-1)))

    def _begin(self, now, *names):
        self.now.copy_(_dev(np.array([now], np.uint64).view(np.int64)))
        for k in names:
            t = self.o[k] if k in self.o else self.arr[k]
            t.fill_(FILL if t.dtype == torch.uint8 else FILL32 if t.dtype == torch.int32 else FILL64)

    def _out(self, names, n=None, **rename):
        torch.cuda.synchronize()
        out = {}
        for k in names:
            t = self.o[k] if k in self.o else self.arr[k]
            out[rename.get(k, k)] = _host(t if n is None or k in self.arr else t[:n])
        return out

    def tables(self):
        torch.cuda.synchronize()
        S, P, R = self.ST, self.PT, self.RT
        t = dict(peer_state=self.pstate, send_keys=S.send_keys, recv_keys=S.recv_keys, receivers=S.receivers,
                 local_ids=S.local_ids, slot_peer=S.slot_peer, windows=S.windows, send_state=S.send_state,
                 peer_slot=S.peer_slot, timers=self.tm, pending=P.pending, pending_timers=P.timers, hs_ids=P.hs_ids,
                 endpoints=self.EP.endpoints, endpoint_claim=self.EP.claim, buckets=R.buckets, seeds=R.seeds,
                 last_reset_ns=R.last_reset_ns)
        t = {k: _host(v) for k, v in t.items()}
        t["rx_lookup"] = (S.rx_table.cpu().numpy().view(np.uint32).reshape(-1, 2).copy(), S.rx_cap)
        t["pend_lookup"] = (P.pend_table.cpu().numpy().view(np.uint32).reshape(-1, 2).copy(), P.pend_cap)
        return t

    # ------------------------------------------------------------- transport
    SEND = ("peers_out", "slots_out", "desc_out", "route_status", "gated_slots", "send_dst", "send_status", "counters", "rekey")

    def send(self, now, desc, plain):
        self._begin(now, *self.SEND)
        self.arr["tx"].copy_(_dev(plain))
        self.stage(sdesc=desc)
        self.send_chain(len(desc))
        return self._out(self.SEND + ("tx",), len(desc), send_dst="dst")

    def send_chain(self, n, stream=None):
        e, o, S, d = self.engine, self.o, self.ST, self.i["sdesc"][:n]
        route.route_batch_dev(e, self.rtable, S.peer_slot, d, self.arr["tx"], o["slots_out"][:n], o["desc_out"][:n],
                              o["route_status"][:n], peers_out=o["peers_out"][:n], stream=stream)
        self.EP.gate_batch_dev(S.slot_peer, o["slots_out"][:n], o["gated_slots"][:n], o["send_dst"][:n], stream=stream)
        e.send_batch_dev_resident(S.send_keys, S.receivers, S.send_state, o["gated_slots"][:n], o["desc_out"][:n],
                                  self.arr["tx"], o["send_status"][:n], counters_out=o["counters"][:n],
                                  rekey_out=o["rekey"][:n], now_ns=self.now, workspace=self.ws_s, stream=stream)
        timers.note_send_batch_dev(e, self.tm, o["gated_slots"][:n], o["send_status"][:n], o["rekey"][:n], self.now,
                                   stream=stream)

    RECV = ("status", "rcounters", "key_idx", "inner_len")

    def receive(self, now, desc, src):
        self._begin(now, *self.RECV)
        self.stage(desc=desc, src=src)
        self.receive_chain(len(desc))
        return self._out(self.RECV + ("rx",), len(desc), rcounters="counters")

    def receive_chain(self, n, stream=None):
        e, o, S = self.engine, self.o, self.ST
        d, s, rx = self.i["desc"][:n], self.i["src"][:n], self.arr["rx"]
        e.recv_batch_dev_resident(S.recv_keys, S.rx_table, S.windows, d, rx, o["status"][:n], o["rcounters"][:n],
                                  o["key_idx"][:n], workspace=self.ws_r, stream=stream)
        self.EP.note_recv_batch_dev(S.slot_peer, o["key_idx"][:n], o["status"][:n], s, stream=stream)
        timers.note_recv_batch_dev(e, self.tm, S.send_state, o["key_idx"][:n], o["status"][:n], self.now, stream=stream)
        route.route_check_batch_dev(e, self.rtable, S.slot_peer, d, o["key_idx"][:n], rx, o["status"][:n],
                                    o["inner_len"][:n], stream=stream)

    # ------------------------------------------------------------ initiator
    START = ("init_peers", "init_gate", "expired", "turn_counts", "dst", "cookies", "has_cookie", "initiate_status", "msgs",
             "batch", "install_status", "installed")

    def _start(self, req_peers, req_status, match, fresh):
        e, o, P = self.engine, self.o, self.PT
        esk, ts, sids, msgs = self.i["esk"], self.i["ts"], self.i["sids"], self.arr["msgs"].view(NP, 160)
        pending.turn_dev(e, P, self.now, o["init_peers"], o["init_gate"], o["turn_counts"], start_peers=req_peers,
                         start_status=req_status, start_match=match, expired_out=o["expired"], workspace=self.ws_p)
        self.EP.peers_batch_dev(o["init_peers"], o["init_peers"], o["dst"])
        e.peer_cookies_dev(self.pstate, o["init_peers"], o["cookies"], o["has_cookie"])
        e.handshake_initiate_dev(self.own, self.peers, o["init_peers"], o["init_gate"], esk, ts, sids, o["cookies"],
                                 o["has_cookie"], msgs, o["batch"], o["initiate_status"])
        e.peer_mac1_dev(self.pstate, o["init_peers"], o["initiate_status"], msgs, 160, 116, self.claim[0])
        pending.install_dev(e, P, o["batch"], o["initiate_status"], self.now, o["install_status"], o["installed"],
                            workspace=self.ws_p)

    def start(self, now, fresh):
        self._begin(now, *self.START)
        self.stage(**fresh)
        self._start(self.o["peers_out"], self.o["route_status"], tn.REJECTED, fresh)
        return self._out(self.START)

    TURN = ("ka_slots", "rekey_peers", "rekey_gate", "timer_counts", "ka_dst", "ka_status", "ka_counters", "ka_rekey", "ka_buf")

    def timer_turn(self, now, fresh):
        e, o, S = self.engine, self.o, self.ST
        self._begin(now, *(self.TURN + self.START))
        self.stage(**fresh)
        timers.turn_dev(e, S, self.tm, self.now, o["ka_slots"], o["rekey_peers"], o["rekey_gate"], o["timer_counts"],
                        workspace=self.ws_t)
        self.EP.gate_batch_dev(S.slot_peer, o["ka_slots"], o["ka_slots"], o["ka_dst"])
        e.send_batch_dev_resident(S.send_keys, S.receivers, S.send_state, o["ka_slots"], self.ka_desc, self.arr["ka_buf"],
                                  o["ka_status"], counters_out=o["ka_counters"], rekey_out=o["ka_rekey"], now_ns=self.now,
                                  workspace=self.ws_s)
        timers.note_send_batch_dev(e, self.tm, o["ka_slots"], o["ka_status"], o["ka_rekey"], self.now)
        self._start(o["rekey_peers"], o["rekey_gate"], tn.OK, fresh)
        return self._out(self.TURN + self.START)

    RESP = ("consume_status", "cookies_out", "filter_status", "finish_status", "pend_idx", "remote", "transport_keys",
            "install_status", "rows_out")

    def handle_responses(self, now, rdesc, cdesc, addrs):
        e, o, P = self.engine, self.o, self.PT
        self._begin(now, *self.RESP)
        self.stage(hdesc=rdesc, cdesc=cdesc, addrs=addrs)
        rd, cd, a = self.i["hdesc"], self.i["cdesc"], self.i["addrs"]
        e.peer_cookie_consume_dev(self.pstate, self.peer_cookie_keys, P.pend_table, cd, None, self.arr["cookie_in"],
                                  o["cookies_out"], self.claim[1], o["consume_status"])
        e.cookie_reply_dev(self.ck, rd, a, self.zero_overload, self.zero_nonces, self.arr["resp_in"], o["scratch_replies"],
                           o["filter_status"])
        e.handshake_finish_dev(self.own, self.peers, P.pend_table, P.pending, rd, o["filter_status"], self.arr["resp_in"],
                               o["transport_keys"], o["pend_idx"], o["remote"], self.claim[2], o["finish_status"])
        self.EP.note_finish_batch_dev(o["pend_idx"], P.peers, o["finish_status"], a)
        session.install_finish_batch_dev(e, self.ST, o["finish_status"], o["pend_idx"], o["remote"], P.hs_ids, P.peers,
                                         o["transport_keys"], o["install_status"], o["rows_out"], now_ns=self.now,
                                         workspace=self.ws_sess)
        timers.arm_batch_dev(e, self.tm, o["rows_out"], o["install_status"], self.now, tc.REKEY_NS)
        return self._out(self.RESP)

    # ------------------------------------------------------------ responder
    INIT = ("reset", "rate_counts", "overload", "filter_status", "replies", "init_status", "results", "peers_out_hs", "cookies",
            "has_cookie", "resp_status", "responses", "transport_keys", "install_status", "rows_out")

    def handle_initiations(self, now, desc, addrs, fresh):
        e, o = self.engine, self.o
        self._begin(now, *self.INIT)
        self.stage(hdesc=desc, addrs=addrs, **fresh)
        d, a, buf, i = self.i["hdesc"], self.i["addrs"], self.arr["hs_in"], self.i
        seeds, nonces, esk, sids = i["seeds"], i["nonces"], i["esk"], i["sids"]
        replies, responses = self.arr["replies"].view(NP, 64), self.arr["responses"].view(NP, 96)
        ratelimit.turn_dev(e, self.RT, self.now, seeds, o["reset"])
        ratelimit.count_dev(e, self.RT, d, a, buf, o["overload"], counts_out=o["rate_counts"], workspace=self.ws_rate)
        e.cookie_reply_dev(self.ck, d, a, o["overload"], nonces, buf, replies, o["filter_status"])
        e.handshake_init_dev(self.own, self.peers, self.peer_table, d, o["filter_status"], buf, o["results"], o["init_status"])
        e.peer_ts_dev(self.pstate, o["results"], o["init_status"], o["peers_out_hs"], workspace=self.ws_ts)
        e.peer_cookies_dev(self.pstate, o["peers_out_hs"], o["cookies"], o["has_cookie"])
        e.handshake_resp_dev(self.peers, o["results"], o["init_status"], esk, sids, o["cookies"], o["has_cookie"], responses,
                             o["transport_keys"], o["resp_status"])
        e.peer_mac1_dev(self.pstate, o["peers_out_hs"], o["resp_status"], responses, 96, 60, self.claim[0])
        session.install_resp_batch_dev(e, self.ST, o["resp_status"], sids, o["results"], o["transport_keys"],
                                       o["install_status"], o["rows_out"], now_ns=self.now, workspace=self.ws_sess)
        timers.arm_batch_dev(e, self.tm, o["rows_out"], o["install_status"], self.now, 0)
        return self._out(self.INIT, peers_out_hs="peers_out")

    def expire(self, now):
        self._begin(now, "session_expired")
        session.expire_batch_dev(self.engine, self.ST, now_ns=self.now, expired_out=self.o["session_expired"],
                                 workspace=self.ws_sess)
        return self._out(("session_expired",), session_expired="expired")


# ---------------------------------------------------------------- comparing
def lookup_differs(got, want, stale_ok=None):
    """a receiver table against the ids it must answer: every live id finds its row, and nothing else is in it.
    stale_ok, for pend_table alone, is the model's pending rows: include/rg_aead.h ("device-resident pending
    handshakes", rg_pending_tables) lets an entry that names a wiped row (peer = RG_PEER_NONE) stay until the next
    rebuild, where it answers RG_PKT_REJECTED; any other entry that is not a live id's is a difference"""
    table, cap = got
    find = _lib.lib().rg_rx_table_find
    ptr = table.ctypes.data_as(ctypes.c_void_p)
    bad = [(hex(i), r, int(find(ptr, cap, i))) for i, r in want.items() if find(ptr, cap, i) != r]
    used = [(int(i), int(r)) for i, r in table[table[:, 1] != tn.NONE]]
    if stale_ok is not None:   # an entry may stay until the next rebuild if the row it names is wiped now
        used = [u for u in used if u in want.items() or not (u[1] < NP and stale_ok[128 * u[1] + 96:128 * u[1] + 100] == b"\xff" * 4)]
    if sorted(used) != sorted(want.items()):
        bad.append(("occupied", sorted(used)[:4], sorted(want.items())[:4]))
    return bad


def differences(got, want, where):
    out = []
    assert set(got) == set(want), (where, set(got) ^ set(want))
    for k in want:
        if isinstance(want[k], dict):
            bad = lookup_differs(got[k], want[k], stale_ok=want["pending"] if k == "pend_lookup" else None)
            if bad:
                out.append((where, k, bad[:4]))
        elif got[k] != want[k]:
            g, w = np.frombuffer(got[k], np.uint8), np.frombuffer(want[k], np.uint8)
            if len(g) != len(w):
                out.append((where, k, "length", len(g), len(w)))
            else:
                at = np.flatnonzero(g != w)
                out.append((where, k, f"{len(at)} bytes differ, first at {int(at[0])}",
                            g[at[0]:at[0] + 8].tobytes().hex(), w[at[0]:at[0] + 8].tobytes().hex()))
    return out


def compare(nodes, out, wout, wtables, where):
    diffs = differences(out, wout, where + " outputs")
    for nm, nd in nodes.items():
        diffs += differences(nd.tables(), wtables[nm], f"{where} tables of {nm}")
    return diffs


def run_against_model(engine, seed):
    """every tick on the device nodes, compared with the model behind every chain; asserts at the end of each tick.
    -> the device nodes"""
    log, _ = tn.model_run(seed)
    nodes = tn.make_nodes(seed, DeviceNode, engine=engine)
    want, tick, diffs = iter(log), 0, []
    for ti, si, now, s, out in tn.play(tn.schedule(seed), nodes):
        if ti != tick:
            assert not diffs, (f"tick {tick}", len(diffs), diffs[:12])
            tick, diffs = ti, []
        wti, wsi, _, op, name, wout, wtables = next(want)
        assert (wti, wsi, op, name) == (ti, si, s["op"], s["node"])
        diffs += compare(nodes, out, wout, wtables, f"tick {ti} step {si} {name}.{op}")
    assert not diffs, (f"tick {tick}", len(diffs), diffs[:12])
    return nodes


def model_after(seed):
    """the model nodes behind the whole lifetime, a copy the caller may run further"""
    return copy.deepcopy(tn.model_run(seed)[1])


@pytest.mark.parametrize("seed", (1, 2))
def test_tunnel_lifetime_matches_model(engine, seed):
    """cold start with a lost response, two handshakes that finish in one batch, an ephemeral of small order, a cookie
    round trip under load and a retry that carries mac2; traffic both ways with forged, replayed, misaligned, unknown
    and handshake frames, roaming and a source of another peer; keepalives after silence; a rekey of three rows with
    a lost response, a retry and a replayed initiation; expiry of the old rows and reaped pending rows: every output
    byte and every table byte of every node equals the model's behind every chain of every tick"""
    run_against_model(engine, seed)


def transport_tick(b, now):
    """B's packets to A, then A's receive and A's send of 63 packets each"""
    b.tick(now)
    b.send("B", 63, [tn.NET_A + 9], tn.NET_B)
    b.deliver("B", "A", [("tx", i) for i in range(63)])
    b.send("A", 63, [tn.NET_B + 7, tn.rt.ip(10, 3, 0, 1), tn.rt.ip(10, 7, 0, 1)], tn.NET_A)


def test_tunnel_transport_tick_captured(engine):
    """behind the lifetime, a steady-state tick of A -- the receive chain, then the send chain -- runs once eagerly,
    is captured into one graph on one stream (no branches: every call is enqueued behind the one before) and replayed
    on the next tick's inputs and clock; a third tick runs eagerly again.  Every tick equals the model: outputs and
    every table of every node"""
    seed = 1
    nodes, model = run_against_model(engine, seed), model_after(seed)
    b = tn.Builder(seed + 200)
    t = tn.schedule(seed)[-1][0]
    for k in range(3):
        transport_tick(b, t + (k + 1) * tn.SEC)
    want = [(s, {k: tn.as_bytes(v) for k, v in out.items()}, {nm: nd.tables() for nm, nd in model.items()})
            for _, _, _, s, out in tn.play(b.ticks, model)]
    A, n, graph = nodes["A"], 63, None
    for k, (now, steps) in enumerate(b.ticks):
        w = iter(want[3 * k:3 * k + 3])
        if k != 1:
            for ti, si, _, s, out in tn.play([(now, steps)], nodes):
                ws, wout, wtables = next(w)
                diffs = compare(nodes, out, wout, wtables, f"tick {k} {s['node']}.{s['op']}")
                assert not diffs, diffs[:12]
            if k == 0:
                stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
                torch.cuda.synchronize()
                with torch.cuda.graph(graph, stream=stream):
                    A.receive_chain(n, stream=stream)
                    A.send_chain(n, stream=stream)
                torch.cuda.synchronize()
            continue
        # the captured tick: B's send and the network eagerly; A's inputs staged; one replay runs both chains
        recv_step, send_step = steps[-2], steps[-1]
        for ti, si, _, s, out in tn.play([(now, steps[:-2])], nodes):
            ws, wout, wtables = next(w)
            assert not compare(nodes, out, wout, wtables, "tick 1 B.send")
        A._begin(now, *(A.RECV + A.SEND))
        A.arr["tx"].copy_(_dev(send_step["plain"]))
        A.stage(desc=recv_step["desc"], src=recv_step["src"], sdesc=send_step["desc"])
        torch.cuda.synchronize()
        graph.replay()
        (_, w_recv, _), (_, w_send, wtables) = next(w), next(w)
        diffs = differences(A._out(A.RECV + ("rx",), n, rcounters="counters"), w_recv, "captured A.receive outputs")
        diffs += compare(nodes, A._out(A.SEND + ("tx",), n, send_dst="dst"), w_send, wtables, "captured A.send")
        assert not diffs, diffs[:12]


RATE = ("buckets", "seeds", "last_reset_ns")


def test_tunnel_tables_survive_a_quiet_turn(engine):
    """behind the whole lifetime, at the last tick's own clock (so that no timer, retry or expiry is newly due), every
    chain of every node runs with nothing in it: a packet for nobody, a frame of an unknown receiver, no request,
    every handshake, response and cookie row RG_KEY_SKIP.  No byte of any table of any node changes, and the model
    says the same.  One exemption: the rate sketch (buckets, seeds, last_reset_ns), whose timed reset is due at
    every responder that has not seen an initiation for a period; it is compared with the model's instead"""
    seed = 1
    nodes, model = run_against_model(engine, seed), model_after(seed)
    b = tn.Builder(seed + 100)
    b.tick(tn.schedule(seed)[-1][0])
    for nm in tn.NODES:
        b.send(nm, 1, [tn.rt.ip(11, 0, 0, 1)], tn.NET_A)
        b.add("start", nm, fresh=b.initiator_fresh())
        b.add("timer_turn", nm, fresh=b.initiator_fresh())
        b.initiations("A", nm, [None] * NP)
        b.responses(nm)
        b.deliver("A", nm, [("raw", (4).to_bytes(4, "little") + (0xDEAD).to_bytes(4, "little") + bytes(40))])
        b.add("expire", nm)
    before = {nm: nd.tables() for nm, nd in nodes.items()}
    before_model = {nm: nd.tables() for nm, nd in model.items()}
    for _ in tn.play(b.ticks, model):
        pass
    after_model = {nm: nd.tables() for nm, nd in model.items()}
    for nm in model:    # a condition on the inputs: they are quiet
        assert all(before_model[nm][k] == after_model[nm][k] for k in before_model[nm] if k not in RATE), nm
    for _ in tn.play(b.ticks, nodes):
        pass
    for nm, nd in nodes.items():
        after = nd.tables()
        for k, v in before[nm].items():
            same = (v[0] == after[k][0]).all() if isinstance(v, tuple) else after[k] == (after_model[nm][k] if k in RATE else v)
            assert same, (nm, k)
