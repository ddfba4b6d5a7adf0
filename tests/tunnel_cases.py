"""Whole nodes on one virtual clock: the model node and the schedule of tests/test_tunnel_cpu.py and
tests/test_gpu_tunnel.py.

The world is test_gpu_pending.py's `World` with every party a whole node: A knows the other side as three peer rows,
each a responder (B, B3, B5) with a key pair, tables and chains of its own, so A's lists hold several real entries
and pads (two handshakes finish in one batch, three rows rekey in one turn).  The mirror image, one responder that
knows A as several rows, is not built: a public key can sit in one peer row only (rg_peer_table_build refuses a
duplicate), and a node has one key pair, so each responder knows A as one row and its handshake batches hold one
finishing row (two real rows where an initiation is replayed).

`ModelNode` holds every table a node keeps as Python / numpy values and has one method per chain of INTEGRATION.md
§4, each of them the existing per-module models (`*_cases.py`) called in the order the chain is written there.  It
is the only source of expected values: nothing here is computed a second way.  `schedule(seed)` is one tunnel
lifetime as a list of ticks `(now_ns, steps)`; `play` runs a schedule over any pair of nodes with the same methods
(the model's here, the device's in test_gpu_tunnel.py), moving bytes between them, and yields every chain's outputs.

Conventions shared with the device node, so that every output array can be compared byte for byte:
  * every output array of a chain starts the chain filled with FILL; a byte no call writes stays FILL;
  * a node's wire arrays (`tx`, `ka_buf`, `msgs`, `responses`, `replies` out; `rx`, `hs_in`, `resp_in`, `cookie_in`
    in, `held` for frames kept in flight) have fixed sizes and frames sit at fixed strides;
  * whatever a caller supplies (ephemeral keys, session ids, cookie nonces, rate seeds, timestamps, payloads) is
    drawn by `schedule` from one seeded generator, in the order of the ticks.
"""
from __future__ import annotations

import functools

import numpy as np

import endpoint_cases as ec
import handshake_cases as hc
import initiator_cases as ic
import peerstate_cases as psc
import pending_cases as pc
import ratelimit_cases as rl
import replay_cases as rc
import route_cases as rt
import send_cases as sendc
import session_cases as sc
import timer_cases as tc
from conftest import load_golden
from oracle import oracle

OK, DECRYPT_ERR, INVALID, REJECTED, UNALIGNED, NOT_DATA, PENDING, COOKIE, KEYEXCHANGE, UNROUTABLE, FULL = range(11)
NONE = SKIP = 0xFFFFFFFF
FILL = 0xA5
NP, NK, NB = 8, 32, 257          # peers a node, session rows, frames a data batch
STRIDE = 16 + 1504 + 16          # a frame slot: header, the longest padded inner packet, tag
SEC = 10**9
DESC = rt.DESC_DTYPE
SIZES = dict(tx=NB * STRIDE, rx=NB * STRIDE, held=NB * STRIDE, ka_buf=NP * 32, msgs=NP * 160, responses=NP * 96,
             replies=NP * 64, hs_in=NP * 160, resp_in=NP * 96, cookie_in=NP * 64)
DATA_BATCHES = (1, 63, 65, 257)


def fill(n, width=None, dtype=np.uint8):
    a = np.full(n if width is None else (n, width), FILL, np.uint8)
    return a if dtype == np.uint8 else np.full(n, int.from_bytes(bytes([FILL]) * np.dtype(dtype).itemsize, "little"), dtype)


def desc_rows(rows):
    return np.array(rows, DESC) if len(rows) else np.zeros(0, DESC)


# ------------------------------------------------------------------ the node
class Config:
    """what a node is configured with: its key pair, its peer rows, its AllowedIPs, the peers' configured endpoints
    and its cookie secret"""

    def __init__(self, sk, peers, routes, endpoints, secret):
        self.sk, self.pk = sk, hc.pubkey(sk)
        self.peers = [(pk, psk, hc.mac1_key(pk)) for pk, psk in peers]
        self.routes = routes                      # rows (net, prefix length, peer) of route_cases
        self.endpoints = endpoints                # {peer: rg_src_addr bytes}
        self.cookie_keys = hc.mac1_key(self.pk) + psc.cookie_key(self.pk) + secret      # rg_cookie_keys
        self.peer_cookie_keys = [psc.cookie_key(pk) for pk, _ in peers]

    def endpoint_rows(self):
        t = np.zeros((NP, ec.ROW), np.uint8)
        for p, a in self.endpoints.items():
            t[p] = np.frombuffer(ec.some_row(a), np.uint8)
        return t


class ModelNode:
    def __init__(self, name, cfg: Config):
        self.name, self.cfg = name, cfg
        self.pstate = [bytes(psc.ROW)] * NP
        self.sess = sc.empty_tables(NK, NP)
        self.timers = [(0, 0, 0)] * NK
        self.pend = pc.empty_table(NP)
        self.ep = cfg.endpoint_rows()
        self.sketch = rl.new_sketch()
        self.arr = {k: np.full(v, FILL, np.uint8) for k, v in SIZES.items()}
        self.last_route = (fill(NB, dtype=np.uint32), fill(NB))   # the last send's peers_out and route status
        self.cov = []                                             # (event, detail): what the coverage checks read

    # -- the network's three moves
    def copy_from(self, dst, doff, node, src, soff, length):
        self.arr[dst][doff:doff + length] = node.arr[src][soff:soff + length]

    def xor(self, name, off, value):
        self.arr[name][off] ^= value

    def put(self, name, off, data):
        self.arr[name][off:off + len(data)] = np.frombuffer(bytes(data), np.uint8)

    # -- the tables, as bytes
    def tables(self):
        s, u32, u64 = self.sess, lambda v: np.array(v, np.uint32).tobytes(), lambda v: np.array(v, np.uint64).tobytes()  # noqa: E731
        return dict(
            peer_state=b"".join(self.pstate), send_keys=b"".join(s["send_keys"]), recv_keys=b"".join(s["recv_keys"]),
            receivers=u32(s["receivers"]), local_ids=u32(s["local_ids"]), slot_peer=u32(s["slot_peer"]),
            windows=b"".join(s["windows"]), send_state=u64(s["send_state"]), peer_slot=u32(s["peer_slot"]),
            timers=b"".join(int(a).to_bytes(8, "little") + int(f).to_bytes(4, "little") + int(p).to_bytes(4, "little")
                            for a, f, p in self.timers),
            pending=b"".join(self.pend["pending"]), pending_timers=u64(self.pend["timers"]), hs_ids=u32(self.pend["hs_ids"]),
            endpoints=self.ep.tobytes(), endpoint_claim=bytes(4 * NP),
            buckets=u32(self.sketch["buckets"]), seeds=u64(self.sketch["seeds"]), last_reset_ns=u64([self.sketch["last_reset_ns"]]),
            rx_lookup=sc.rx_pairs(s), pend_lookup=pc.lookup(self.pend))

    # ------------------------------------------------------------- transport
    def _send_resident(self, now, slots, desc, buf):
        """rg_send_batch_dev_resident: send_cases.loop, then the oracle's seal of every packet that took a counter"""
        state = np.array(self.sess["send_state"], np.uint64).reshape(NK, 3)
        status, ctrs, rekey, state = sendc.loop(state, slots, desc["len"], now)
        took = np.flatnonzero(status == PENDING)
        if len(took):
            work = desc[took].copy()
            work["key_idx"] = np.array(slots, np.uint32)[took]
            keys = np.frombuffer(b"".join(self.sess["send_keys"]), np.uint8).reshape(NK, 32)
            oracle.seal_batch(keys, np.array(self.sess["receivers"], np.uint32), work, ctrs[took], buf)
            status[took] = OK
        self.sess["send_state"] = [tuple(int(x) for x in r) for r in state]
        self.timers = tc.note_send_loop(self.timers, slots, status, rekey, now)
        return status, ctrs, rekey

    def send(self, now, desc, plain):
        """rg_route_batch_dev -> rg_endpoint_gate_batch_dev -> rg_send_batch_dev_resident -> rg_timer_note_send_batch_dev"""
        n, s = len(desc), self.sess
        self.arr["tx"][:] = plain
        peers, slots, desc_out, rstatus, buf = rt.route_model(self.cfg.routes, s["peer_slot"], desc, self.arr["tx"])
        gslots, dst = ec.gate_loop(self.ep, s["slot_peer"], slots)
        status, ctrs, rekey = self._send_resident(now, gslots, desc_out, buf)
        self.arr["tx"] = buf
        self.last_route = (fill(NB, dtype=np.uint32), fill(NB))
        self.last_route[0][:n], self.last_route[1][:n] = peers, rstatus
        self.cov.append(("send", dict(route=list(rstatus), send=list(status), slots=list(slots), gated=gslots, peers=list(peers))))
        return dict(peers_out=peers, slots_out=slots, desc_out=desc_out, route_status=rstatus,
                    gated_slots=np.array(gslots, np.uint32), dst=dst, send_status=status, counters=ctrs, rekey=rekey, tx=buf)

    def receive(self, now, desc, src):
        """rg_recv_batch_dev_resident -> rg_endpoint_note_recv_batch_dev -> rg_timer_note_recv_batch_dev ->
        rg_route_check_batch_dev"""
        s, buf = self.sess, self.arr["rx"]
        live = [r for r in range(NK) if s["slot_peer"][r] != NONE]
        keys = np.frombuffer(b"".join(s["recv_keys"][r] for r in live) or bytes(32), np.uint8).reshape(-1, 32)
        ids = [s["local_ids"][r] for r in live] or [0xFFFFFFFE]
        opened = buf.copy()
        st, ctr, k = oracle.open_batch_rx(keys, ids, desc, opened)
        kidx = np.array([live[int(x)] if int(x) < len(live) else SKIP for x in k], np.uint32)
        windows = np.frombuffer(b"".join(s["windows"]), np.uint64).reshape(NK, 33)
        fin, _, W, cls = rc.host_commit(windows, kidx, ctr, st)
        for i, d in enumerate(desc):
            if fin[i] == OK:
                o, w = int(d["offset"]), int(d["len"])
                buf[o:o + w] = opened[o:o + w]
        s["windows"] = [W[r].tobytes() for r in range(NK)]
        before = self.ep.copy()
        self.ep = ec.note_loop(self.ep, ec.recv_peers(s["slot_peer"], kidx), fin, src)
        self.timers = tc.note_recv_loop(self.timers, s["send_state"], kidx, fin, now)
        status, inner = rt.check_model(self.cfg.routes, s["slot_peer"], desc, kidx, buf, fin)
        self.cov.append(("receive", dict(recv=list(fin), final=list(status), key_idx=list(kidx), classes=cls,
                                         moved=[p for p in range(NP) if before[p].tobytes() != self.ep[p].tobytes()],
                                         roamed=[p for p in range(NP) if ec.is_some(before[p]) and
                                                 before[p].tobytes() != self.ep[p].tobytes()])))
        return dict(status=status, counters=ctr, key_idx=kidx, inner_len=inner, rx=buf)

    # ------------------------------------------------------------ initiator
    def _start(self, now, req_peers, req_status, match, fresh):
        """rg_pending_turn_dev -> rg_endpoint_peers_batch_dev (in place) -> rg_peer_cookies_batch_dev ->
        rg_handshake_initiate_batch_dev -> rg_peer_mac1_batch_dev -> rg_pending_install_batch_dev, each n = NP"""
        cfg = self.cfg
        before = [pc.is_live(self.pend, p) for p in range(NP)]
        self.pend, init, gate, expired, counts = pc.turn_loop(self.pend, now, req_peers, req_status, match)
        retried = [p for p in init if p != NONE and before[p]]
        init_g, dst = ec.peers_loop(self.ep, init)
        cookies, has = psc.gather(self.pstate, init_g)
        status, msgs, batch = fill(NP), fill(NP, 160), [bytes([FILL]) * pc.ROW] * NP
        for i in range(NP):
            if gate[i] != OK:
                status[i] = REJECTED
                continue
            st, msg, row = ic.initiate(cfg.sk, cfg.peers, init_g[i], fresh["esk"][i], fresh["ts"][i], fresh["sids"][i],
                                       cookies[i] if has[i] else None)
            status[i], msgs[i], batch[i] = st, np.frombuffer(msg, np.uint8), row
        self.pstate = psc.record_loop(self.pstate, init_g, list(status), [m.tobytes() for m in msgs], 116)
        self.pend, batch, st_inst, installed = pc.install_loop(self.pend, batch, list(status), now)
        self.arr["msgs"] = msgs.reshape(-1).copy()
        self.cov.append(("start", dict(init=init, gated=init_g, status=list(status), retried=retried, expired=expired,
                                       mac2=[i for i in range(NP) if status[i] == OK and has[i]])))
        return dict(init_peers=np.array(init_g, np.uint32), init_gate=np.array(gate, np.uint8),
                    expired=np.array(expired, np.uint8), turn_counts=np.array(counts, np.uint32), dst=dst,
                    cookies=np.frombuffer(b"".join(cookies), np.uint8), has_cookie=np.array(has, np.uint8),
                    initiate_status=status, msgs=msgs, batch=np.frombuffer(b"".join(batch), np.uint8),
                    install_status=np.array(st_inst, np.uint8), installed=np.array(installed, np.uint32))

    def start(self, now, fresh):
        """the peers whose packets found no session: the last send's peers_out with its route status, start_match =
        RG_PKT_REJECTED"""
        return self._start(now, [int(p) for p in self.last_route[0]], [int(x) for x in self.last_route[1]], REJECTED, fresh)

    def timer_turn(self, now, fresh):
        """rg_timer_turn_dev, then the keepalive chain (gate in place -> resident send over the fixed {32 k, 0}
        descriptors -> note) and the rekey list through the start-and-retry chain"""
        s = self.sess
        self.timers, ka, rk, rk_gate, counts = tc.turn_loop(s, self.timers, now)
        ka_g, ka_dst = ec.gate_loop(self.ep, s["slot_peer"], ka)
        buf = fill(NP * 32)
        ka_desc = desc_rows([(32 * k, 0, 0) for k in range(NP)])
        status, ctrs, rekey = self._send_resident(now, ka_g, ka_desc, buf)
        self.arr["ka_buf"] = buf
        self.cov.append(("turn", dict(ka=ka, ka_gated=ka_g, ka_status=list(status), rekey=rk)))
        out = dict(ka_slots=np.array(ka_g, np.uint32), rekey_peers=np.array(rk, np.uint32),
                   rekey_gate=np.array(rk_gate, np.uint8), timer_counts=np.array(counts, np.uint32), ka_dst=ka_dst,
                   ka_status=status, ka_counters=ctrs, ka_rekey=rekey, ka_buf=buf)
        out.update(self._start(now, rk, rk_gate, OK, fresh))
        return out

    def handle_responses(self, now, rdesc, cdesc, addrs):
        """type-3 messages: rg_peer_cookie_consume_batch_dev over pend_table.  type-2 messages: the filter (mac1; the
        initiator's side is never overloaded here) -> rg_handshake_finish_batch_dev -> rg_endpoint_note_finish_batch_dev
        -> rg_session_install_finish_batch_dev -> rg_timer_arm_batch_dev(RG_REKEY_AFTER_TIME_NS)"""
        cfg, n = self.cfg, NP
        cbuf, rbuf = self.arr["cookie_in"], self.arr["resp_in"]
        cmsgs = [cbuf[int(d["offset"]):int(d["offset"]) + 64].tobytes() for d in cdesc]
        flags = [dict(key_skip=int(d["key_idx"]) == SKIP) for d in cdesc]
        self.pstate, c_status, c_out = psc.consume_loop(self.pstate, cfg.peer_cookie_keys, pc.lookup(self.pend), cmsgs, flags)
        rmsgs = [rbuf[int(d["offset"]):int(d["offset"]) + 92].tobytes() for d in rdesc]
        f_status, _ = self._filter(rdesc, rmsgs, addrs, [0] * n, None)
        flags = [dict(gated=f_status[i] != OK, key_skip=int(rdesc[i]["key_idx"]) == SKIP) for i in range(n)]
        st, keys, pidx, remote, pending = ic.commit(rmsgs, flags, pc.lookup(self.pend), self.pend["pending"], cfg.sk, cfg.peers)
        self.pend["pending"] = pending
        self.ep = ec.note_loop(self.ep, ec.recv_peers(list(range(NP)), pidx), st, addrs)
        lids, rids, peers = sc.gather_finish(st, pidx, remote, self.pend["hs_ids"], list(range(NP)))
        old = list(self.sess["peer_slot"])
        self.sess, st_sess, rows, keys = sc.install_loop(self.sess, st, lids, rids, peers, keys, now)
        self.timers = tc.arm_loop(self.timers, rows, st_sess, now, tc.REKEY_NS)
        self.cov.append(("responses", dict(consume=c_status, finish=st, install=st_sess, rows=rows,
                                           replaced=[p for p in range(NP) if old[p] != SKIP and self.sess["peer_slot"][p] != old[p]])))
        return dict(consume_status=np.array(c_status, np.uint8), cookies_out=np.frombuffer(b"".join(c_out), np.uint8),
                    filter_status=np.array(f_status, np.uint8), finish_status=np.array(st, np.uint8),
                    pend_idx=np.array(pidx, np.uint32), remote=np.array(remote, np.uint32),
                    transport_keys=np.frombuffer(b"".join(keys), np.uint8), install_status=np.array(st_sess, np.uint8),
                    rows_out=np.array(rows, np.uint32))

    # ------------------------------------------------------------ responder
    def _filter(self, desc, msgs, addrs, overload, nonces):
        """rg_cookie_reply_batch_dev by the header's table, for aligned frames inside the buffer"""
        ck = self.cfg.cookie_keys
        status, replies = [], fill(len(desc), 64)
        for i, (d, msg) in enumerate(zip(desc, msgs)):
            L = len(msg)
            if int(d["key_idx"]) == SKIP:
                status.append(REJECTED)
            elif msg[0:4] != (1 if L == 148 else 2).to_bytes(4, "little"):
                status.append(INVALID)
            elif oracle.blake2s(msg[:L - 32], ck[:32], 16) != msg[L - 32:L - 16]:
                status.append(REJECTED)
            elif not overload[i]:
                status.append(OK)
            else:
                cookie = oracle.blake2s(bytes(addrs[i][:18]), ck[64:96], 16)
                if oracle.blake2s(msg[:L - 16], cookie, 16) == msg[L - 16:]:
                    status.append(OK)
                else:
                    ct, tag = oracle.xaead_seal(ck[32:64], nonces[i], msg[L - 32:L - 16], cookie)
                    replies[i] = np.frombuffer((3).to_bytes(4, "little") + msg[4:8] + nonces[i] + ct + tag, np.uint8)
                    status.append(COOKIE)
        return status, replies

    def handle_initiations(self, now, desc, addrs, fresh):
        """rg_rate_turn_dev -> rg_rate_count_batch_dev -> rg_cookie_reply_batch_dev (overload = the count's flags) ->
        rg_handshake_init_batch_dev -> rg_peer_ts_batch_dev -> rg_peer_cookies_batch_dev -> rg_handshake_resp_batch_dev
        -> rg_peer_mac1_batch_dev -> rg_session_install_resp_batch_dev -> rg_timer_arm_batch_dev(0)"""
        cfg, n, buf = self.cfg, NP, self.arr["hs_in"]
        self.sketch, reset = rl.turn_loop(self.sketch, now, rl.PERIOD_NS, fresh["seeds"])
        drows = [(int(d["offset"]), int(d["len"]), int(d["key_idx"])) for d in desc]
        self.sketch, counts, overload = rl.count_loop(self.sketch, drows, [bytes(a) for a in addrs], buf.tobytes())
        msgs = [buf[o:o + ln].tobytes() for o, ln, _ in drows]
        f_status, replies = self._filter(desc, msgs, addrs, overload, fresh["nonces"])
        status, results = [], []
        for i in range(n):
            if f_status[i] != OK:
                st, row = REJECTED, hc.ZERO_ROW
            elif msgs[i][0:4] != (1).to_bytes(4, "little"):
                st, row = INVALID, hc.ZERO_ROW
            else:
                st, row = hc.consume_initiation(msgs[i], cfg.sk, [p[0] for p in cfg.peers])
            status.append(st)
            results.append(row)
        init_status = list(status)
        self.pstate, results, status, peers_out = psc.ts_loop(self.pstate, results, status)
        cookies, has = psc.gather(self.pstate, peers_out)
        r_status, responses, keys = fill(n), fill(n, 96), [bytes([FILL]) * 64] * n
        for i in range(n):
            if status[i] != OK:
                r_status[i] = REJECTED
                continue
            st, msg, key = hc.build_response(results[i], cfg.peers, fresh["esk"][i], fresh["sids"][i],
                                             cookies[i] if has[i] else None)
            r_status[i], responses[i], keys[i] = st, np.frombuffer(msg.ljust(96, b"\0"), np.uint8), key
            results[i] = bytes(64) + results[i][64:]
        self.pstate = psc.record_loop(self.pstate, peers_out, list(r_status), [r.tobytes() for r in responses], 60)
        lids, rids, peers = sc.gather_resp(fresh["sids"], results)
        self.sess, st_sess, rows, keys_after = sc.install_loop(self.sess, list(r_status), lids, rids, peers, keys, now)
        self.timers = tc.arm_loop(self.timers, rows, st_sess, now, 0)
        self.arr["responses"], self.arr["replies"] = responses.reshape(-1).copy(), replies.reshape(-1).copy()
        self.cov.append(("initiations", dict(filter=f_status, init=init_status, ts=list(status), resp=list(r_status),
                                             install=st_sess, overload=overload, keys=keys, responses=responses.copy())))
        return dict(reset=np.array([reset], np.uint32), rate_counts=np.array(counts, np.uint32),
                    overload=np.array(overload, np.uint8), filter_status=np.array(f_status, np.uint8), replies=replies,
                    init_status=np.array(status, np.uint8), results=np.frombuffer(b"".join(results), np.uint8),
                    peers_out=np.array(peers_out, np.uint32), cookies=np.frombuffer(b"".join(cookies), np.uint8),
                    has_cookie=np.array(has, np.uint8), resp_status=r_status, responses=responses,
                    transport_keys=np.frombuffer(b"".join(keys_after), np.uint8),
                    install_status=np.array(st_sess, np.uint8), rows_out=np.array(rows, np.uint32))

    def expire(self, now):
        """rg_session_expire_batch_dev(now_ns)"""
        self.sess, expired = sc.expire_loop(self.sess, now)
        self.cov.append(("expire", dict(expired=expired)))
        return dict(expired=np.array(expired, np.uint8))


# -------------------------------------------------------------- the schedule
ADDR_A, ADDR_A2, ADDR_A3 = ec.addr("192.0.2.1", 51820), ec.addr("192.0.2.77", 4000), ec.addr("2001:db8::a3", 4003)
ADDR = {"A": ADDR_A, "B": ec.addr("198.51.100.2", 51820), "B3": ec.addr("198.51.100.3", 51823),
        "B5": ec.addr("2001:db8::b5", 51825)}
ADDR_B = ADDR["B"]
ADDR_FLOOD = ec.addr("192.0.2.1", 9)     # the flood shares A's IP: the sketch is keyed by the address alone
ADDR_LOW = ec.addr("203.0.113.200", 7)   # whoever sends the initiation with an ephemeral of small order
# A's three tunnels: the responder's name, its row at A, A's row at it, its inner network
TUNNELS = (("B", 0, 2, rt.ip(10, 2, 0, 0)), ("B3", 3, 1, rt.ip(10, 3, 0, 0)), ("B5", 5, 6, rt.ip(10, 5, 0, 0)))
NODES = ("A",) + tuple(t[0] for t in TUNNELS)
PEER_B, PEER_A = 0, 2                     # B's row at A, A's row at B
NET_A, NET_B = rt.ip(10, 1, 0, 0), rt.ip(10, 2, 0, 0)
T0 = 1000 * SEC


@functools.lru_cache(maxsize=None)
def configs(seed):
    """Four key pairs: A, the initiator with the recorded static key of golden/handshake_full.json, knows the other
    side as three peer rows (0, 3, 5), each a responder with a key pair and a node of its own that knows A as one of
    its eight rows (test_gpu_pending.py's World, every party a whole node); B holds the recorded responder key, so
    that peer 0's first handshake is the recorded one.  A's peers 6 and 7 and B's peer 4 never answer: nobody holds
    their keys.  A's peer 7 has no endpoint, and no responder has one for A."""
    g = load_golden("handshake_full.json")["handshake"]
    rng = np.random.default_rng([seed, 1])
    rb = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
    sk_a, sk_b, psk = (bytes.fromhex(g[k]) for k in ("static_private_i", "static_private_r", "preshared_key"))
    others = lambda: [(hc.pubkey(rb(32)), rb(32)) for _ in range(NP)]  # noqa: E731
    peers_a, out = others(), {}
    routes_a = [(rt.ip(10, 6, 0, 0), 16, 6), (rt.ip(10, 7, 0, 0), 16, 7)]
    ends_a = {6: ec.addr("203.0.113.6", 1)}
    for name, at_a, a_at, net in TUNNELS:
        sk, key = (sk_b, psk) if name == "B" else (rb(32), rb(32))
        peers = others()
        peers[a_at], peers_a[at_a] = (hc.pubkey(sk_a), key), (hc.pubkey(sk), key)
        routes, ends = [(NET_A, 16, a_at)], {}
        if name == "B":
            routes, ends = routes + [(rt.ip(10, 4, 0, 0), 16, 4)], {4: ec.addr("203.0.113.4", 1)}
        out[name] = Config(sk, peers, routes, ends, rb(32))
        routes_a.append((net, 16, at_a))
        ends_a[at_a] = ADDR[name]
    out["A"] = Config(sk_a, peers_a, routes_a, ends_a, rb(32))
    return out


class Builder:
    """the ticks of one lifetime; every random value comes from self.rng, in the order the steps are added"""

    def __init__(self, seed):
        self.g = load_golden("handshake_full.json")["handshake"]
        self.seed, self.rng = seed, np.random.default_rng([seed, 2])
        self.ticks, self.sid, self.ts = [], 0x1000, int.from_bytes(bytes.fromhex(self.g["timestamp"]), "big")
        self.sent = {}    # node -> the W of every frame of its last send

    def rb(self, k):
        return self.rng.integers(0, 256, k, dtype=np.uint8).tobytes()

    def tick(self, now):
        self.steps = []
        self.ticks.append((now, self.steps))

    def add(self, op, node, **kw):
        self.steps.append(dict(op=op, node=node, **kw))

    def ids(self):
        self.sid += NP
        return [self.sid + k for k in range(NP)]

    def initiator_fresh(self, golden=False):
        ts = self.ts.to_bytes(12, "big")
        self.ts += 1
        esk = [self.rb(32) for _ in range(NP)]
        if golden:
            esk[0] = bytes.fromhex(self.g["esk_i"])
        return dict(esk=esk, ts=[ts] * NP, sids=self.ids())

    def responder_fresh(self, golden_row=None):
        esk = [self.rb(32) for _ in range(NP)]
        if golden_row is not None:
            esk[golden_row] = bytes.fromhex(self.g["esk_r"])
        return dict(esk=esk, sids=self.ids(), nonces=[self.rb(24) for _ in range(NP)],
                    seeds=[(int.from_bytes(self.rb(8), "little"), int.from_bytes(self.rb(8), "little")) for _ in range(rl.DEPTH)])

    # -- data
    def send(self, node, n, dsts, src_net, odd=()):
        """n inner packets with lengths from route_cases.INNER_LENGTHS (those IPv4 accepts, and the two it does not
        at `odd`), destinations cycling through dsts; the sources are the sender's own addresses"""
        desc, buf, good = np.zeros(n, DESC), self.rng.integers(1, 256, NB * STRIDE, dtype=np.uint8), rt.INNER_LENGTHS[2:]
        W = []
        for i in range(n):
            L = rt.INNER_LENGTHS[i % 2] if i in odd else good[i % len(good)]
            dst = dsts[i % len(dsts)]
            pkt = rt.ipv4(L, src_net + 1 + i % 200, dst, self.rng)
            buf[i * STRIDE + 16:i * STRIDE + 16 + L] = pkt
            desc[i] = (i * STRIDE, L, 0x7777)
            W.append(32 + rt.roundup16(L))
        self.sent[node] = W
        self.add("send", node, desc=desc, plain=buf)
        return W

    def deliver(self, src, dst, plan, tag=None):
        """plan: one item a received frame: (kind, i) -- frame i of src's last send ('tx'), of the frames dst holds in
        flight ('held'), of src's keepalives ('ka'), or synthetic bytes ('raw', bytes); plus tampering.  -> the
        network's moves, the receive's descriptors and source addresses"""
        rows, addrs = [], []
        for j, item in enumerate(plan):
            kind, i = item[0], item[1]
            opt = item[2] if len(item) > 2 else {}
            off = j * STRIDE
            if kind == "tx":
                W = self.sent[src][i]
                self.add("copy", dst, dst="rx", doff=off, src_node=src, src="tx", soff=i * STRIDE, length=W)
            elif kind == "held":
                W = opt["W"]
                self.add("copy", dst, dst="rx", doff=off, src_node=dst, src="held", soff=i * STRIDE, length=W)
            elif kind == "ka":
                W = 32
                self.add("copy", dst, dst="rx", doff=off, src_node=src, src="ka_buf", soff=32 * i, length=32)
            else:
                W = len(i)
                self.add("put", dst, name="rx", off=off, data=i)
            if "flip" in opt:
                self.add("xor", dst, name="rx", off=off + opt["flip"], value=1)
            rows.append((off + opt.get("shift", 0), opt.get("W", W), 0))
            addrs.append(opt.get("addr", ADDR[src]))
        self.add("receive", dst, desc=desc_rows(rows), src=np.frombuffer(b"".join(addrs), np.uint8).reshape(-1, 24).copy(),
                 tag=tag)

    def hold(self, node, src, count):
        """dst keeps the first `count` frames of src's last send in flight"""
        self.add("copy", node, dst="held", doff=0, src_node=src, src="tx", soff=0, length=count * STRIDE)

    # -- handshake messages
    def low_order(self, dst):
        """an initiation whose ephemeral is a point of small order, under a valid mac1: the responder's first DH is
        all zero"""
        msg = (1).to_bytes(4, "little") + self.rb(4) + hc.ORDER8_A + self.rb(76)
        return msg + hc.mac(hc.mac1_key(configs(self.seed)[dst].pk), msg) + bytes(16)

    def initiations(self, src, dst, rows, golden_row=None):
        """rows: NP entries, each ('msg', i) = row i of src's initiations, ('saved', offset) = a message dst recorded,
        ('junk',) = a flood message of type 1 from the flood address, ('badtype',) = one with a type word no length
        goes with, ('loworder',) = low_order's message, None = an empty row (RG_KEY_SKIP)"""
        desc, addrs = [], []
        for j, r in enumerate(rows):
            if r is None:
                desc.append((160 * j, 148, SKIP))
                addrs.append(bytes(24))
                continue
            if r[0] == "msg":
                self.add("copy", dst, dst="hs_in", doff=160 * j, src_node=src, src="msgs", soff=160 * r[1], length=160)
            elif r[0] == "saved":
                self.add("copy", dst, dst="hs_in", doff=160 * j, src_node=dst, src="held", soff=r[1], length=160)
            elif r[0] == "loworder":
                self.add("put", dst, name="hs_in", off=160 * j, data=self.low_order(dst))
            else:
                self.add("put", dst, name="hs_in", off=160 * j, data=(1 if r[0] == "junk" else 7).to_bytes(4, "little") + self.rb(144))
            desc.append((160 * j, 148, 0))
            addrs.append(ADDR_FLOOD if r[0] in ("junk", "badtype") else ADDR_LOW if r[0] == "loworder" else ADDR[src])
        self.add("handle_initiations", dst, desc=desc_rows(desc), fresh=self.responder_fresh(golden_row),
                 addrs=np.frombuffer(b"".join(addrs), np.uint8).reshape(-1, 24).copy())

    def responses(self, dst, resp=(), cookies=()):
        """resp / cookies: (src, row) pairs: row `row` of src's responses / cookie replies arrives at dst, in the same
        row; every other row of both arrays is handed over as RG_KEY_SKIP (lost, or never sent)"""
        addrs = [bytes(24)] * NP
        for src, row in resp:
            self.add("copy", dst, dst="resp_in", doff=96 * row, src_node=src, src="responses", soff=96 * row, length=96)
            addrs[row] = ADDR[src]
        for src, row in cookies:
            self.add("copy", dst, dst="cookie_in", doff=64 * row, src_node=src, src="replies", soff=64 * row, length=64)
        rr, cr = {r for _, r in resp}, {r for _, r in cookies}
        self.add("handle_responses", dst, rdesc=desc_rows([(96 * j, 92, 0 if j in rr else SKIP) for j in range(NP)]),
                 cdesc=desc_rows([(64 * j, 64, 0 if j in cr else SKIP) for j in range(NP)]),
                 addrs=np.frombuffer(b"".join(addrs), np.uint8).reshape(NP, 24).copy())


@functools.lru_cache(maxsize=None)
def schedule(seed):
    """one tunnel lifetime -> [(now_ns, steps)]; see the sections below"""
    b = Builder(seed)
    ip = rt.ip
    to_b, to_a = [NET_B + 7, NET_B + 300], [NET_A + 9]
    to_all = to_b + [ip(10, 3, 0, 1), ip(10, 5, 0, 1)]
    junk, real = ("junk",), lambda i: ("msg", i)  # noqa: E731
    resp = ("B", "B3", "B5")

    def row(k, what):
        return [what if j == k else None for j in range(NP)]

    # ---- 1. cold start.  A's packets find no session: peers 0, 3, 5, 6 and 7 are requested; 7 has no endpoint.
    b.tick(T0)
    b.send("A", 63, to_all + [ip(10, 6, 0, 1), ip(10, 7, 0, 1), ip(11, 0, 0, 1)], NET_A, odd=(7, 8))
    b.add("start", "A", fresh=b.initiator_fresh(golden=True))
    # the responders are idle.  B's is the recorded handshake; beside it an initiation with an ephemeral of small
    # order.  B's response is lost; those of B3 and B5 finish in one batch.
    b.initiations("A", "B", [real(0), ("loworder",)] + [None] * 6, golden_row=0)
    b.initiations("A", "B3", row(1, real(1)))
    b.initiations("A", "B5", row(2, real(2)))
    b.responses("A", resp=[("B3", 1), ("B5", 2)])
    # B has a session for A now and no endpoint: its packet leaves the gate as RG_KEY_SKIP
    b.send("B", 1, to_a, NET_B)
    b.add("timer_turn", "B", fresh=b.initiator_fresh())
    # +5 s exactly: no retry is due yet
    b.tick(T0 + 5 * SEC)
    b.add("timer_turn", "A", fresh=b.initiator_fresh())
    # +6 s: the retry meets B under load (a flood from A's address within one period): a cookie reply, which A consumes
    b.tick(T0 + 6 * SEC)
    b.add("timer_turn", "A", fresh=b.initiator_fresh())
    b.initiations("A", "B", [junk] * 7 + [("badtype",)])
    b.initiations("A", "B", [junk] * 3 + [real(0)] + [junk] * 4)
    b.responses("A", cookies=[("B", 3)])
    # +12 s: the retry carries mac2 and passes the loaded filter; A finishes, installs and arms
    b.tick(T0 + 12 * SEC)
    b.add("timer_turn", "A", fresh=b.initiator_fresh())
    b.initiations("A", "B", [junk] * 8)
    b.initiations("A", "B", [junk] * 5 + [real(0)] + [junk] * 2)
    b.responses("A", resp=[("B", 5)])
    # every responder learns A's endpoint from A's first authenticated packets; the frames of the other tunnels are
    # of unknown receivers to it
    b.tick(T0 + 13 * SEC)
    W = b.send("A", 65, to_all, NET_A)
    for name in resp:
        b.deliver("A", name, [("tx", i) for i in range(65)])
    b.hold("B", "A", 8)

    # ---- 2. traffic both ways, with everything a batch can hold
    b.tick(T0 + 14 * SEC)
    b.send("A", 257, to_b, NET_A)
    step = b.steps[-1]
    for i in range(5, 257, 16):     # every 16th inner source belongs to B's peer 4
        step["plain"][i * STRIDE + 16 + 12:i * STRIDE + 16 + 16] = np.frombuffer(ip(10, 4, 0, 9).to_bytes(4, "big"), np.uint8)
    plan = [("tx", i) for i in range(257)]
    plan[3] = ("tx", 3, dict(flip=40))                                   # forged
    plan[9] = ("tx", 2)                                                  # replayed within the batch
    plan[10] = ("held", 0, dict(W=W[0]))                                 # replayed from the batch before
    plan[11] = ("raw", (4).to_bytes(4, "little") + (0xDEAD).to_bytes(4, "little") + bytes(40))   # unknown receiver
    plan[12] = ("raw", (1).to_bytes(4, "little") + b.rb(144))            # a handshake message among the data
    plan[13] = ("tx", 13, dict(shift=8))                                 # misaligned
    for j in range(100, 257):                                            # A roams mid-batch ...
        plan[j] = (plan[j][0], plan[j][1], dict(addr=ADDR_A2))
    plan[256] = ("tx", 256, dict(flip=30, addr=ec.addr("203.0.113.66", 6)))   # ... and a forged frame from elsewhere is last
    # frame 245's inner source belongs to another peer.  It arrives as the last authentic frame, from an address
    # of its own: the endpoint moves to it although the packet ends RG_PKT_UNROUTABLE
    plan[245], plan[255] = ("tx", 255, dict(addr=ADDR_A2)), ("tx", 245, dict(addr=ADDR_A3))
    b.deliver("A", "B", plan)
    b.send("B", 63, to_a + [ip(10, 4, 0, 1)], NET_B)                     # peer 4 has no session: B asks for one
    b.deliver("B", "A", [("tx", i) for i in range(63)])
    b.add("start", "B", fresh=b.initiator_fresh())
    b.send("B3", 1, to_a, rt.ip(10, 3, 0, 0))
    b.deliver("B3", "A", [("tx", 0)])
    b.send("B5", 63, to_a, rt.ip(10, 5, 0, 0))
    b.deliver("B5", "A", [("tx", i) for i in range(63)])

    # ---- 3. A is silent for longer than the keepalive interval; two peers' packets make A's turn list two rows
    b.tick(T0 + 25 * SEC)
    b.send("B", 1, to_a, NET_B)
    b.deliver("B", "A", [("tx", 0)])
    b.send("B3", 1, to_a, rt.ip(10, 3, 0, 0))
    b.deliver("B3", "A", [("tx", 0)])
    b.add("timer_turn", "A", fresh=b.initiator_fresh())
    b.deliver("A", "B", [("ka", 0), ("ka", 1), ("ka", 2)], tag="keepalive")   # its own, B3's, a pad row's untouched bytes
    b.deliver("A", "B3", [("ka", 1)])

    # ---- 4. rekey: the rekey time passes on all three rows of A; B3's response is lost, the rest finish
    t = T0 + 12 * SEC + tc.REKEY_NS + SEC
    b.tick(t)
    b.add("timer_turn", "A", fresh=b.initiator_fresh())
    b.add("copy", "B3", dst="held", doff=NB * STRIDE - 160, src_node="A", src="msgs", soff=160, length=160)   # recorded
    b.send("A", 63, to_b + [ip(10, 6, 0, 1)], NET_A)                     # in flight on the old session
    b.hold("B", "A", 63)
    Wold = list(b.sent["A"])
    for k, name in enumerate(resp):
        b.initiations("A", name, row(k, real(k)))
    b.responses("A", resp=[("B", 0), ("B5", 2)])
    b.tick(t + 6 * SEC)
    b.add("timer_turn", "A", fresh=b.initiator_fresh())
    # peer 3's new initiation, and behind it the recorded one with its old timestamp: the ts pass rejects it
    b.initiations("A", "B3", [None, real(0), ("saved", NB * STRIDE - 160)] + [None] * 5)
    b.responses("A", resp=[("B3", 1)])
    b.send("A", 1, to_b, NET_A)                                          # on the new row
    b.deliver("A", "B", [("tx", 0)] + [("held", i, dict(W=Wold[i])) for i in range(5, 63, 5)])   # the old row still opens
    b.send("B", 65, to_a, NET_B)                                         # B answers on its new row
    b.deliver("B", "A", [("tx", i) for i in range(65)])
    b.add("start", "A", fresh=b.initiator_fresh())                       # peer 6, reaped at the turn before, starts afresh

    # ---- 5. expiry: reject-after passes on the old rows; abandoned pending rows are reaped
    t2 = T0 + 12 * SEC + tc.REJECT_NS + SEC
    b.tick(t2)
    for name in NODES:
        b.add("timer_turn", name, fresh=b.initiator_fresh())
        b.add("expire", name)
    b.deliver("A", "B", [("held", 0, dict(W=Wold[0])), ("held", 1, dict(W=Wold[1]))], tag="freed")   # for a freed row
    b.send("A", 63, to_all + [ip(10, 6, 0, 1)], NET_A)
    b.add("start", "A", fresh=b.initiator_fresh())
    for name in resp:
        b.deliver("A", name, [("tx", i) for i in range(63)])
    return b.ticks


def make_nodes(seed, cls=ModelNode, **kw):
    return {name: cls(name, configs(seed)[name], **kw) for name in NODES}


def play(ticks, nodes):
    """runs the ticks over the nodes; yields (tick index, step index, now, step, the chain's outputs) behind every
    chain, the network's moves in between"""
    for ti, (now, steps) in enumerate(ticks):
        for si, s in enumerate(steps):
            node, op = nodes[s["node"]], s["op"]
            if op == "copy":
                node.copy_from(s["dst"], s["doff"], nodes[s["src_node"]], s["src"], s["soff"], s["length"])
            elif op == "xor":
                node.xor(s["name"], s["off"], s["value"])
            elif op == "put":
                node.put(s["name"], s["off"], s["data"])
            else:
                if op == "send":
                    out = node.send(now, s["desc"], s["plain"])
                elif op == "receive":
                    out = node.receive(now, s["desc"], s["src"])
                elif op in ("start", "timer_turn"):
                    out = getattr(node, op)(now, s["fresh"])
                elif op == "handle_initiations":
                    out = node.handle_initiations(now, s["desc"], s["addrs"], s["fresh"])
                elif op == "handle_responses":
                    out = node.handle_responses(now, s["rdesc"], s["cdesc"], s["addrs"])
                else:
                    out = node.expire(now)
                yield ti, si, now, s, out


def as_bytes(v):
    return v if isinstance(v, (bytes, dict)) else np.ascontiguousarray(v).tobytes()


@functools.lru_cache(maxsize=None)
def model_run(seed):
    """the model's whole lifetime, once a seed: [(tick, step, now, op, node, outputs as bytes, both nodes' tables)] and
    the nodes (for their coverage records)"""
    nodes = make_nodes(seed)
    log = []
    for ti, si, now, s, out in play(schedule(seed), nodes):
        log.append((ti, si, now, s["op"], s["node"], {k: as_bytes(v) for k, v in out.items()},
                    {name: nd.tables() for name, nd in nodes.items()}))
    return log, nodes
