"""The tunnel model and its schedule (tests/tunnel_cases.py), checked without a GPU: the four model nodes agree with
each other, the schedule holds every event the device test relies on (asserted from the model's own
outputs: conditions on the inputs, not measurements), and the first handshake is the recorded one of
golden/handshake_full.json."""
import time

import pytest

import handshake_cases as hc
import tunnel_cases as tn
from conftest import load_golden

OK, ERR, INVALID, REJECTED, UNALIGNED, NOT_DATA, PENDING, COOKIE, KEYEXCHANGE, UNROUTABLE = range(10)
SEED = 1


@pytest.fixture(scope="module")
def run():
    return tn.model_run(SEED)


def events(run, kind, node=None):
    """the coverage records of one chain, in the order it ran"""
    _, nodes = run
    return [d for name, nd in nodes.items() if node in (None, name) for k, d in nd.cov if k == kind]


def tagged(run, ticks, tag):
    """the coverage record and the step of the receive the schedule tagged"""
    recvs = [s for _, steps in ticks for s in steps if s["op"] == "receive"]
    step = next(s for s in recvs if s.get("tag") == tag)
    k = [id(s) for s in recvs if s["node"] == step["node"]].index(id(step))
    return events(run, "receive", step["node"])[k], step


def test_model_run_time_and_size():
    """the model with its pure-Python X25519 stays far below tens of seconds: a lifetime needs fewer than two hundred
    ladders (hc.x25519 is cached, so a ladder both ends compute counts once)"""
    tn.oracle.blake2s(b"")   # the oracle builds itself on its first call: not the model's time
    hc.x25519.cache_clear()
    tn.model_run.cache_clear()
    t0 = time.perf_counter()
    log, _ = tn.model_run(SEED)
    dt = time.perf_counter() - t0
    ladders = hc.x25519.cache_info().misses
    ticks = tn.schedule(SEED)
    packets = sum(len(s["desc"]) for _, steps in ticks for s in steps if s["op"] in ("send", "receive"))
    print(f"ticks {len(ticks)}, chains {len(log)}, packets {packets}, ladders {ladders}, model run {dt:.1f} s")
    assert ladders <= 200 and dt < 10
    assert {len(s["desc"]) for _, steps in ticks for s in steps if s["op"] == "send"} == set(tn.DATA_BATCHES)


def test_both_ends_hold_mirrored_keys(run):
    """every handshake that completed left A's new row and a row of B with mirrored transport keys and ids"""
    _, nodes = run
    done = [(r, d) for d in events(run, "responses", "A") for r, s in zip(d["rows"], d["install"]) if s == OK]
    assert len(done) >= 6 and any(sum(s == OK for s in d["install"]) >= 2 for d in events(run, "responses", "A"))
    log = run[0]
    for ti, si, now, op, node, out, tables in log:
        if op != "handle_responses" or node != "A":
            continue
        a = tables["A"]
        rows = [int.from_bytes(out["rows_out"][4 * i:4 * i + 4], "little") for i in range(tn.NP) if out["install_status"][i] == OK]
        for r in rows:
            lid = a["local_ids"][4 * r:4 * r + 4]
            q = [(tables[nm], k) for nm in tn.NODES[1:] for k in range(tn.NK)
                 if tables[nm]["receivers"][4 * k:4 * k + 4] == lid and tables[nm]["slot_peer"][4 * k:4 * k + 4] != b"\xff" * 4]
            assert len(q) == 1
            b, q = q[0]
            assert a["send_keys"][32 * r:32 * r + 32] == b["recv_keys"][32 * q:32 * q + 32] != bytes(32)
            assert a["recv_keys"][32 * r:32 * r + 32] == b["send_keys"][32 * q:32 * q + 32] != bytes(32)
            assert a["receivers"][4 * r:4 * r + 4] == b["local_ids"][4 * q:4 * q + 4]


def test_untampered_frames_open(run):
    """every frame one node sealed and the other received as it was, once, from a live session, is RG_PKT_OK at the
    receive (the route check may still turn it away)"""
    ticks = tn.schedule(SEED)
    recs = {nm: iter(events(run, "receive", nm)) for nm in tn.NODES}
    sends = {nm: iter(events(run, "send", nm)) for nm in tn.NODES}
    last, checked = {}, 0
    for _, steps in ticks:
        moves = []
        for s in steps:
            if s["op"] == "send":
                last[s["node"]] = next(sends[s["node"]])
            elif s["op"] in ("copy", "xor", "put"):
                moves.append(s)
            elif s["op"] == "receive":
                rec = next(recs[s["node"]])
                tampered = {m["off"] // tn.STRIDE for m in moves if m["op"] in ("xor", "put")}
                seen = set()
                for m in moves:
                    if m["op"] != "copy" or m["src"] != "tx" or m["dst"] != "rx":
                        continue
                    j, i = m["doff"] // tn.STRIDE, m["soff"] // tn.STRIDE
                    d = s["desc"][j]
                    mine = last[m["src_node"]]["peers"][i] == {nm: at_a for nm, at_a, _, _ in tn.TUNNELS}.get(s["node"], last[m["src_node"]]["peers"][i])
                    if j in tampered or i in seen or int(d["offset"]) % 16 or last[m["src_node"]]["send"][i] != OK or not mine:
                        seen.add(i)
                        continue
                    seen.add(i)
                    assert rec["recv"][j] == OK, (s["node"], j)
                    checked += 1
                moves = []
    assert checked > 400


def test_every_status_occurs_where_it_is_written(run):
    sends, recvs, inits, resps, starts = (events(run, k) for k in ("send", "receive", "initiations", "responses", "start"))
    route = {s for d in sends for s in d["route"]}
    assert {OK, INVALID, REJECTED, UNROUTABLE} <= route                      # rg_route_batch_dev
    assert {OK, REJECTED} <= {s for d in sends for s in d["send"]}           # the resident send
    recv = {s for d in recvs for s in d["recv"]}
    assert {OK, ERR, REJECTED, UNALIGNED, NOT_DATA} <= recv                  # the resident receive
    assert any(c == "duplicate" or c == "seen_initial" for d in recvs for c in d["classes"])
    final = {s for d in recvs for s in d["final"]}
    assert {OK, INVALID, UNROUTABLE} <= final                                # rg_route_check_batch_dev
    assert {OK, REJECTED, INVALID, COOKIE} <= {s for d in inits for s in d["filter"]}
    assert {OK, REJECTED, KEYEXCHANGE} <= {s for d in inits for s in d["init"]}
    assert any(a == OK and b == REJECTED for d in inits for a, b in zip(d["init"], d["ts"]))    # the ts pass
    assert {OK, REJECTED} <= {s for d in inits for s in d["resp"]}
    assert {OK, REJECTED} <= {s for d in resps for s in d["finish"]}
    assert OK in {s for d in resps for s in d["consume"]}
    assert {OK, REJECTED, INVALID} <= {s for d in starts for s in d["status"]}   # the initiate call


def test_pads_occur_in_every_padded_list(run):
    NONE = tn.NONE
    both = lambda lists: any(NONE in x and any(v != NONE for v in x) for x in lists)  # noqa: E731
    turns, starts, sends = events(run, "turn"), events(run, "start"), events(run, "send")
    assert both([d["ka"] for d in turns]) and both([d["rekey"] for d in turns])
    assert both([d["init"] for d in starts]) and both([d["gated"] for d in starts])
    assert both([d["slots"] for d in sends]) and both([d["gated"] for d in sends]) and both([d["peers"] for d in sends])
    assert both([d["rows"] for d in events(run, "responses")])
    # a peer with a session and no endpoint leaves the gate as RG_KEY_SKIP and takes no counter
    assert any(s != NONE and g == NONE and st == REJECTED
               for d in events(run, "send", "B") for s, g, st in zip(d["slots"], d["gated"], d["send"]))


def test_lifetime_events(run):
    turns, starts, recvs = events(run, "turn", "A"), events(run, "start", "A"), events(run, "receive", "B")
    assert any(OK in d["ka_status"] for d in turns)                                  # a keepalive is listed and sent
    assert any(any(p != tn.NONE for p in d["rekey"]) for d in turns)                 # a rekey is listed
    assert any(d["retried"] for d in starts)                                         # a retry happens
    assert any(d["mac2"] for d in starts) and any(COOKIE in d["filter"] for d in events(run, "initiations"))
    assert any(OK in d["filter"] and any(d["overload"]) and OK in d["resp"] for d in events(run, "initiations"))
    assert any(any(d["expired"]) for d in events(run, "expire", "A")) and any(any(d["expired"]) for d in events(run, "expire", "B"))
    assert any(any(d["expired"]) for d in starts)                                    # a pending row is reaped ...
    reaped = next(i for i, d in enumerate(starts) if any(d["expired"]))
    assert any(3 in d["init"] for d in starts[reaped + 1:])                          # ... and started afresh
    assert any(d["roamed"] for d in recvs)                                           # an endpoint roams
    assert any(d["moved"] and any(a == OK and b == UNROUTABLE for a, b in zip(d["recv"], d["final"])) and
               max(i for i, s in enumerate(d["recv"]) if s == OK) ==
               max(i for i, (a, b) in enumerate(zip(d["recv"], d["final"])) if a == OK and b == UNROUTABLE) for d in recvs)
    assert any(d["replaced"] for d in events(run, "responses", "A"))                 # peer_slot replaced by a rekey
    assert any(len([s for s in d["install"] if s == OK]) for d in events(run, "initiations", "B"))
    # a keepalive arrives: a 32-byte frame that ends RG_PKT_OK
    ticks = tn.schedule(SEED)
    ka, step = tagged(run, ticks, "keepalive")
    assert int(step["desc"][0]["len"]) == 32 and ka["final"][:2] == [OK, REJECTED]
    # a frame for a freed row is rejected: the old session's frames, behind the expiry
    assert tagged(run, ticks, "freed")[0]["recv"] == [REJECTED, REJECTED]


def test_first_handshake_is_the_recorded_one(run):
    """peer 0's first handshake, from the recorded keys, ephemerals and timestamp: B's response carries the recorded
    empty tag and B's transport keys are the recorded pair"""
    g = load_golden("handshake_full.json")["handshake"]
    first = events(run, "initiations", "B")[0]
    assert first["resp"][0] == OK
    assert first["responses"][0][44:60].tobytes().hex() == g["empty_tag"]
    assert first["keys"][0].hex() == g["transport_k2"] + g["transport_k1"]
