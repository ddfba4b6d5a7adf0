"""The device-resident peer endpoints, the part that needs no GPU: the ABI surface (header, both libraries, ctypes
table, source list), the layout of rg_endpoint, the argument rules -- each answered before the device is touched --
the in-order model (tests/endpoint_cases.py) against the reference's own scenarios, and the generated cases against
what they claim to contain."""
import ctypes
import os
import re
import subprocess
import textwrap

import numpy as np

import endpoint_cases as ec
from conftest import REPO
from rustyguard_amd import _lib, build, endpoint

NAMES = ("rg_endpoint_note_recv_batch_dev", "rg_endpoint_note_peers_batch_dev", "rg_endpoint_note_finish_batch_dev",
         "rg_endpoint_gate_batch_dev", "rg_endpoint_peers_batch_dev")
EINVAL, EDEVICE = -1, -2
OK, DECRYPT_ERR, REJECTED, PENDING, SKIP, NONE = ec.OK, ec.DECRYPT_ERR, ec.REJECTED, ec.PENDING, ec.SKIP, ec.NONE


def test_header_libraries_and_binding_have_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "rg_aead.h")).read(), flags=re.S)
    build.build()
    for path in (build.LIB, build.TEST_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in NAMES:
            assert f" T {name}\n" in out, (name, path)
        assert ("rg_debug_" in out) == (path == build.TEST_LIB)  # the product library exports no test hook
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _lib.SIGNATURES
    assert re.search(r"#define\s+RG_ABI_VERSION\s+6\b", text)  # additive: the version stays
    assert _lib.lib().rg_abi_version() == 6
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [11, 9, 11, 10, 8]
    assert "rg_endpoint.hip" in build.KERNELS and "rg_endpoint.hip" not in build.HOST
    for unit in build.HOST:
        assert "rg_endpoint_" not in open(os.path.join(build.CSRC, unit)).read(), unit


def test_layout_with_gcc(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "rg_aead.h"
        int main(void) {
            printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(rg_endpoint), sizeof(rg_endpoint) % 16, offsetof(rg_endpoint, ip),
                   offsetof(rg_endpoint, port_le), offsetof(rg_endpoint, set), offsetof(rg_endpoint, zero));
            printf("%zu %zu %zu\\n", sizeof(rg_src_addr), offsetof(rg_src_addr, port_le), offsetof(rg_src_addr, pad));
            return 0;
        }
    """))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                   check=True)
    vals = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    # 32-byte rows: an array that starts 16-byte aligned (the calls refuse any other) has every row 16-byte aligned
    assert vals[:6] == [32, 0, 0, 16, 18, 20] and vals[6:] == [24, 16, 18]
    S = endpoint.EndpointStruct
    assert [ctypes.sizeof(S), S.ip.offset, S.port_le.offset, S.set.offset, S.zero.offset] == [32, 0, 16, 18, 20]
    assert endpoint.ENDPOINT_BYTES == ec.ROW == 32 and endpoint.ADDR_BYTES == ec.ADDR == 24
    # the package's row and the model's agree, and the address encoding is the filter's
    from rustyguard_amd.aead import encode_src_addr
    assert endpoint.row_bytes("10.0.2.1", 1234) == ec.some_row(ec.addr("10.0.2.1", 1234)) == \
        bytes([10, 0, 2, 1]) + bytes(12) + (1234).to_bytes(2, "little") + b"\x01\x00" + bytes(12)
    assert ec.addr("2001:db8::7", 51820) == encode_src_addr("2001:db8::7", 51820)


# ------------------------------------------------------------------ refusals
class Args:
    """A set of arguments every rule accepts, as plain addresses that nothing may dereference: the context is a block
    whose device ordinal no machine has, so a call that got past its argument rules ends in RG_EDEVICE at
    hipSetDevice, with nothing enqueued, and every refusal below is the work of the one thing changed."""

    N = 9

    def __init__(self):
        self.ctx = ctypes.create_string_buffer(1 << 16)
        ctypes.memmove(self.ctx, (ctypes.c_int * 1)(0x3FFFFFF0), 4)  # rg_ctx.device
        self.base = dict(ctx=ctypes.cast(self.ctx, ctypes.c_void_p).value, endpoints=0x10000, npeers=5, map=0x20000,
                         nmap=7, idx=0x30000, status=0x40001, src=0x50000, n=self.N, claim=0x60000, out=0x70000,
                         dst=0x80000)

    def _call(self, name, order, kw):
        a = {**self.base, **kw}
        assert set(kw) <= set(order) | {"ctx"}, (name, kw)
        args = [a["ctx"]] + [a[k] for k in order] + [None]
        return getattr(_lib.lib(), name)(*[None if (v == 0 and k not in ("npeers", "nmap", "n")) else v
                                           for k, v in zip(["ctx"] + list(order) + ["stream"], args)])

    def note_recv(self, **kw):
        return self._call(NAMES[0], ("endpoints", "npeers", "map", "nmap", "idx", "status", "src", "n", "claim"), kw)

    def note_peers(self, **kw):
        return self._call(NAMES[1], ("endpoints", "npeers", "idx", "status", "src", "n", "claim"), kw)

    def note_finish(self, **kw):
        return self._call(NAMES[2], ("endpoints", "npeers", "idx", "map", "nmap", "status", "src", "n", "claim"), kw)

    def gate(self, **kw):
        return self._call(NAMES[3], ("endpoints", "npeers", "map", "nmap", "idx", "n", "out", "dst"), kw)

    def peers(self, **kw):
        return self._call(NAMES[4], ("endpoints", "npeers", "idx", "n", "out", "dst"), kw)


def _refused(call, name, bad):
    assert call(**bad) == EINVAL, (name, bad)
    assert name in _lib.lib().rg_last_error(), (name, bad, _lib.lib().rg_last_error())


def test_every_argument_rule_is_answered_before_the_device_is_touched():
    a = Args()
    b = a.base
    calls = ((a.note_recv, b"endpoint note recv", True, True), (a.note_peers, b"endpoint note peers", False, True),
             (a.note_finish, b"endpoint note finish", True, True), (a.gate, b"endpoint gate", True, False),
             (a.peers, b"endpoint peers", False, False))
    for call, name, mapped, note in calls:
        # the arguments as they stand pass every rule: the call gets as far as selecting the device
        assert call() == EDEVICE, name
        assert call(npeers=0) == EDEVICE and call(npeers=NONE) == EDEVICE and call(n=NONE) == EDEVICE, name
        # a size of zero, whatever else; a null context, whatever else
        assert call(n=0) == 0 and call(n=0, endpoints=0, idx=0) == 0, name
        assert call(ctx=0) == EINVAL and call(ctx=0, n=0) == EINVAL, name
        rules = [dict(endpoints=0), dict(idx=0),                                  # a null required pointer
                 dict(n=1 << 32), dict(n=(1 << 64) - 1),                          # a count above 2^32 - 1
                 dict(endpoints=b["endpoints"] + 1), dict(endpoints=b["endpoints"] + 8),  # rg_endpoint rows: 16 bytes
                 dict(idx=b["idx"] + 1), dict(idx=b["idx"] + 2)]                  # words: 4
        if mapped:
            assert call(nmap=0) == EDEVICE and call(nmap=NONE) == EDEVICE, name
            rules += [dict(map=0), dict(map=b["map"] + 1), dict(map=b["map"] + 2)]
        if note:
            assert call(status=b["status"] + 2) == EDEVICE, name  # bytes: any address
            rules += [dict(status=0), dict(src=0), dict(claim=0),
                      dict(src=b["src"] + 1), dict(src=b["src"] + 4),             # rg_src_addr rows: 8 bytes
                      dict(claim=b["claim"] + 1), dict(claim=b["claim"] + 2)]
        else:
            assert call(out=b["idx"]) == EDEVICE, name  # in place
            rules += [dict(out=0), dict(dst=0), dict(dst=b["dst"] + 1), dict(dst=b["dst"] + 4),
                      dict(out=b["out"] + 1), dict(out=b["out"] + 2)]
        for bad in rules:
            _refused(call, name, bad)


# ------------------------------------------- the model and the reference's tests
def _table(npeers):
    return np.zeros((npeers, ec.ROW), np.uint8)


def test_model_forged_packet_does_not_update_peer_endpoint():
    """lib.rs:788-844: the responder knows the initiator at client_addr; a data packet from there is read; the same
    packet with byte 47 flipped, sent from attacker_addr, fails its tag; the reply still goes to client_addr.  And
    a replay of the genuine packet from attacker_addr (RG_PKT_REJECTED) moves nothing either."""
    client, attacker = ec.addr("10.0.2.1", 1234), ec.addr("10.0.3.1", 9999)
    slot_peer = [0]
    t = _table(1)
    t[0] = np.frombuffer(ec.some_row(client), np.uint8)  # session_with_peer(..., client_addr): the configured endpoint
    src = np.frombuffer(client + attacker + attacker, np.uint8).reshape(3, ec.ADDR)
    t1 = ec.note_loop(t, ec.recv_peers(slot_peer, [0, 0, 0]), [OK, DECRYPT_ERR, REJECTED], src)
    assert t1[0].tobytes() == ec.some_row(client)
    slots_out, dst = ec.gate_loop(t1, slot_peer, [0])
    assert slots_out == [0] and dst[0].tobytes() == client
    # had the forgery been accepted the reply would have gone to the attacker: the model can tell
    t2 = ec.note_loop(t, ec.recv_peers(slot_peer, [0, 0]), [OK, OK], src[:2])
    assert ec.gate_loop(t2, slot_peer, [0])[1][0].tobytes() == attacker
    # an unconfigured peer: send_message's early return, then roaming by authenticated packets only
    t0 = _table(2)
    slots_out, dst = ec.gate_loop(t0, [0, 1], [0, 1, SKIP])
    assert slots_out == [SKIP] * 3 and dst.shape == (3, ec.ADDR) and not dst.any()
    t3 = ec.note_loop(t0, ec.recv_peers([0, 1], [1, 1]), [OK, DECRYPT_ERR], src[:2])
    assert ec.gate_loop(t3, [0, 1], [0, 1])[0] == [SKIP, 1] and not t3[0].any()


def test_model_init_does_not_move_and_response_does():
    """handle_handshake_init leaves peer.endpoint alone (there is no note for it); handle_handshake_resp sets it for
    the response that finishes a pending handshake (handshake.rs:205) -- the winning one: a second valid response for
    the same pending row reads RG_PKT_REJECTED with pend_idx_out = RG_PEER_NONE and moves nothing."""
    a1, a2 = ec.addr("192.0.2.1", 7), ec.addr("2001:db8::2", 8, b"\xff" * 6)
    pend_peers = [2, 0]  # pending row 0 is peer 2's, row 1 is peer 0's
    t = _table(3)
    src = np.frombuffer(a1 + a2 + a2, np.uint8).reshape(3, ec.ADDR)
    t1 = ec.note_loop(t, ec.recv_peers(pend_peers, [0, NONE, 5]), [OK, REJECTED, OK], src)
    assert t1[2].tobytes() == ec.some_row(a1) and not t1[:2].any()
    assert ec.peers_loop(t1, [0, 1, 2, 3, NONE])[0] == [NONE, NONE, 2, NONE, NONE]
    dst = ec.peers_loop(t1, [2])[1]
    assert dst[0].tobytes() == a1
    # the pad of an incoming address is not carried into the row or out of it
    t2 = ec.note_loop(t, [1], [OK], src[1:2])
    assert t2[1].tobytes() == a2[:18] + b"\x01\x00" + bytes(12) and ec.peers_loop(t2, [1])[1][0].tobytes() == a2[:18] + bytes(6)


def _eligible(c):
    npeers = len(c["table"])
    peers = ec.recv_peers(c["slot_peer"], c["key_idx"])
    return peers, [s == OK and p < npeers for p, s in zip(peers, c["status"])]


def test_cases_cover_what_they_claim():
    seen = set()
    for npeers in ec.NPEERS:
        for n in ec.SIZES:
            for kind in ec.KINDS:
                c = ec.note_case(n, npeers, kind)
                peers, elig = _eligible(c)
                nkeys = len(c["slot_peer"])
                assert len(peers) == n and c["src"].shape == (n, ec.ADDR)
                for w in range(0, n, ec.WAVE):
                    named = {p for p, e in zip(peers[w:w + ec.WAVE], elig[w:w + ec.WAVE]) if e}
                    seen.add(("wave", min(len(named), 2)))
                    if len(named) > 4:
                        seen.add("more peers in a wave than the rounds of the wave reduction")
                last_any, last_elig = {}, {}
                for i, (p, e) in enumerate(zip(peers, elig)):
                    if p < npeers:
                        last_any[p] = i
                        if e:
                            last_elig[p] = i
                if any(last_elig[p] != last_any[p] for p in last_elig):
                    seen.add("last eligible item is not the last item")
                if set(last_any) - set(last_elig):
                    seen.add("named only by ineligible items")
                    if c["quiet_peer"] in set(last_any) - set(last_elig) and c["table"][c["quiet_peer"]].any():
                        seen.add("... and its row is seeded")
                if any(s == OK and npeers <= p < NONE for p, s in zip(peers, c["status"])):
                    seen.add("p >= npeers")
                if any(s == OK and k >= nkeys for k, s in zip(c["key_idx"], c["status"])):
                    seen.add("key_idx >= nkeys")
                if any(s == OK and k < nkeys and c["slot_peer"][k] == NONE for k, s in zip(c["key_idx"], c["status"])):
                    seen.add("a free row")
                assert {OK, REJECTED} <= set(c["status"]) or n == 1
                if n >= 257:
                    assert {OK, REJECTED, DECRYPT_ERR, PENDING} <= set(c["status"])
                # rows nothing writes: seeded ones with the planted bytes among them
                after = ec.note_loop(c["table"], peers, c["status"], c["src"])
                same = [p for p in range(0, npeers, 3) if p not in last_elig]
                assert all(after[p, 20:].tobytes() == b"\xee" * 12 for p in same[:50])
                assert all(after[p].tobytes() == ec.some_row(bytes(c["src"][i])) for p, i in last_elig.items())
                if npeers >= 300 and n >= 257:
                    assert same and last_elig
    assert ec.note_case(63, 3, "random", seed=1)["status"].count(OK) <= 6  # a lone wave with no eligible lane
    assert not any(_eligible(ec.note_case(63, 3, "random", seed=1))[1])
    assert seen >= {("wave", 0), ("wave", 1), ("wave", 2), "more peers in a wave than the rounds of the wave reduction",
                    "last eligible item is not the last item", "named only by ineligible items",
                    "... and its row is seeded", "p >= npeers", "key_idx >= nkeys", "a free row"}, seen
    # the gathers: unset peers, the "no" value as input, indices out of range
    for npeers in ec.NPEERS:
        g = ec.gather_case(257, npeers)
        nkeys = len(g["slot_peer"])
        assert SKIP in g["slots"] and any(nkeys <= s < SKIP for s in g["slots"])
        assert NONE in g["peer_idx"] and any(npeers <= p < NONE for p in g["peer_idx"])
        so, _ = ec.gate_loop(g["table"], g["slot_peer"], g["slots"])
        po, dst = ec.peers_loop(g["table"], g["peer_idx"])
        assert SKIP in so and NONE in po and (npeers == 1 or (any(s != SKIP for s in so) and any(p != NONE for p in po)))
        if npeers >= 3:  # a peer in range without an endpoint
            assert any(p < npeers and q == NONE for p, q in zip(g["peer_idx"], po))
        assert all((q == NONE) == (not d.any()) for q, d in zip(po, dst))
