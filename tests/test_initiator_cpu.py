"""CPU-side checks of the batched IKpsk2 initiator: the model of tests/initiator_cases.py against the reference's
recorded handshakes (tests/golden/handshake_full.json, handshake_initiator.json), the commit rule's two forms
against each other, rg_hs_pending as gcc and ctypes lay it out, and that both entry points are declared,
documented, bound and exported."""
import ctypes
import os
import re
import subprocess
import textwrap

import numpy as np

import handshake_cases as hc
import initiator_cases as ic
from conftest import REPO, load_golden
from rustyguard_amd import _lib, aead
from rustyguard_amd.workloads import DESC_DTYPE

ENTRY_POINTS = ["rg_handshake_initiate_batch_dev", "rg_handshake_finish_batch_dev"]
HEADER = os.path.join(REPO, "include", "rg_aead.h")


def test_model_runs_the_crypto_crate_handshake_from_the_initiator():
    """test `handshake` (seed 3): initiate with the recorded esk_i and timestamp, the responder model with the
    recorded esk_r, then the empty tag and consume_response's K1 || K2."""
    g = load_golden("handshake_full.json")["handshake"]
    sk_i, sk_r, psk = (bytes.fromhex(g[k]) for k in ("static_private_i", "static_private_r", "preshared_key"))
    esk_i, esk_r, ts = bytes.fromhex(g["esk_i"]), bytes.fromhex(g["esk_r"]), bytes.fromhex(g["timestamp"])
    pk_i, pk_r = hc.pubkey(sk_i), hc.pubkey(sk_r)
    peers = [(pk_r, psk, hc.mac1_key(pk_r))]
    st, msg, pend = ic.initiate(sk_i, peers, 0, esk_i, ts, 0x1234)
    assert st == ic.OK and len(msg) == 160 and msg[148:] == bytes(12) and msg[132:148] == bytes(16)
    assert msg[:116] == hc.make_initiation(sk_i, pk_r, esk_i, ts, 0x1234)[0][:116]
    assert pend[64:96] == esk_i and pend[96:104] == (0).to_bytes(4, "little") + (0x1234).to_bytes(4, "little")
    st, row = hc.consume_initiation(msg[:148], sk_r, [pk_i])
    assert st == hc.OK
    st, resp, keys_r = hc.build_response(row, [(pk_i, psk, hc.mac1_key(pk_i))], esk_r, 0x77, None)
    assert st == hc.OK and resp[44:60].hex() == g["empty_tag"]
    st, keys, prow, remote = ic.consume_response(resp, {0x1234: 0}, [pend], sk_i, peers)
    assert (st, prow, remote) == (ic.OK, 0, 0x77)
    assert keys.hex() == g["transport_k1"] + g["transport_k2"]
    assert keys == keys_r[32:] + keys_r[:32]  # the mirror of the responder's row
    # a cookie fills mac2 and nothing else
    st, msg2, pend2 = ic.initiate(sk_i, peers, 0, esk_i, ts, 0x1234, cookie=bytes(range(16)))
    assert msg2[:132] == msg[:132] and msg2[132:148] == hc.mac(bytes(range(16)), msg[:132]) and pend2 == pend
    # the status table's other rows
    assert ic.initiate(sk_i, peers, 1, esk_i, ts, 1) == (ic.INVALID, ic.ZERO_MSG, ic.ZERO_PENDING)
    low = [(hc.ORDER8_A, psk, bytes(32))]
    assert ic.initiate(sk_i, low, 0, esk_i, ts, 1) == (ic.KEYEXCHANGE, ic.ZERO_MSG, ic.ZERO_PENDING)
    bad = bytearray(resp)
    bad[50] ^= 1
    assert ic.consume_response(bytes(bad), {0x1234: 0}, [pend], sk_i, peers)[0] == ic.DECRYPT_ERR
    assert ic.consume_response(resp, {}, [pend], sk_i, peers) == (ic.REJECTED, *ic.ZERO_OUT)
    assert ic.consume_response(resp, {0x1234: 1}, [pend], sk_i, peers)[0] == ic.INVALID
    assert ic.consume_response(resp, {0x1234: 0}, [ic.ZERO_PENDING], sk_i, peers)[0] == ic.REJECTED
    assert ic.consume_response(resp, {0x1234: 0}, [pend], sk_i, [])[0] == ic.INVALID
    bad = bytearray(resp)
    bad[12:44] = hc.le(1)
    assert ic.consume_response(bytes(bad), {0x1234: 0}, [pend], sk_i, peers)[0] == ic.KEYEXCHANGE


def test_model_reproduces_the_recorded_initiation():
    """test `snapshot` (seed 1): when the generator recovered the initiator's ephemeral key, the model's
    initiation is the reference's recorded 148 bytes, and the responder model accepts it."""
    g = load_golden("handshake_initiator.json").get("snapshot_initiation")
    full = load_golden("handshake_full.json")["snapshot"]
    if g is None:
        return  # the generator found no RNG offset: nothing recorded to compare with
    assert g["initiation"] == full["initiation"] and g["timestamp"] == full["timestamp"]
    sk_i, sk_r = bytes.fromhex(g["static_private_i"]), bytes.fromhex(g["static_private_r"])
    pk_r = hc.pubkey(sk_r)
    st, msg, pend = ic.initiate(sk_i, [(pk_r, bytes(32), hc.mac1_key(pk_r))], 0, bytes.fromhex(g["esk_i"]),
                                bytes.fromhex(g["timestamp"]), g["sender"])
    assert st == ic.OK and msg[:148].hex() == g["initiation"] and pend.hex() == g["pending_row"]
    # and the recorded response finishes it into the recorded keys
    psk = bytes.fromhex(full["preshared_key"])
    st, keys, _, remote = ic.consume_response(bytes.fromhex(full["response"]), {g["sender"]: 0}, [pend], sk_i,
                                              [(pk_r, psk, hc.mac1_key(pk_r))])
    assert st == ic.OK and remote == full["session_id"]
    assert keys.hex() == full["recv_key"] + full["send_key"]


def test_commit_by_min_equals_the_in_order_loop():
    """a batch with duplicates of one pending row (both valid; the lower one forged), failures of every kind
    and rows consumed earlier: the claim-by-minimum form gives what the in-order loop gives."""
    w = ic.FinishWorld(31, npending=10)
    plan = [("valid", 0), ("tag_flipped", 1), ("valid", 2), ("valid", 0), ("valid", 1), ("eph_one", 3), ("valid", 3),
            ("consumed_row", 0), ("bad_peer_row", 0), ("unknown_receiver", 4), ("gated", 4), ("valid", 4), ("valid", 4),
            ("valid", 0), ("type1", 5), ("key_skip", 5), ("offset8", 5), ("len148", 5), ("past_buf", 5)]
    desc, gate, buf, msgs, flags = ic.finish_batch(w, plan, DESC_DTYPE)
    a = ic.commit(msgs, flags, w.table, w.pending, w.ini.sk_i, w.ini.peers)
    b = ic.commit_by_min(msgs, flags, w.table, w.pending, w.ini.sk_i, w.ini.peers)
    assert a == b
    assert a[0] == [ic.OK, ic.DECRYPT_ERR, ic.OK, ic.REJECTED, ic.OK, ic.KEYEXCHANGE, ic.OK, ic.REJECTED, ic.INVALID,
                    ic.REJECTED, ic.REJECTED, ic.OK, ic.REJECTED, ic.REJECTED, ic.INVALID, ic.REJECTED, ic.UNALIGNED,
                    ic.INVALID, ic.INVALID]
    assert a[2][:7] == [0, ic.PEER_NONE, 2, ic.PEER_NONE, 1, ic.PEER_NONE, 3]
    after = a[4]
    assert [r for r in range(10) if after[r] == ic.ZERO_PENDING] == [0, 1, 2, 3, 4, 8, 9]
    assert after[5] == w.pending[5] and after[7] == w.pending[7]  # untouched: only failures named row 5
    # the same batch again: every row it finished is gone, also for the forgeries that named one (1 and 5)
    again = ic.commit(msgs, flags, w.table, after, w.ini.sk_i, w.ini.peers)
    assert all(s2 == (ic.REJECTED if s1 == ic.OK or i in (1, 5) else s1)
               for i, (s1, s2) in enumerate(zip(a[0], again[0])))
    assert again[4] == after and all(k == bytes(64) for k in again[1])


def test_pending_struct_layout_with_gcc_and_ctypes(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "rg_aead.h"
        int main(void) {
            printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(rg_hs_pending), offsetof(rg_hs_pending, chain),
                   offsetof(rg_hs_pending, hash), offsetof(rg_hs_pending, esk), offsetof(rg_hs_pending, peer),
                   offsetof(rg_hs_pending, sender), offsetof(rg_hs_pending, pad));
            return RG_ABI_VERSION == 6 ? 0 : 1;
        }
    """))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o",
                    str(exe)], check=True)
    vals = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert vals == [128, 0, 32, 64, 96, 100, 104]
    P = aead.HsPending
    assert ctypes.sizeof(P) == 128
    assert [getattr(P, f).offset for f in ("chain", "hash", "esk", "peer", "sender", "pad")] == vals[1:]
    assert len(ic.ZERO_PENDING) == 128 and len(ic.pending_row(bytes(32), bytes(32), bytes(32), 1, 2)) == 128


def test_pending_table_maps_senders_to_rows():
    rows = np.zeros((6, 128), np.uint8)
    for r in range(6):
        rows[r] = np.frombuffer(ic.pending_row(bytes(32), bytes(32), bytes(32), r % 3, 0x9000 + 17 * r), np.uint8)
    rows[4] = np.frombuffer(ic.ZERO_PENDING, np.uint8)  # a consumed row is left out
    table = aead.pending_table(rows)
    assert table.shape == (16, 2)
    for r in range(6):
        assert aead.rx_find(table, 0x9000 + 17 * r) == (-1 if r == 4 else r)
    assert aead.rx_find(table, 0) == -1
    by_id = aead.pending_table(np.array([5, 9, 0xFFFFFFFF], np.uint32), cap=32)
    assert by_id.shape == (32, 2) and [aead.rx_find(by_id, s) for s in (5, 9, 0xFFFFFFFF, 6)] == [0, 1, 2, -1]


def test_header_declares_both_calls():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert re.search(r"typedef struct rg_hs_pending \{.*?\} rg_hs_pending;", text, flags=re.S)
    assert "#define RG_ABI_VERSION 6" in text  # symbols were added, nothing changed


def test_entry_points_documented_bound_and_exported():
    text = open(os.path.join(REPO, "INTEGRATION.md")).read()
    block = max(re.findall(r'extern "C" \{.*?\n\}', text, flags=re.S), key=len)
    for name in ENTRY_POINTS:
        assert f"pub fn {name}(" in block, name
        assert name in _lib.SIGNATURES
    assert "rg_hs_pending" in text and "new_handshake" in text and "handle_handshake_resp" in text
    from rustyguard_amd import build

    build.build()
    for path in (build.LIB, build.TEST_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r" T (rg_[a-z0-9_]+)", out))
        assert set(ENTRY_POINTS) <= exported, path
    for m in ("handshake_initiate_dev", "handshake_finish_dev"):
        assert hasattr(aead.Engine, m)
