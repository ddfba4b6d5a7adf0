"""CPU-side checks of the batched IKpsk2 responder: the public structs and the new status as gcc lays them
out, the peer table on the host, the model of tests/handshake_cases.py against the reference's recorded
handshake (tests/golden/handshake_full.json), and that the entry points are documented, bound and exported."""
import ctypes
import os
import re
import subprocess
import textwrap

import numpy as np
import pytest

import handshake_cases as hc
from conftest import REPO, load_golden
from rustyguard_amd import _lib, aead

ENTRY_POINTS = ["rg_x25519_batch_dev", "rg_peer_table_build", "rg_peer_table_find", "rg_handshake_init_batch_dev",
                "rg_handshake_resp_batch_dev"]


def test_struct_layouts_and_status_with_gcc(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "rg_aead.h"
        int main(void) {
            printf("%zu %zu %zu\\n", sizeof(rg_hs_static), offsetof(rg_hs_static, private_key),
                   offsetof(rg_hs_static, public_key));
            printf("%zu %zu %zu %zu\\n", sizeof(rg_hs_peer), offsetof(rg_hs_peer, public_key),
                   offsetof(rg_hs_peer, preshared_key), offsetof(rg_hs_peer, mac1_key));
            printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(rg_hs_init_result), offsetof(rg_hs_init_result, chain),
                   offsetof(rg_hs_init_result, hash), offsetof(rg_hs_init_result, ephemeral),
                   offsetof(rg_hs_init_result, timestamp), offsetof(rg_hs_init_result, peer),
                   offsetof(rg_hs_init_result, sender), offsetof(rg_hs_init_result, pad));
            printf("%d %d %u\\n", (int)RG_PKT_KEYEXCHANGE, RG_ABI_VERSION, RG_PEER_NONE);
            return 0;
        }
    """))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o",
                    str(exe)], check=True)
    rows = [list(map(int, ln.split())) for ln in
            subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert rows == [[64, 0, 32], [96, 0, 32, 64], [128, 0, 32, 64, 96, 108, 112, 116], [8, 6, 0xFFFFFFFF]]
    assert aead.PKT_KEYEXCHANGE == 8 and aead.PEER_NONE == 0xFFFFFFFF
    assert len(hc.ZERO_ROW) == 128 and hc.KEYEXCHANGE == 8


def _peers(n, seed, first_word=None):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 256, (n, 96), dtype=np.uint8)
    if first_word is not None:
        rows[:, 0:4] = np.frombuffer(first_word.to_bytes(4, "little"), np.uint8)
    return rows


@pytest.mark.parametrize("n", [1, 5, 1000])
def test_peer_table_finds_every_peer(n):
    rows = _peers(n, 100 + n)
    table = aead.peer_table(rows)
    cap = table.shape[0]
    assert cap >= 2 * n and cap & (cap - 1) == 0
    assert sorted(int(x) for x in table[table != 0xFFFFFFFF]) == list(range(n))
    for i in range(n):
        assert aead.peer_find(rows, table, rows[i, :32].tobytes()) == i
    # the documented slot rule: every row sits at or after its home slot, with no empty slot in between
    shift = 32 - (cap.bit_length() - 1)
    for i in range(0, n, max(1, n // 50)):
        home = ((int.from_bytes(rows[i, :4].tobytes(), "little") * 0x9E3779B1) & 0xFFFFFFFF) >> shift
        s = home
        while table[s] != i:
            assert table[s] != 0xFFFFFFFF
            s = (s + 1) & (cap - 1)
    absent = np.random.default_rng(1).integers(0, 256, 32, dtype=np.uint8).tobytes()
    assert aead.peer_find(rows, table, absent) == -1
    # a key that differs from a peer's in its last byte only is absent too (all 32 bytes are compared)
    near = bytearray(rows[0, :32].tobytes())
    near[31] ^= 0x80
    assert aead.peer_find(rows, table, bytes(near)) == -1


def test_peer_table_forced_collisions_and_refusals():
    rows = _peers(40, 7, first_word=0xDEADBEEF)  # equal first words: one probe chain
    table = aead.peer_table(rows, cap=128)
    for i in range(40):
        assert aead.peer_find(rows, table, rows[i, :32].tobytes()) == i
    filled = np.flatnonzero(table != 0xFFFFFFFF)
    assert len(filled) == 40 and ((filled - filled[0]) % 128 < 40).all()  # contiguous from the home slot
    L = _lib.lib()
    t = np.zeros(128, np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert L.rg_peer_table_build(p(rows), 40, p(t), 64) == -1  # cap < 2 n
    assert b"cap" in L.rg_last_error()
    assert L.rg_peer_table_build(p(rows), 40, p(t), 96) == -1  # not a power of two
    assert L.rg_peer_table_build(p(rows), 40, p(t), 0) == -1
    dup = rows.copy()
    dup[17, :32] = dup[3, :32]  # the same public key under another preshared key
    assert L.rg_peer_table_build(p(dup), 40, p(t), 128) == -1
    assert b"duplicate" in L.rg_last_error()
    assert L.rg_peer_table_build(p(rows), 40, None, 128) == -1
    assert L.rg_peer_table_build(None, 0, p(t), 2) == 0 and (t[:2] == 0xFFFFFFFF).all()  # an empty table
    assert L.rg_peer_table_find(p(rows), p(t), 96, p(rows)) == -1


def test_model_reproduces_the_recorded_handshake():
    """initiation -> result row -> the reference's recorded response and both transport keys, byte for byte."""
    g = load_golden("handshake_full.json")["snapshot"]
    sk_i, sk_r = bytes.fromhex(g["static_private_i"]), bytes.fromhex(g["static_private_r"])
    psk, esk_r = bytes.fromhex(g["preshared_key"]), bytes.fromhex(g["esk_r"])
    init, resp = bytes.fromhex(g["initiation"]), bytes.fromhex(g["response"])
    old = load_golden("handshake_vectors.json")["handshake_macs"]
    assert init.hex() == old["initiation"] and resp.hex() == old["response"]  # the same recorded messages
    pk_i = hc.pubkey(sk_i)
    st, row = hc.consume_initiation(init, sk_r, [hc.pubkey(b"\x01" * 32), pk_i])
    want = bytearray.fromhex(g["result_row"])  # recorded with the peer in row 0; here it is row 1
    want[108:112] = (1).to_bytes(4, "little")
    assert st == hc.OK and row == bytes(want)
    assert row[96:108].hex() == g["timestamp"] == "400000000000000a00000000"
    assert row[64:96] == init[8:40] and row[112:116] == init[4:8] and row[108:112] == (1).to_bytes(4, "little")
    peers = [(hc.pubkey(b"\x01" * 32), bytes(32), bytes(32)), (pk_i, psk, hc.mac1_key(pk_i))]
    st, got, keys = hc.build_response(row, peers, esk_r, g["session_id"], None)
    assert st == hc.OK and got == resp
    assert keys[:32].hex() == g["send_key"] and keys[32:].hex() == g["recv_key"]
    assert g["recv_key"] == "5c1ba0299237c9d32ff307464bebce9e055f1fb481cf6a05ce83ee11590ec95b"
    assert g["session_id"] == 0x630DC0F5
    # the failures the model must report: a flipped static byte, a flipped timestamp tag, an unknown peer
    bad = bytearray(init)
    bad[50] ^= 1
    assert hc.consume_initiation(bytes(bad), sk_r, [pk_i]) == (hc.DECRYPT_ERR, hc.ZERO_ROW)
    bad = bytearray(init)
    bad[110] ^= 1
    assert hc.consume_initiation(bytes(bad), sk_r, [pk_i]) == (hc.DECRYPT_ERR, hc.ZERO_ROW)
    assert hc.consume_initiation(init, sk_r, [hc.pubkey(b"\x02" * 32)]) == (hc.REJECTED, hc.ZERO_ROW)
    bad = bytearray(init)
    bad[8:40] = hc.ORDER8_A
    assert hc.consume_initiation(bytes(bad), sk_r, [pk_i]) == (hc.KEYEXCHANGE, hc.ZERO_ROW)


def test_model_reproduces_the_crypto_crate_handshake():
    """test `handshake` (seed 3): resp.empty and K1 / K2 from the five secrets, and the initiator's finish."""
    g = load_golden("handshake_full.json")["handshake"]
    sk_i, sk_r, psk = (bytes.fromhex(g[k]) for k in ("static_private_i", "static_private_r", "preshared_key"))
    esk_i, esk_r, ts = bytes.fromhex(g["esk_i"]), bytes.fromhex(g["esk_r"]), bytes.fromhex(g["timestamp"])
    msg, hs_i = hc.make_initiation(sk_i, hc.pubkey(sk_r), esk_i, ts, 0)
    pk_i = hc.pubkey(sk_i)
    st, row = hc.consume_initiation(msg, sk_r, [pk_i])
    assert st == hc.OK
    st, resp, keys = hc.build_response(row, [(pk_i, psk, hc.mac1_key(pk_i))], esk_r, 0, None)
    assert st == hc.OK and resp[44:60].hex() == g["empty_tag"]
    assert keys[32:].hex() == g["transport_k1"] and keys[:32].hex() == g["transport_k2"]
    assert hc.finish_initiator(resp, hs_i, sk_i, esk_i, psk) == (keys[32:], keys[:32])
    old = load_golden("handshake_vectors.json")["aead_with_aad"]
    assert old["tag"] == g["empty_tag"] and old["transport_k1"] == g["transport_k1"]


def test_entry_points_documented_bound_and_exported():
    text = open(os.path.join(REPO, "INTEGRATION.md")).read()
    block = max(re.findall(r'extern "C" \{.*?\n\}', text, flags=re.S), key=len)
    for name in ENTRY_POINTS:
        assert f"pub fn {name}(" in block, name
        assert name in _lib.SIGNATURES
    for s in ("rg_hs_static", "rg_hs_peer", "rg_hs_init_result"):
        assert s in text
    from rustyguard_amd import build

    build.build()
    for path in (build.LIB, build.TEST_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r" T (rg_[a-z0-9_]+)", out))
        assert set(ENTRY_POINTS) <= exported, path
    for m in ("x25519_dev", "handshake_init_dev", "handshake_resp_dev"):
        assert hasattr(aead.Engine, m)
