"""Poly1305 carry-edge vectors (tests/golden/poly1305_edges.json) on the GPU.

Random bytes reach the carry and reduction branches of rg_device.h's Poly1305 with probability 2^-30 or
less; the fixture's vectors sit on them (tests/golden/make_poly_edges.py: accumulators held as p + T or
2^130 + T, tags that carry through every word, segment partial sums of 0..5 and p - 1, partial sums that
cancel or whose fold carries).  Every kernel family opens them, rejects them with one tag bit flipped and
seals their plaintexts back, bit for bit against the fixture, which tests/test_poly_edges_cpu.py pins to
Poly1305 in Python integers and to the C oracle.

The flattened kernel's own path (per-lane pieces, carry powers, 64-bit slot sums, phase F) gets a fixture of its
own, tests/golden/poly1305_flat_edges.json, sent one packet per call: tests/test_poly_flat_edges_cpu.py.
"""
import sys

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from rustyguard_amd import aead
from test_gpu_parity import MODES, _configure, _gpu_open, _gpu_seal, _mode_id, _reset  # tests/ is on sys.path

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_poly_edges as G  # noqa: E402

pytestmark = pytest.mark.gpu

VECTORS = load_golden("poly1305_edges.json")["vectors"]
_batches = {}


def _batch(layout):
    """the batched vectors alone, or with random-size filler frames between them (both built once)"""
    if layout not in _batches:
        _batches[layout] = G.frame_batch(VECTORS, None if layout == "alone" else 7)
    return _batches[layout]


@pytest.mark.parametrize("mode", MODES, ids=_mode_id)
def test_batched_edge_vectors(engine, mode):
    _configure(engine, mode)
    try:
        for layout in ("alone", "interleaved"):
            b = _batch(layout)
            n = len(b["desc_open"])
            # the split the segment vectors were built for is the one in force
            if mode[0] == "pipe" and mode[1] in (2, 4):
                assert engine.kernel_for(n) == 0 and engine.lanes_per_packet(n) == mode[1]
                assert any(v.get("seg_k") == mode[1] for v in b["vectors"])
            if mode[0] == "tile" and mode[3] in (2, 4):
                assert engine.kernel_for(n) == mode[1]  # rg_set_segments(k) holds for every packet
                assert any(v.get("seg_k") == mode[3] for v in b["vectors"])
            # open with the fixture's tags
            back, st, co = _gpu_open(engine, b["keys"], b["desc_open"], b["sealed"])
            bad = np.nonzero(st != aead.PKT_OK)[0]
            assert bad.size == 0, [b["vectors"][list(b["vec"]).index(i)]["label"] for i in bad if i in b["vec"]]
            assert np.array_equal(co, b["counters"])
            assert np.array_equal(back, b["plain"])
            if mode[0] in ("pipe", "tile", "flat"):
                assert engine.last_kernel() == {"pipe": 0, "tile": mode[1], "flat": 3}[mode[0]]
            # one tag bit flipped, in the lowest and in the highest byte
            for byte, bit in ((-16, 0x01), (-1, 0x80)):
                forged = b["sealed"].copy()
                for d in b["desc_open"]:
                    forged[int(d["offset"]) + int(d["len"]) + byte] ^= bit
                back, st, _ = _gpu_open(engine, b["keys"], b["desc_open"], forged)
                assert (st == aead.PKT_DECRYPT_ERR).all()
                assert np.array_equal(back, forged)
            # seal of the derived plaintexts: headers, ciphertexts and tags of the fixture
            got, st = _gpu_seal(engine, b["keys"], b["receivers"], b["desc_seal"], b["counters"], b["plain"])
            assert (st == aead.PKT_OK).all()
            for i, v in zip(b["vec"], b["vectors"]):
                o, p = int(b["desc_seal"][i]["offset"]), int(b["desc_seal"][i]["len"])
                assert got[o + 16: o + 16 + p].tobytes().hex() == v["ct"], v["label"]
                assert got[o + 16 + p: o + 32 + p].tobytes().hex() == v["tag"], v["label"]
            assert np.array_equal(got, b["sealed"])
    finally:
        _reset(engine)


FLAT_VECTORS = load_golden("poly1305_flat_edges.json")["vectors"]
_flat_frames = {}


def _flat_frame(v):
    """the vector as a one-packet call (built once, shared by the three modes, never written to)"""
    if v["id"] not in _flat_frames:
        _flat_frames[v["id"]] = G.flat_frame(v)
    return _flat_frames[v["id"]]


@pytest.mark.parametrize("mode", [m for m in MODES if m[0] == "flat"], ids=_mode_id)
def test_flat_one_packet_edge_vectors(engine, mode):
    """tests/golden/poly1305_flat_edges.json: each vector alone in a call, so that the flattened kernel deals its
    chunks over the lanes as make_poly_edges.flat_pieces says and the vector's pieces, carry powers and slot sums
    are the ones it was solved for.  Open, open with the tag's lowest and highest bit flipped (the frame comes
    back as it was), seal: bit for bit, in the three flat modes."""
    _configure(engine, mode)
    try:
        for v in FLAT_VECTORS:
            b = _flat_frame(v)
            at, n = b["at"], b["P"]
            back, st, co = _gpu_open(engine, b["keys"], b["desc_open"], b["sealed"])
            assert engine.last_kernel() == 3
            assert st[0] == aead.PKT_OK, v["label"]
            assert co[0] == v["counter"], v["label"]
            assert np.array_equal(back, b["plain"]), v["label"]
            for byte, bit in ((-16, 0x01), (-1, 0x80)):
                forged = b["sealed"].copy()
                forged[at + n + 32 + byte] ^= bit
                back, st, _ = _gpu_open(engine, b["keys"], b["desc_open"], forged)
                assert engine.last_kernel() == 3
                assert st[0] == aead.PKT_DECRYPT_ERR, v["label"]
                assert np.array_equal(back, forged), v["label"]
            got, st = _gpu_seal(engine, b["keys"], b["receivers"], b["desc_seal"], b["counters"], b["plain"])
            assert engine.last_kernel() == 3
            assert st[0] == aead.PKT_OK, v["label"]
            assert got[at + 16 + n: at + 32 + n].tobytes().hex() == v["tag"], v["label"]
            assert got[at + 16: at + 16 + n].tobytes() == G.flat_vector_ct(v), v["label"]
            assert np.array_equal(got, b["sealed"]), v["label"]  # header, and every byte outside the frame
    finally:
        _reset(engine)


@pytest.mark.parametrize("kind", ["msg", "xmsg"])
def test_per_message_edge_vectors(engine, kind):
    """chacha20poly1305_{enc,dec} / xchacha20poly1305_{enc,dec} on the per-message shapes (AAD of 0, 12, 16
    bytes, lengths 1, 15, 17, 100): exact ciphertext and tag; a forged tag raises and leaves the buffer as
    it came."""
    from oracle import oracle

    enc = engine.chacha20poly1305_enc if kind == "msg" else engine.xchacha20poly1305_enc
    dec = engine.chacha20poly1305_dec if kind == "msg" else engine.xchacha20poly1305_dec
    ref_open = oracle.aead_open if kind == "msg" else oracle.xaead_open
    vs = [v for v in VECTORS if v["kind"] == kind]
    assert len(vs) == 24
    for v in vs:
        key, nonce, aad = bytes.fromhex(v["key"]), bytes.fromhex(v["nonce"]), bytes.fromhex(v["aad"])
        tag = bytes.fromhex(v["tag"])
        pt = ref_open(key, nonce, aad, bytes.fromhex(v["ct"]), tag)
        assert pt is not None
        buf = bytearray(pt)
        got = enc(key, nonce, aad, buf)
        assert buf.hex() == v["ct"] and got.hex() == v["tag"], v["label"]
        for byte, bit in ((0, 0x01), (15, 0x80)):
            bad = bytearray(tag)
            bad[byte] ^= bit
            with pytest.raises(aead.DecryptionError):
                dec(key, nonce, aad, buf, bytes(bad))
            assert buf.hex() == v["ct"], v["label"]
        dec(key, nonce, aad, buf, tag)
        assert bytes(buf) == pt, v["label"]
