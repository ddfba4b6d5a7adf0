"""Poly1305 carry-edge vectors (tests/golden/poly1305_edges.json) without a GPU.

The fixture's vectors put the Poly1305 accumulator on the carry and reduction branches of
rustyguard_amd/csrc/rg_device.h that random data does not reach (tests/golden/make_poly_edges.py).
Here every vector is checked against Poly1305 in Python integers, against the C oracle (and OpenSSL),
and against the generator's limb model of the kernel arithmetic: the model's events say which branches
a vector takes, its mutants say that the vector would notice the branch being wrong, and 10^4 random
messages say that random data would not.
"""
import collections
import os
import random
import sys

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from oracle import oracle

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_poly_edges as G  # noqa: E402

FIX = load_golden("poly1305_edges.json")
VECTORS = FIX["vectors"]
P = (1 << 130) - 5


def _poly1305(otk: bytes, msg: bytes) -> bytes:
    """RFC 8439 §2.5.1, written out once more so that the check does not lean on the generator"""
    r = int.from_bytes(otk[:16], "little") & 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
    s = int.from_bytes(otk[16:32], "little")
    a = 0
    for i in range(0, len(msg), 16):
        a = (a + int.from_bytes(msg[i:i + 16] + b"\x01", "little")) * r % P
    return ((a + s) % (1 << 128)).to_bytes(16, "little")


def _parts(v):
    return bytes.fromhex(v["key"]), bytes.fromhex(v["aad"]), bytes.fromhex(v["ct"]), bytes.fromhex(v["tag"])


def test_generator_reproduces_the_fixture():
    with open(os.path.join(GOLDEN, "poly1305_edges.json")) as f:
        committed = f.read()
    assert G.dumps(G.generate()) == committed
    assert len(committed) < 256 * 1024


def test_vectors_against_the_integer_reference():
    for v in VECTORS:
        _, aad, ct, tag = _parts(v)
        msg = G.mac_input(aad, ct)
        assert len(msg) % 16 == 0
        assert _poly1305(G.vector_otk(v), msg) == tag, v["label"]
        assert "plaintext" not in v


def test_vectors_against_the_c_oracle():
    for v in VECTORS:
        key, aad, ct, tag = _parts(v)
        assert oracle.poly1305(G.vector_otk(v), G.mac_input(aad, ct)) == tag, v["label"]
        if v["kind"] == "xmsg":
            op, seal, nonce = oracle.xaead_open, oracle.xaead_seal, bytes.fromhex(v["nonce"])
        else:
            op, seal = oracle.aead_open, oracle.aead_seal
            nonce = oracle.wg_nonce(v["counter"]) if v["kind"] == "batch" else bytes.fromhex(v["nonce"])
        pt = op(key, nonce, aad, ct, tag)
        assert pt is not None and len(pt) == len(ct), v["label"]
        assert seal(key, nonce, aad, pt) == (ct, tag), v["label"]
        for byte in (0, 15):
            bad = bytearray(tag)
            bad[byte] ^= 1 << (7 * (byte == 15))
            assert op(key, nonce, aad, ct, bytes(bad)) is None, v["label"]


@pytest.mark.parametrize("filler", [None, 7], ids=["alone", "interleaved"])
def test_batched_vectors_against_the_batch_oracles(filler):
    b = G.frame_batch(VECTORS, filler)  # opens the batch with the C oracle: every status OK
    n = len(b["desc_open"])
    assert 90 <= len(b["vec"]) <= 150 and (filler is None) == (n == len(b["vec"]))
    resealed = b["plain"].copy()
    oracle.seal_batch(b["keys"], b["receivers"], b["desc_seal"], b["counters"], resealed)
    assert np.array_equal(resealed, b["sealed"])
    for byte in (-16, -1):  # lowest and highest tag byte
        forged = b["sealed"].copy()
        for d in b["desc_open"]:
            forged[int(d["offset"]) + int(d["len"]) + byte] ^= 1 if byte == -16 else 0x80
        back = forged.copy()
        st, _ = oracle.open_batch(b["keys"], b["desc_open"], back)
        assert (st == oracle.DECRYPT_ERR).all() and np.array_equal(back, forged)
    if oracle.openssl_available():
        back = b["sealed"].copy()
        st = oracle.openssl_open_batch(b["keys"], b["desc_open"], back)
        assert (st == 0).all() and np.array_equal(back, b["plain"])
        again = b["plain"].copy()
        oracle.openssl_seal_batch(b["keys"], b["receivers"], b["desc_seal"], b["counters"], again)
        assert np.array_equal(again, b["sealed"])


# ------------------------------------------------------------------ limb model
# every branch named in the model, and the orders of evaluation in which a vector must take it
# ("h" straight Horner, "p" lane-kernel butterfly, "t" tile-kernel Horner over segments)
REQUIRED_EVENTS = {
    "acc_mul:fold_carry_out_of_w3": "hpt", "acc_mul:exit_h4==4": "hpt",
    "acc_finish:h_in_[p,2^130)": "h", "acc_finish:use_g": "h", "acc_finish:fold_h4>=4": "h",
    "acc_finish:g_ripples_all_words": "h", "acc_finish:tag_carries_all_words": "h",
    "acc_add:h4>=3+carry": "hpt", "acc_add:h4_in==4": "hpt", "acc_add:h4_out==6": "h",
    "acc_add_acc:h4>=7": "pt", "acc_fold:h4>=4": "pt", "acc_fold:carry_out_of_h3": "pt",
    "acc_mul_gen:h>=p": "pt", "to26:value>=p": "pt", "to26:l4>=2^26": "pt",
}


def test_events_are_the_models_and_cover_every_branch():
    seen = collections.Counter()
    for v in VECTORS:
        ev, tags = G.model_events(v)
        assert all(t.hex() == v["tag"] for t in tags.values()), v["label"]
        assert [e for e in ev if ":T:" not in e] == v["events"], v["label"]
        for e in v["events"]:
            path, name = e.split(":", 1)
            seen[(path[0], name)] += 1
    for name, paths in REQUIRED_EVENTS.items():
        for p in paths:
            assert seen[(p, name)] >= 1, (name, p)
    assert {n for _, n in seen} == set(REQUIRED_EVENTS)  # no event that this table does not know


def test_every_target_class_is_present():
    by = collections.defaultdict(list)
    for v in VECTORS:
        by[v["class"]].append(v["label"])
    assert set(by) == {"final", "pre_length", "intermediate", "segment", "segment_sum", "message", "xmessage"}
    fin = " | ".join(by["final"])
    for t in ["= 0 ", "= 1 ", "= 2 ", "= 3 ", "= 4 ", "= 5 ", "= 6 ", "= 2^32+4", "= 2^32+5", "p-1", "p-2", "p-3", "p-4",
              "p-5", "p-6", "= 2^128-1", "= 2^128", "= 2^129-1", "= 2^129", "= 3*2^128-1", "0xfffffffb", "0xffffffff",
              "tag all-zero", "tag all-ones", "carries through all four words"]:
        assert t in fin, t
    for cls in ("pre_length", "intermediate"):
        for t in ["= 0", "= 1", "= 2", "= 3", "= 4", "= 5", "= p-1"]:
            assert any(lab.endswith(t) or t + " " in lab or t + "," in lab for lab in by[cls]), (cls, t)
    assert any("carry out of h3" in lab for lab in by["pre_length"])
    assert {len(v["ct"]) // 2 for v in VECTORS if v["class"] == "final"} == {32, 64, 96, 272}
    seg = by["segment"]
    for K in (2, 4):
        for nb in (16, 20, 33):
            for pos in ("first", "last") + (("middle",) if K == 4 else ()):
                labs = [lab for lab in seg if lab.startswith(f"K={K} nb={nb} {pos} ")]
                assert any(" r^" in lab for lab in labs) and any(" r^" not in lab for lab in labs), (K, nb, pos)
        for t in ["0", "1", "2", "3", "4", "5", "p-1"]:
            assert any(lab.startswith(f"K={K} ") and lab.endswith("= " + t) for lab in seg), (K, t)
    assert sum("= 0" in lab for lab in by["segment_sum"]) >= 2 and sum("= p-1" in lab for lab in by["segment_sum"]) >= 2
    for cls, name in (("message", "ChaCha20-Poly1305"), ("xmessage", "XChaCha20-Poly1305")):
        shapes = {(len(v["aad"]) // 2, len(v["ct"]) // 2) for v in VECTORS if v["class"] == cls}
        assert {a for a, _ in shapes} == {0, 12, 16} and {n for _, n in shapes} == {1, 15, 17, 100}
        assert all(lab.startswith(name) for lab in by[cls])
    for v in VECTORS:  # the split a segment vector was built for is recorded
        assert ("seg_k" in v) == (v["class"] in ("segment", "segment_sum"))


def test_every_mutant_fails_a_fixture_vector():
    for m in G.MUTANTS:
        killed = 0
        for v in VECTORS:
            if not any(e.endswith(":T:" + m) for e in G.model_events(v)[0]):
                continue  # the mutated branch is not taken: the mutant computes what the model does
            killed += any(t.hex() != v["tag"] for t in G.model_events(v, m)[1].values())
        assert killed >= 1, m


def test_random_messages_match_and_do_not_see_the_rare_mutants():
    """10^4 random messages in all five orders of evaluation: the model equals the integer reference, and
    no mutant of a rare branch computes a different tag on any of them (the branch is never taken, so
    the old random-data suite could not have seen it).  The two combine mutants outside RARE_MUTANTS sit on
    a branch random multi-segment packets take (partial sums whose h4 add up to 4 or more, about one
    packet in three): they are counted here to show that the random-data parity tests do reach them."""
    rng = random.Random(20250101)
    killed = collections.Counter()
    for _ in range(10000):
        otk, ct = G.random_message(rng)
        want = _poly1305(otk, G.mac_input(b"", ct))
        for path in G.ALL_PATHS:
            m = G.Limbs()
            assert m.tag(otk, b"", ct, path) == want
            for e in m.ev:
                if e.startswith("T:") and G.Limbs(e[2:]).tag(otk, b"", ct, path) != want:
                    killed[e[2:]] += 1
    for m in G.RARE_MUTANTS:
        assert killed[m] == 0, m
    common = sorted(set(G.MUTANTS) - set(G.RARE_MUTANTS))
    assert common == ["combine_fold_removed", "fold_drop_mask"]
    for m in common:
        assert killed[m] >= 1, m
