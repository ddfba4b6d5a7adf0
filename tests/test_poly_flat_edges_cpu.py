"""Poly1305 carry-edge vectors for the flattened kernel (tests/golden/poly1305_flat_edges.json) without a GPU.

rg_flat.hip sums a packet's Poly1305 as per-lane Horner pieces, carries h r^pe from a per-lane
square-and-multiply, 64-bit LDS slot sums and a limb walk with a fold of a large h4 (phase F).  A call
with one packet puts it alone in one unit, so the deal of its chunks over the lanes is a function of its
length (make_poly_edges.flat_pieces) and vectors that sit on that path's rare branches can be solved ahead
of time.  Here every vector is checked against Poly1305 in Python integers and the C oracle; the limb model
of the path (Limbs.flat_tag, both directions) must give the same tag, names the branches each vector takes
and carries one mutant per decision point: every mutant fails a fixture vector, and the mutants of the rare
branches pass 10^4 random one-packet messages.
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

FIX = load_golden("poly1305_flat_edges.json")
VECTORS = FIX["vectors"]
P = (1 << 130) - 5
SIZES = [80, 128, 1504, 4096, 4112, 8208, 65536]


def _poly1305(otk: bytes, msg: bytes) -> bytes:
    """RFC 8439 §2.5.1, written out once more so that the check does not lean on the generator"""
    r = int.from_bytes(otk[:16], "little") & 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
    s = int.from_bytes(otk[16:32], "little")
    a = 0
    for i in range(0, len(msg), 16):
        a = (a + int.from_bytes(msg[i:i + 16] + b"\x01", "little")) * r % P
    return ((a + s) % (1 << 128)).to_bytes(16, "little")


@pytest.fixture(scope="module")
def models():
    """every vector under the unmutated model, both directions (computed once)"""
    return [G.flat_model(v) for v in VECTORS]


def test_generator_reproduces_both_fixtures():
    with open(os.path.join(GOLDEN, "poly1305_flat_edges.json")) as f:
        committed = f.read()
    assert G.dumps(G.generate_flat()) == committed
    assert len(committed) < 128 * 1024  # the first fixture's order of size
    # the first fixture comes from a generator of its own: making the second one before it changes nothing
    with open(os.path.join(GOLDEN, "poly1305_edges.json")) as f:
        assert G.dumps(G.generate()) == f.read()


def test_vectors_against_the_integer_reference_and_the_c_oracle():
    assert collections.Counter(v["P"] for v in VECTORS).keys() == set(SIZES)
    assert sum(v["P"] == 65536 for v in VECTORS) <= 2
    for v in VECTORS:
        key, ct, tag = bytes.fromhex(v["key"]), G.flat_vector_ct(v), bytes.fromhex(v["tag"])
        assert len(ct) == v["P"] and all(0 <= i < v["P"] // 16 for i, _ in v["solved"])
        otk, nonce = G.flat_vector_otk(v), oracle.wg_nonce(v["counter"])
        assert _poly1305(otk, G.mac_input(b"", ct)) == tag, v["label"]
        assert oracle.poly1305(otk, G.mac_input(b"", ct)) == tag, v["label"]
        pt = oracle.aead_open(key, nonce, b"", ct, tag)
        assert pt is not None and oracle.aead_seal(key, nonce, b"", pt) == (ct, tag), v["label"]
        for byte in (0, 15):
            bad = bytearray(tag)
            bad[byte] ^= 1 << (7 * (byte == 15))
            assert oracle.aead_open(key, nonce, b"", ct, bytes(bad)) is None, v["label"]
            assert G.Limbs().flat_tag(otk, ct, "open", bytes(bad)) is False, v["label"]


def test_one_packet_frames_against_the_batch_oracle():
    """the frames the GPU test sends: the C oracle seals their plaintexts back to the fixture's bytes"""
    for v in VECTORS:
        b = G.flat_frame(v)
        at, n = b["at"], v["P"]
        assert b["sealed"][at + 16:at + 16 + n].tobytes() == G.flat_vector_ct(v)
        again = b["plain"].copy()
        oracle.seal_batch(b["keys"], b["receivers"], b["desc_seal"], b["counters"], again)
        assert np.array_equal(again, b["sealed"]), v["label"]


def test_flat_pieces_invariants():
    for n in list(range(0, 8257, 16)) + SIZES:
        L = G.flat_pieces(n)
        nb, D, lanes = L["nb"], L["D"], L["lanes"]
        assert D == max(1, -(-nb // 4)) and L["S"] == -(-D // 64) and len(lanes) == 64
        assert lanes[0]["c_lo"] == 0 and lanes[-1]["c_hi"] == D  # the ranges tile [0, D)
        for a, b in zip(lanes, lanes[1:]):
            assert a["c_hi"] == b["c_lo"]
        assert all(0 <= x["c_hi"] - x["c_lo"] <= L["S"] for x in lanes)
        assert sum(x["b1"] - x["b0"] for x in lanes) == nb == n // 16
        live = [x for x in lanes if x["c_hi"] > x["c_lo"]]
        assert len(live) == min(D, 64)
        for x in lanes:
            behind = nb - x["b1"] if x["c_hi"] > x["c_lo"] else 0  # data blocks of the packet behind the lane
            assert x["pe"] == behind and x["carries"] == (x["pe"] > 0)
            assert (x["b0"], x["b1"]) == (min(4 * x["c_lo"], nb), min(4 * x["c_hi"], nb))
            if x["carries"]:
                assert x["b1"] - x["b0"] == 4 * (x["c_hi"] - x["c_lo"])  # a carrying piece is whole chunks
        assert not live[-1]["carries"] and live[-1]["b1"] == nb  # the last live lane carries nothing
        assert all(x["carries"] for x in live[:-1])
        mx = max(x["pe"] for x in lanes)
        assert L["pb"] == (mx.bit_length() - 1 if mx else -1)
    # the layouts the fixture's sizes were chosen for
    lay = {n: [x for x in G.flat_pieces(n)["lanes"] if x["c_hi"] > x["c_lo"]] for n in SIZES}
    assert [x["b1"] - x["b0"] for x in lay[80]] == [4, 1] and [x["pe"] for x in lay[80]] == [1, 0]
    assert [x["b1"] - x["b0"] for x in lay[128]] == [4, 4]
    assert len(lay[1504]) == 24 and lay[1504][-1]["b1"] - lay[1504][-1]["b0"] == 2 and lay[1504][0]["pe"] == 90
    assert len(lay[4096]) == 64 and all(x["c_hi"] - x["c_lo"] == 1 for x in lay[4096])
    assert [x["c_hi"] - x["c_lo"] for x in lay[4112]] == [1] * 63 + [2]
    assert {x["c_hi"] - x["c_lo"] for x in lay[8208]} == {2, 3}
    assert all(x["c_hi"] - x["c_lo"] == 16 for x in lay[65536]) and G.flat_pieces(65536)["pb"] == 11


# every decision point of the flat path named in the model.  "b": a vector must take it in seal and in open (the
# arithmetic is shared), "o": in the open (the compare exists there alone).
REQUIRED = {
    "flat:piece_h==0(mod p)": "b", "flat:piece_h>=p": "b", "flat:piece_h4==4": "b",
    "acc_mul_gen:h>=p": "b", "to26:value>=p": "b", "to26:l4>=2^26": "b",
    **{f"flat:cv=={t}(mod p)": "b" for t in range(6)}, "flat:cv==p-1(mod p)": "b", "flat:cv>=p": "b",
    "flat:pow_first_takes_1": "b", "flat:pow_first_takes_r": "b", "flat:pow_squares_1_for>=2_steps": "b",
    "flat:pow_pe==1": "b", "flat:pow_top_bit_in_multi_chunk_lane": "b", "flat:pow_bit_set": "b", "flat:pow_bit_clear": "b",
    "flat:slot_carry>=2": "b", "flat:slot_carry>=32": "b", "flat:h4>=8": "b", "flat:h4>=64": "b",
    "flat:fold_carry_out_of_h3_h4>=8": "b", "flat:sum==0(mod p)": "b", "flat:sum_limbs==p": "b",
    "flat:two_pieces_cancel": "b",
    **{f"flat:finish_held_p+{t}": "b" for t in range(5)}, "flat:finish_held_2^130+0": "b", "flat:finish_held_2^130+1": "b",
    "acc_finish:h_in_[p,2^130)": "b", "acc_finish:use_g": "b", "acc_finish:fold_h4>=4": "b",
    "acc_finish:g_ripples_all_words": "b",
    "flat:open_tag-s_borrows_every_word": "o", "flat:open_tag-s==0": "o", "flat:open_tag-s==2^128-1": "o",
}


def test_events_are_the_models_and_cover_every_branch(models):
    seen = {"seal": collections.Counter(), "open": collections.Counter()}
    for v, res in zip(VECTORS, models):
        assert res["seal"][1].hex() == v["tag"] and res["open"][1] is True, v["label"]
        ev = {d: {e for e in res[d][0] if not e.startswith("T:")} for d in res}
        assert sorted(ev["seal"] & ev["open"]) == v["events"], v["label"]
        assert sorted(ev["seal"] - ev["open"]) == v["events_seal"], v["label"]
        assert sorted(ev["open"] - ev["seal"]) == v["events_open"], v["label"]
        for d in ev:
            seen[d].update(ev[d])
    for name, where in REQUIRED.items():
        assert seen["open"][name] >= 1, name
        if where == "b":
            assert seen["seal"][name] >= 1, name
    # what depends on r alone is named as unreachable, recorded under "pow." and never taken
    assert FIX["unreachable"] == G.FLAT_UNREACHABLE
    for d in seen:
        assert not any(e in seen[d] for e in G.FLAT_UNREACHABLE)
        assert all(e.startswith("pow.") for e in G.FLAT_UNREACHABLE)


def test_first_fixture_finish_branches_through_the_flat_path():
    """The batch vectors of poly1305_edges.json, run as one-packet flat calls, take every acc_finish branch they
    take in straight order (the last acc_mul sees another representative of the same sum, and leaves the same
    one); the flat fixture reaches each of them through its own layouts as well (REQUIRED above)."""
    got = G.flat_old_fixture_finish(load_golden("poly1305_edges.json")["vectors"])
    names = {"acc_finish:h_in_[p,2^130)", "acc_finish:use_g", "acc_finish:fold_h4>=4", "acc_finish:g_ripples_all_words",
             "acc_finish:tag_carries_all_words"}
    assert set(got["h"]) == names
    assert got["flat"] == got["h"]


# the mutants of the flat path: its own and those of the shared arithmetic it runs through (the lane and tile
# kernels' combine step is not on it)
MUTANTS = G.FLAT_MUTANTS + [m for m in G.MUTANTS if m != "combine_fold_removed"]


def _killed(v, m, ct=None):
    res = G.flat_model(v, m, ct)
    return res["seal"][1].hex() != v["tag"] or res["open"][1] is not True


def test_every_mutant_fails_a_fixture_vector(models):
    for m in MUTANTS:
        killed = 0
        for v, res in zip(VECTORS, models):
            if killed >= 2 or v["P"] > 8208:
                continue
            if "T:" + m not in res["seal"][0] and "T:" + m not in res["open"][0]:
                continue  # the mutated branch is not taken: the mutant computes what the model does
            killed += _killed(v, m)
        assert killed >= 1, m


def _random_packet(rng):
    """key material and a ciphertext of whole blocks: mostly up to 40 blocks (up to 10 pieces), one in ten up
    to 130, one in a hundred 256..520 (64 pieces of one to three chunks)"""
    u = rng.random()
    nb = rng.randrange(0, 41) if u < 0.9 else rng.randrange(41, 131) if u < 0.99 else rng.randrange(256, 521)
    return rng.randbytes(32), rng.randbytes(16 * nb)


def test_random_packets_match_and_do_not_see_the_rare_mutants():
    """10^4 random one-packet messages: the model of the flat path equals the integer reference in both
    directions, and no mutant of a rare branch computes anything else on any of them.  The other mutants sit on
    branches that random packets of enough pieces do take; each is run on the messages that reach it until one
    kills it, which shows that the split into rare and common is the right one."""
    rng = random.Random(20250202)
    killed = collections.Counter()
    for _ in range(10000):
        otk, ct = _random_packet(rng)
        want = _poly1305(otk, G.mac_input(b"", ct))
        a, b = G.Limbs(), G.Limbs()
        assert a.flat_tag(otk, ct, "seal") == want and b.flat_tag(otk, ct, "open", want) is True
        for e in a.ev | b.ev:
            m = e[2:]
            if not e.startswith("T:") or m not in MUTANTS or (m not in G.FLAT_RARE_MUTANTS and killed[m]):
                continue
            if G.Limbs(m).flat_tag(otk, ct, "seal") != want or G.Limbs(m).flat_tag(otk, ct, "open", want) is not True:
                killed[m] += 1
    assert set(G.FLAT_RARE_MUTANTS) <= set(MUTANTS)
    for m in MUTANTS:
        assert (killed[m] == 0) == (m in G.FLAT_RARE_MUTANTS), (m, killed[m])
