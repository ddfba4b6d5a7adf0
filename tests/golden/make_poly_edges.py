#!/usr/bin/env python3
"""Generate tests/golden/poly1305_edges.json and tests/golden/poly1305_flat_edges.json: Poly1305
carry-edge vectors.

Run by hand (deterministic from a fixed seed: two runs write the same bytes of both files):

    python tests/golden/make_poly_edges.py

Random data reaches the carry and reduction branches of the radix-2^32 Poly1305
in rustyguard_amd/csrc/rg_device.h with probability 2^-30 or less.  They are
reachable on purpose: r and s follow from key and nonce, and with every other
block fixed the accumulator after any block (or a segment's partial sum) is an
affine function over GF(2^130 - 5) of one free 16-byte block, so that block can
be solved for.  The solved block must land in [0, 2^128): one try in four; each
retry redraws the filler blocks and the counter.

Three parts, all imported by tests/test_poly_edges_cpu.py:

  reference   Poly1305 in Python integers (RFC 8439 §2.5, §2.8).  Keystream and
              one-time key come from oracle.chacha20_block, pinned to the RFC.
  solver      solve_block(): the free block that puts an observation at a target.
  limb model  Limbs: acc_add, acc_mul, acc_fold, acc_add_acc, to26 / make_gen /
              acc_mul_gen / acc_sqr_gen and acc_finish transliterated from
              rg_device.h, run in the straight Horner order ("h"), the lane
              kernel's K-segment butterfly (rg_pipe.hip combine_segments, "p2",
              "p4") and the tile kernel's Horner over segments (rg_tile.hip,
              "t2", "t4").  It records which rare branches fired (the fixture's
              `events`) and has mutants, one per branch (MUTANTS).

Two targets of the final state, 2^32+4 and 2^32+5, cannot be held as 2^130 + T - 5:
acc_mul folds at most c = 5 (w4 >> 2) < 2^32 into h0, so its result stays below
2^130 + 2^32 - 1.  They are kept as targets; the model shows which form they take.

Mutants.  A mutant differs from the model only where its branch fires, so the
model records a trigger "T:<mutant>" there.  Two `+ k` lines are left without a
mutant: acc_add's and acc_add_acc's carries into h4 fire on every other random
block, so the random-data parity tests already pin them; and the carry out of h3
in acc_finish's first fold cannot fire at all (h4 >= 4 on entry comes only from
acc_mul's own carry, which leaves h1 = h2 = h3 = 0), so no input kills it.
acc_add instead gets "add_h4_in_masked" (entry h4 == 4 ignored), the rare half
of that line.  The combine mutants (fold_drop_mask, combine_fold_removed) sit
on a branch that random multi-segment packets do reach (two partial sums with
h4 summing to 4 or more): RARE_MUTANTS lists the ones random data cannot see.

The flattened kernel (rg_flat.hip) has a Poly1305 path of its own, modelled in the second half of this
file: flat_pieces() (the deal of a one-packet call's chunks over the 64 lanes), Limbs.flat_tag() (the
per-lane Horner pieces, the carry power, the 64-bit slot sums and phase F) and the second fixture,
poly1305_flat_edges.json, made from a generator of its own seed after the first one (which therefore
stays byte-identical).  See the comment above flat_pieces().
"""
from __future__ import annotations

import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import oracle  # noqa: E402

P = (1 << 130) - 5
M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
M128 = (1 << 128) - 1
HI = 1 << 128
SEED = 0x706F6C7931333035
FIXTURE = os.path.join(HERE, "poly1305_edges.json")
FLAT_FIXTURE = os.path.join(HERE, "poly1305_flat_edges.json")
FLAT_SEED = 0x666C617431333035


# ------------------------------------------------------------ integer reference
def clamp(r: int) -> int:
    return r & 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF


def pad16(b: bytes) -> bytes:
    return b + b"\0" * (-len(b) % 16)


def mac_input(aad: bytes, ct: bytes) -> bytes:
    """RFC 8439 §2.8: pad16(aad) || pad16(ct) || le64(len(aad)) || le64(len(ct))"""
    return pad16(aad) + pad16(ct) + len(aad).to_bytes(8, "little") + len(ct).to_bytes(8, "little")


def to_blocks(m: bytes) -> list[int]:
    assert len(m) % 16 == 0
    return [int.from_bytes(m[i:i + 16], "little") for i in range(0, len(m), 16)]


def ref_state(r: int, blocks: list[int], h: int = 0) -> int:
    """RFC 8439 §2.5 accumulator over whole 16-byte blocks (each gets the 2^128 bit)"""
    for b in blocks:
        h = (h + b + HI) * r % P
    return h


def ref_tag(otk: bytes, msg: bytes) -> bytes:
    r, s = clamp(int.from_bytes(otk[:16], "little")), int.from_bytes(otk[16:32], "little")
    return ((ref_state(r, to_blocks(msg)) + s) & M128).to_bytes(16, "little")


def one_time_key(key: bytes, nonce12: bytes) -> bytes:
    return oracle.chacha20_block(key, 0, nonce12)[:32]


def xchacha_inner(key: bytes, nonce24: bytes) -> tuple[bytes, bytes]:
    """draft-irtf-cfrg-xchacha-03 §2.3: (subkey, 12-byte nonce) of the inner ChaCha20-Poly1305"""
    return oracle.hchacha20(key, nonce24[:16]), b"\0" * 4 + nonce24[16:]


def keystream_xor(key: bytes, nonce12: bytes, data: bytes) -> bytes:
    out = bytearray(data)
    for c in range((len(data) + 63) // 64):
        ks = oracle.chacha20_block(key, c + 1, nonce12)
        for i in range(64 * c, min(len(data), 64 * c + 64)):
            out[i] ^= ks[i - 64 * c]
    return bytes(out)


def split(nb: int, K: int, j: int) -> tuple[int, int, int]:
    """make_seg (rg_pipe.hip; rg_tile.hip shares the rule): blocks [b0, b1) of segment j and the
    blocks after it"""
    C = (nb + 3) >> 2
    L = (C + K - 1) // K
    c0 = min(j * L, C)
    c1 = min(c0 + L, C)
    b0, b1 = min(4 * c0, nb), min(4 * c1, nb)
    return b0, b1, nb - b1


# ---------------------------------------------------------------------- solver
def solve_block(F, blocks: list[int], k: int, T: int):
    """The value of blocks[k] in [0, 2^128) with F(blocks) == T (mod p), or None.  F is affine in
    every block."""
    b = list(blocks)
    b[k] = 0
    base = F(b)
    b[k] = 1
    coef = (F(b) - base) % P
    if coef == 0:
        return None
    x = (T - base) * pow(coef, -1, P) % P
    return x if x < HI else None


def F_state(r, j):
    """accumulator after block j"""
    return lambda b: ref_state(r, b[:j + 1])


def F_seg(r, nb, K, j, shifted):
    """Horner sum of segment j from zero (A_j), or A_j r^after_j"""
    b0, b1, after = split(nb, K, j)
    return lambda b: ref_state(r, b[b0:b1]) * (pow(r, after, P) if shifted else 1) % P


def F_sum(r, nb, K, js):
    fs = [F_seg(r, nb, K, j, True) for j in js]
    return lambda b: sum(f(b) for f in fs) % P


def F_tile_run(r, nb, K, upto):
    """the tile kernel's running value after it has taken in segment `upto`"""
    def f(b):
        acc = 0
        for j in range(upto + 1):
            b0, b1, _ = split(nb, K, j)
            acc = (acc * pow(r, b1 - b0, P) + ref_state(r, b[b0:b1])) % P
        return acc
    return f


# ------------------------------------------------------------------ limb model
MUTANTS = ["mul_exit_drop_k", "add_h4_in_masked", "finish_fold_drop_mask", "finish_use_g_0", "finish_g4_drop_k",
           "fold_drop_mask", "fold_drop_k", "combine_fold_removed"]
# mutants whose branch random data does not reach (see the module docstring)
RARE_MUTANTS = ["mul_exit_drop_k", "add_h4_in_masked", "finish_fold_drop_mask", "finish_use_g_0",
                "finish_g4_drop_k", "fold_drop_k"]


# ---- the flattened kernel's path (flat_pieces, Limbs.flat_tag): one mutant per decision point it adds.
# Value edges that are no branch of the code (a piece or a carry that is 0 or p - 1 mod p, two pieces that
# cancel, tag - s of 0 or 2^128 - 1) have no mutant of their own: a mutation that is wrong only there and
# right mod p everywhere else does not exist.  Pieces and carries held at or above p get a "saturates"
# mutant (the value is taken as p - 1), which stands for any code that assumes a canonical value.
FLAT_MUTANTS = [
    "flat_first_always_r",        # the first power step takes r although the top bit is clear
    "flat_first_skipped",         # the 1-or-r first step is skipped (x stays 1, the top bit is lost)
    "flat_pe1_as_zero",           # an exponent of 1 is taken for "no power"
    "flat_select_sq_on_set",      # pow_step keeps the square where the bit is set
    "flat_lead_zero_takes_mul",   # pow_step multiplies by r on a leading zero bit (x still 1)
    "flat_zero_bit_takes_mul",    # pow_step multiplies by r on a clear bit below the top bit
    "flat_skip_bit0",             # the power loop stops above bit 0
    "flat_tend_one_chunk",        # the exponent of a lane with several chunks counts one chunk only
    "flat_piece_ge_p_saturates",  # a carrying piece held at or above p is taken as p - 1
    "flat_to26_l4_mask26",        # to26 cuts the top limb to 26 bits (h4 == 4 on entry)
    "flat_cv_ge_p_saturates",     # a carry h r^pe held at or above p is taken as p - 1
    "flat_walk_carry_1bit",       # phase F's limb walk keeps one bit of a slot's carry
    "flat_walk_carry_5bit",       # ... five bits
    "flat_fold_h4_and7",          # acc_fold sees h4 & 7
    "flat_fold_h4_and63",         # acc_fold sees h4 & 63
    "flat_open_borrow_chain_cut",  # tag - s: the borrow into the top word is dropped when all three below borrow
]
# of these and of MUTANTS, the ones 10^4 random one-packet messages do not see when run through flat_tag
# (tests/test_poly_flat_edges_cpu.py checks both directions: these are never killed, the others are)
FLAT_RARE_MUTANTS = ["flat_piece_ge_p_saturates", "flat_to26_l4_mask26", "flat_cv_ge_p_saturates", "fold_drop_k",
                     "mul_exit_drop_k", "add_h4_in_masked", "finish_fold_drop_mask", "finish_use_g_0",
                     "finish_g4_drop_k"]
# Branches of the flat path that depend on r alone (r^(2^k), r^pe or the unselected x r of a power step held at
# or above p or 2^130, the clamped-r product's own carries inside the chain): no data steers them, and a
# counter search reaches 2^-30 at best against the 2^-98 or less they need.  Recorded with the "pow." prefix.
FLAT_UNREACHABLE = ["pow.acc_sqr_gen:h>=p", "pow.to26:value>=p", "pow.to26:l4>=2^26",
                    "pow.acc_mul:fold_carry_out_of_w3", "pow.acc_mul:exit_h4==4"]


def flat_pieces(P: int) -> dict:
    """The deal of a one-packet call's Poly1305 work over the 64 lanes of the flattened kernel
    (rustyguard_amd/csrc/rg_flat.hip; P = payload bytes, a multiple of 16).

    One packet is one unit and one sub-unit in all three flat modes.  launch_flat (rg_flat.hip:1123-1174): n = 1
    gives head = 0, so no short-last-group split, and flat_coop_ok (:1115-1121) returns 0 below 4096 packets,
    whatever rg_set_plan says (plan 0: balance = 0, plans 1 and 2: balance = 1, rg_batch.cpp launch_flat_any).
    The one-wave search (:565-650) then has g = 0, f0 = 0, f1 = NU, gn = 1 for every unit u = j: the packet's
    doubled midpoint is its work W (balance) or 1, the cuts are c(j) = [W < 2 floor(W j / NU)] for j > 0 and
    c(0) = 0, c(NU) = 1 (:621-642), and unit j holds the packet when c(j) = 0 and c(j + 1) = 1: c rises with
    j, so exactly one unit does, with m = 1 (:657-658), whatever the CU count.  Inside it (:730-740) D =
    flat_chunks(nb) (:147), lane l takes chunks [l D >> 6, (l + 1) D >> 6) (:779), starts in packet 0 at chunk
    c_lo (:782-787, kstart = 0) and ends in it (:924-929, kend = 0, rec.w = 0): pe = nb - 4 c_hi when blocks
    remain behind the lane, pb = the top bit of the wave's largest pe (:934-938).  A lane carries (publishes
    h r^pe, :951-983) when its cursor is still inside the packet after its last chunk (cur.t > 0: c_hi < D);
    otherwise its piece holds the packet's last chunk and is published as it is (:279-281 open, :959-964 seal).

    Returns nb, D, S (steps of the wave), pb and lanes: 64 dicts c_lo, c_hi, b0, b1 (data blocks [b0, b1)),
    pe, carries."""
    assert P % 16 == 0 and 0 <= P <= 1 << 20
    nb = P >> 4
    D = (nb + 3) >> 2 if nb else 1
    lanes = []
    for l in range(64):
        c_lo, c_hi = (l * D) >> 6, ((l + 1) * D) >> 6
        pe = nb - 4 * c_hi if c_hi > c_lo and 4 * c_hi < nb else 0
        lanes.append({"c_lo": c_lo, "c_hi": c_hi, "b0": min(4 * c_lo, nb), "b1": min(4 * c_hi, nb), "pe": pe,
                      "carries": c_hi > c_lo and c_hi < D})
    mx = max(x["pe"] for x in lanes)
    return {"nb": nb, "D": D, "S": (D + 63) // 64, "pb": mx.bit_length() - 1, "lanes": lanes}


def words(x: int) -> list[int]:
    return [(x >> (32 * i)) & M32 for i in range(4)]


def _addc(a, b, cin):
    t = a + b + cin
    return t & M32, t >> 32


class Limbs:
    """rg_device.h's Poly1305 as written: an accumulator is [h0, h1, h2, h3, h4]."""

    def __init__(self, mutant: str | None = None):
        assert mutant is None or mutant in MUTANTS or mutant in FLAT_MUTANTS
        self.mut = mutant
        self.ev: set[str] = set()
        self.ctx = ""  # "pow." while a power of r is computed (not steerable)

    def hit(self, e):
        self.ev.add(self.ctx + e)

    @staticmethod
    def value(h):
        return h[0] | h[1] << 32 | h[2] << 64 | h[3] << 96 | h[4] << 128

    @staticmethod
    def make_mul(k):
        r0, r1, r2, r3 = k[0] & 0x0FFFFFFF, k[1] & 0x0FFFFFFC, k[2] & 0x0FFFFFFC, k[3] & 0x0FFFFFFC
        return (r0, r1, r2, r3, r1 + (r1 >> 2), r2 + (r2 >> 2), r3 + (r3 >> 2))

    def acc_add(self, h, m, hibit):
        h4_in = h[4]
        h[0], k = _addc(h[0], m[0], 0)
        h[1], k = _addc(h[1], m[1], k)
        h[2], k = _addc(h[2], m[2], k)
        h[3], k = _addc(h[3], m[3], k)
        if h4_in >= 3 and k:
            self.hit("acc_add:h4>=3+carry")
        if h4_in >= 4:
            self.hit("acc_add:h4_in==4")
            self.hit("T:add_h4_in_masked")
            if k:
                self.hit("acc_add:h4_out==6")
        if self.mut == "add_h4_in_masked":
            h4_in &= 3
        h[4] = (h4_in + hibit + k) & M32

    def acc_mul(self, h, r):
        r0, r1, r2, r3, rr1, rr2, rr3 = r
        h0, h1, h2, h3, h4 = h
        d0 = h3 * rr1 + h2 * rr2 + h1 * rr3 + h0 * r0
        d1 = h4 * rr1 + h3 * rr2 + h2 * rr3 + h1 * r0 + h0 * r1
        d2 = h4 * rr2 + h3 * rr3 + h2 * r0 + h1 * r1 + h0 * r2
        d3 = h4 * rr3 + h3 * r0 + h2 * r1 + h1 * r2 + h0 * r3
        d0, d1, d2, d3 = d0 & M64, d1 & M64, d2 & M64, d3 & M64  # u64 arithmetic as written
        d4 = (h4 * r0) & M32
        w0 = d0 & M32
        w1, k = _addc(d1 & M32, d0 >> 32, 0)
        w2, k = _addc(d2 & M32, d1 >> 32, k)
        w3, k = _addc(d3 & M32, d2 >> 32, k)
        w4 = (d4 + (d3 >> 32) + k) & M32
        c = ((w4 >> 2) + (w4 & ~3 & M32)) & M32
        h[0], k = _addc(w0, c, 0)
        h[1], k = _addc(w1, 0, k)
        h[2], k = _addc(w2, 0, k)
        h[3], k = _addc(w3, 0, k)
        if k:
            self.hit("acc_mul:fold_carry_out_of_w3")
            self.hit("T:mul_exit_drop_k")
        if self.mut == "mul_exit_drop_k":
            k = 0
        h[4] = (w4 & 3) + k
        if h[4] == 4:
            self.hit("acc_mul:exit_h4==4")

    def acc_finish(self, hin, s):
        h = list(hin)
        if h[4] >= 4:
            self.hit("acc_finish:fold_h4>=4")
            self.hit("T:finish_fold_drop_mask")
        c = (h[4] >> 2) + (0 if self.mut == "finish_fold_drop_mask" else h[4] & ~3)
        t = h[0] + c
        h[0] = t & M32
        t = h[1] + (t >> 32)
        h[1] = t & M32
        t = h[2] + (t >> 32)
        h[2] = t & M32
        t = h[3] + (t >> 32)
        h[3] = t & M32
        h[4] = (h[4] & 3) + (t >> 32)
        if self.value(h) >= P:
            self.hit("acc_finish:h_in_[p,2^130)")
        g, ripple = [0] * 4, True
        t = h[0] + 5
        g[0] = t & M32
        ripple &= bool(t >> 32)
        t = h[1] + (t >> 32)
        g[1] = t & M32
        ripple &= bool(t >> 32)
        t = h[2] + (t >> 32)
        g[2] = t & M32
        ripple &= bool(t >> 32)
        t = h[3] + (t >> 32)
        g[3] = t & M32
        ripple &= bool(t >> 32)
        if ripple:
            self.hit("acc_finish:g_ripples_all_words")
        if t >> 32:
            self.hit("T:finish_g4_drop_k")
        g4 = h[4] + (0 if self.mut == "finish_g4_drop_k" else t >> 32)
        use_g = (0 - (g4 >> 2)) & M32
        if use_g:
            self.hit("acc_finish:use_g")
            self.hit("T:finish_use_g_0")
        if self.mut == "finish_use_g_0":
            use_g = 0
        w = [(h[i] & ~use_g & M32) | (g[i] & use_g) for i in range(4)]
        tag, carries = [0] * 4, True
        t = w[0] + s[0]
        tag[0] = t & M32
        carries &= bool(t >> 32)
        t = w[1] + s[1] + (t >> 32)
        tag[1] = t & M32
        carries &= bool(t >> 32)
        t = w[2] + s[2] + (t >> 32)
        tag[2] = t & M32
        carries &= bool(t >> 32)
        t = w[3] + s[3] + (t >> 32)
        tag[3] = t & M32
        carries &= bool(t >> 32)
        if carries:
            self.hit("acc_finish:tag_carries_all_words")
        return b"".join(x.to_bytes(4, "little") for x in tag)

    def to26(self, h):
        M = 0x3FFFFFF
        if self.value(h) >= P:
            self.hit("to26:value>=p")
        l4 = ((h[3] >> 8) | (h[4] << 24)) & M32
        if l4 >= 1 << 26:
            self.hit("to26:l4>=2^26")
            if not self.ctx:
                self.hit("T:flat_to26_l4_mask26")
                if self.mut == "flat_to26_l4_mask26":
                    l4 &= M
        assert h[4] < 8 and l4 < 1 << 27  # the bounds stated in rg_device.h
        return [h[0] & M, ((h[0] >> 26) | (h[1] << 6)) & M, ((h[1] >> 20) | (h[2] << 12)) & M,
                ((h[2] >> 14) | (h[3] << 18)) & M, l4]

    def make_gen(self, g):
        l = self.to26(g)
        return (l[0], l[1], l[2], l[3], l[4], l[1] * 5 & M32, l[2] * 5 & M32, l[3] * 5 & M32, l[4] * 5 & M32)

    @staticmethod
    def _from26(h, d0, d1, d2, d3, d4):
        M = 0x3FFFFFF
        for d in (d0, d1, d2, d3, d4):
            assert d <= M64
        d1 += d0 >> 26
        d2 += d1 >> 26
        d3 += d2 >> 26
        d4 += d3 >> 26
        assert d4 <= M64
        t0 = (d0 & M) + (d4 >> 26) * 5
        l0 = t0 & M
        l1 = (d1 & M) + (t0 >> 26)
        t = (l0 + (l1 << 26)) & M64
        h[0] = t & M32
        t = (t >> 32) + ((d2 & M) << 20)
        h[1] = t & M32
        t = (t >> 32) + ((d3 & M) << 14)
        h[2] = t & M32
        t = (t >> 32) + ((d4 & M) << 8)
        h[3] = t & M32
        h[4] = (t >> 32) & M32

    def acc_mul_gen(self, h, G):
        if self.value(h) >= P:
            self.hit("acc_mul_gen:h>=p")
        a = self.to26(h)
        g0, g1, g2, g3, g4, s1, s2, s3, s4 = G
        d0 = a[0] * g0 + a[1] * s4 + a[2] * s3 + a[3] * s2 + a[4] * s1
        d1 = a[0] * g1 + a[1] * g0 + a[2] * s4 + a[3] * s3 + a[4] * s2
        d2 = a[0] * g2 + a[1] * g1 + a[2] * g0 + a[3] * s4 + a[4] * s3
        d3 = a[0] * g3 + a[1] * g2 + a[2] * g1 + a[3] * g0 + a[4] * s4
        d4 = a[0] * g4 + a[1] * g3 + a[2] * g2 + a[3] * g1 + a[4] * g0
        self._from26(h, d0, d1, d2, d3, d4)

    def acc_sqr_gen(self, h):
        if self.value(h) >= P:
            self.hit("acc_sqr_gen:h>=p")
        a = self.to26(h)
        t0, t1, t2, t3 = 2 * a[0], 2 * a[1], 2 * a[2], 2 * a[3]
        u3, u4 = 5 * a[3], 5 * a[4]
        assert max(t0, t1, t2, t3, u3, u4) <= M32
        d0 = a[0] * a[0] + t1 * u4 + t2 * u3
        d1 = t0 * a[1] + t2 * u4 + a[3] * u3
        d2 = t0 * a[2] + a[1] * a[1] + t3 * u4
        d3 = t0 * a[3] + t1 * a[2] + a[4] * u4
        d4 = t0 * a[4] + t1 * a[3] + a[2] * a[2]
        self._from26(h, d0, d1, d2, d3, d4)

    def acc_add_acc(self, h, o):
        h[0], k = _addc(h[0], o[0], 0)
        h[1], k = _addc(h[1], o[1], k)
        h[2], k = _addc(h[2], o[2], k)
        h[3], k = _addc(h[3], o[3], k)
        h[4] = h[4] + o[4] + k
        if h[4] >= 7:
            self.hit("acc_add_acc:h4>=7")

    def acc_fold(self, h):
        if h[4] >= 4:
            self.hit("acc_fold:h4>=4")
            self.hit("T:fold_drop_mask")
            self.hit("T:combine_fold_removed")
        c = (h[4] >> 2) + (0 if self.mut == "fold_drop_mask" else h[4] & ~3)
        h[0], k = _addc(h[0], c, 0)
        h[1], k = _addc(h[1], 0, k)
        h[2], k = _addc(h[2], 0, k)
        h[3], k = _addc(h[3], 0, k)
        if k:
            self.hit("acc_fold:carry_out_of_h3")
            self.hit("T:fold_drop_k")
        if self.mut == "fold_drop_k":
            k = 0
        h[4] = (h[4] & 3) + k

    # ---- orders of evaluation
    def horner(self, r, blocks, track=False):
        """(accumulator over whole blocks from zero, r^len(blocks) as the tile kernel tracks it)"""
        h, pw = [0] * 5, [1, 0, 0, 0, 0]
        for b in blocks:
            self.acc_add(h, words(b), 1)
            self.acc_mul(h, r)
            if track:
                self.ctx = "pow."
                self.acc_mul(pw, r)
                self.ctx = ""
        return h, pw

    def tail(self, h, r, s, aad_len, ct_len):
        self.acc_add(h, [aad_len & M32, aad_len >> 32, ct_len & M32, ct_len >> 32], 1)
        self.acc_mul(h, r)
        return self.acc_finish(h, s)

    def combine_pipe(self, parts, afters, r):
        """combine_segments (rg_pipe.hip) as lane 0 of the group sees it"""
        K = len(parts)
        bits = max(afters).bit_length()
        hs = []
        for h, after in zip(parts, afters):
            h = list(h)
            if bits > 0:
                self.ctx = "pow."
                x = [1, 0, 0, 0, 0]
                for b in range(bits - 1, -1, -1):
                    self.acc_sqr_gen(x)
                    if (after >> b) & 1:
                        self.acc_mul(x, r)
                G = self.make_gen(x)
                self.ctx = ""
                self.acc_mul_gen(h, G)
            hs.append(h)
        o = 1
        while o < K:
            nxt = {}
            for j in range(0, K, 2 * o):  # the lanes lane 0 depends on
                h = list(hs[j])
                self.acc_add_acc(h, hs[j + o])
                if self.mut != "combine_fold_removed":
                    self.acc_fold(h)
                nxt[j] = h
            for j, h in nxt.items():
                hs[j] = h
            o <<= 1
        return hs[0]

    def combine_tile(self, parts, pws):
        """rg_tile.hip: h = (..(A_0 q_1 + A_1) q_2 + ..) + A_{K-1}"""
        acc = list(parts[0])
        for a, q in zip(parts[1:], pws[1:]):
            self.ctx = "pow."
            G = self.make_gen(q)
            self.ctx = ""
            self.acc_mul_gen(acc, G)
            self.acc_add_acc(acc, a)
            if self.mut != "combine_fold_removed":
                self.acc_fold(acc)
        return acc

    def tag(self, otk: bytes, aad: bytes, ct: bytes, path: str = "h") -> bytes:
        """path "h": straight Horner (any AAD, any length); "p2"/"p4"/"t2"/"t4": K segments (empty AAD,
        whole blocks)"""
        k = [int.from_bytes(otk[4 * i:4 * i + 4], "little") for i in range(8)]
        r, s = self.make_mul(k[:4]), k[4:]
        if path == "h":
            h, _ = self.horner(r, to_blocks(pad16(aad) + pad16(ct)))
            return self.tail(h, r, s, len(aad), len(ct))
        assert not aad and len(ct) % 16 == 0
        K, blocks = int(path[1]), to_blocks(ct)
        parts, pws, afters = [], [], []
        for j in range(K):
            b0, b1, after = split(len(blocks), K, j)
            h, pw = self.horner(r, blocks[b0:b1], track=path[0] == "t" and j > 0)
            parts.append(h)
            pws.append(pw)
            afters.append(after)
        h = self.combine_pipe(parts, afters, r) if path[0] == "p" else self.combine_tile(parts, pws)
        return self.tail(h, r, s, 0, len(ct))

    # ---- the flattened kernel (rg_flat.hip), a one-packet call: see flat_pieces()
    def flat_pow(self, r, ln, pb):
        """r^pe of a carrying lane as rg_flat.hip:973-978 and pow_step (:222-232) compute it: the first step is a
        choice of 1 or r, every later one squares, multiplies by r and selects; pb is the wave's top bit"""
        pe = ln["pe"]
        multi = ln["c_hi"] - ln["c_lo"] >= 2
        if multi:
            self.ev.add("T:flat_tend_one_chunk")
            if self.mut == "flat_tend_one_chunk":
                pe = (pe + 4 * (ln["c_hi"] - ln["c_lo"] - 1)) & ((2 << pb) - 1)
        one, rr = [1, 0, 0, 0, 0], [r[0], r[1], r[2], r[3], 0]
        if pe == 1:
            self.ev.add("flat:pow_pe==1")
            self.ev.add("T:flat_pe1_as_zero")
            if self.mut == "flat_pe1_as_zero":
                return one
        self.ctx = "pow."
        bit = (pe >> pb) & 1
        if bit:
            self.ev.add("flat:pow_first_takes_r")
            self.ev.add("T:flat_first_skipped")
            if multi:
                self.ev.add("flat:pow_top_bit_in_multi_chunk_lane")
            px = one if self.mut == "flat_first_skipped" else rr
        else:
            self.ev.add("flat:pow_first_takes_1")
            self.ev.add("T:flat_first_always_r")
            px = rr if self.mut == "flat_first_always_r" else one
        ones = 0  # steps that squared x = 1
        for b in range(pb - 1, -1, -1):
            if b == 0:
                self.ev.add("T:flat_skip_bit0")
                if self.mut == "flat_skip_bit0":
                    break
            lead = px == one
            sq = list(px)
            self.acc_sqr_gen(sq)
            xr = list(sq)
            self.acc_mul(xr, r)
            if lead:
                assert sq == one
                ones += 1
            if (pe >> b) & 1:
                self.ev.add("flat:pow_bit_set")
                self.ev.add("T:flat_select_sq_on_set")
                px = sq if self.mut == "flat_select_sq_on_set" else xr
            elif lead:
                self.ev.add("T:flat_lead_zero_takes_mul")
                px = xr if self.mut == "flat_lead_zero_takes_mul" else sq
            else:
                self.ev.add("flat:pow_bit_clear")
                self.ev.add("T:flat_zero_bit_takes_mul")
                px = xr if self.mut == "flat_zero_bit_takes_mul" else sq
        if ones >= 2:
            self.ev.add("flat:pow_squares_1_for>=2_steps")
        self.ctx = ""
        return px

    def flat_sum(self, r, blocks):
        """the packet's accumulator before the length block: per-lane Horner pieces, the carries h r^pe, the five
        64-bit slot sums (add_h, :237-243), phase F's limb walk (:996-1005) and acc_fold (:1006)"""
        L = flat_pieces(16 * len(blocks))
        slots, vals = [0] * 5, []
        for ln in L["lanes"]:
            if ln["c_hi"] == ln["c_lo"]:
                continue  # no chunk: nothing published (its power chain runs on x = 1 and is not used)
            h, _ = self.horner(r, blocks[ln["b0"]:ln["b1"]])
            if ln["carries"]:
                v = self.value(h)
                if v % P == 0:
                    self.ev.add("flat:piece_h==0(mod p)")
                if v >= P:
                    self.ev.add("flat:piece_h>=p")
                    self.ev.add("T:flat_piece_ge_p_saturates")
                    if self.mut == "flat_piece_ge_p_saturates":
                        h = words(P - 1) + [(P - 1) >> 128]
                if h[4] == 4:
                    self.ev.add("flat:piece_h4==4")
                px = self.flat_pow(r, ln, L["pb"])
                self.ctx = "pow."
                G = self.make_gen(px)
                self.ctx = ""
                self.acc_mul_gen(h, G)
                v = self.value(h)
                if v % P <= 5:
                    self.ev.add(f"flat:cv=={v % P}(mod p)")
                if v % P == P - 1:
                    self.ev.add("flat:cv==p-1(mod p)")
                if v >= P:
                    self.ev.add("flat:cv>=p")
                    self.ev.add("T:flat_cv_ge_p_saturates")
                    if self.mut == "flat_cv_ge_p_saturates":
                        h = words(P - 1) + [(P - 1) >> 128]
            vals.append(self.value(h))
            for i in range(5):
                slots[i] += h[i]
        assert len(vals) <= 64 and max(slots) <= M64
        if len(vals) == 2 and 0 < vals[0] < P and vals[0] + vals[1] == P:
            self.ev.add("flat:two_pieces_cancel")
        # phase F: carry the slot sums into 32-bit limbs
        h, t = [0] * 5, 0
        for i in range(4):
            k = t >> 32
            if i:
                if k >= 2:
                    self.ev.add("flat:slot_carry>=2")
                    self.ev.add("T:flat_walk_carry_1bit")
                    if self.mut == "flat_walk_carry_1bit":
                        k &= 1
                if k >= 32:
                    self.ev.add("flat:slot_carry>=32")
                    self.ev.add("T:flat_walk_carry_5bit")
                    if self.mut == "flat_walk_carry_5bit":
                        k &= 31
            t = (k + slots[i]) & M64
            h[i] = t & M32
        k = t >> 32
        if k >= 2:
            self.ev.add("flat:slot_carry>=2")
            self.ev.add("T:flat_walk_carry_1bit")
            if self.mut == "flat_walk_carry_1bit":
                k &= 1
        if k >= 32:
            self.ev.add("flat:slot_carry>=32")
            self.ev.add("T:flat_walk_carry_5bit")
            if self.mut == "flat_walk_carry_5bit":
                k &= 31
        h[4] = (k + slots[4]) & M32
        if self.value(h) % P == 0 and self.value(h) > 0:
            self.ev.add("flat:sum==0(mod p)")
            if self.value(h) == P:
                self.ev.add("flat:sum_limbs==p")
        if h[4] >= 8:
            self.ev.add("flat:h4>=8")
            self.ev.add("T:flat_fold_h4_and7")
            if self.mut == "flat_fold_h4_and7":
                h[4] &= 7
        if h[4] >= 64:
            self.ev.add("flat:h4>=64")
            self.ev.add("T:flat_fold_h4_and63")
            if self.mut == "flat_fold_h4_and63":
                h[4] &= 63
        if (self.value(h) & M128) + 5 * (h[4] >> 2) > M128:
            self.ev.add("flat:fold_carry_out_of_h3" + ("_h4>=8" if h[4] >= 8 else ""))
        self.acc_fold(h)
        return h

    def flat_tag(self, otk: bytes, ct: bytes, direction: str = "seal", tag: bytes | None = None):
        """A one-packet call of the flattened kernel on ciphertext ct (whole blocks).  "seal": the tag (acc_finish
        adds s, :1014).  "open": whether `tag` is accepted: phase A holds tag - s mod 2^128 (:846-852), phase F
        finishes with s = 0 and compares (:1019-1021)."""
        assert len(ct) % 16 == 0 and direction in ("seal", "open")
        k = [int.from_bytes(otk[4 * i:4 * i + 4], "little") for i in range(8)]
        r, s = self.make_mul(k[:4]), k[4:]
        h = self.flat_sum(r, to_blocks(ct))
        self.acc_add(h, [0, 0, len(ct), 0], 1)
        self.acc_mul(h, r)
        v = self.value(h)
        if P <= v < 1 << 130:
            self.ev.add(f"flat:finish_held_p+{v - P}")
        elif v >= 1 << 130:
            self.ev.add(f"flat:finish_held_2^130+{v - (1 << 130)}" if v - (1 << 130) < 2 else "flat:finish_held_>2^130+1")
        if direction == "seal":
            return self.acc_finish(h, s)
        t = [int.from_bytes(tag[4 * i:4 * i + 4], "little") for i in range(4)]
        sw, b, borrows = [0] * 4, 0, []
        for i in range(4):
            if i == 3 and borrows == [1, 1, 1]:
                self.ev.add("T:flat_open_borrow_chain_cut")
                if self.mut == "flat_open_borrow_chain_cut":
                    b = 0
            d = t[i] - s[i] - b
            b = int(d < 0)
            borrows.append(b)
            sw[i] = d & M32
        if all(borrows):
            self.ev.add("flat:open_tag-s_borrows_every_word")
        x = sw[0] | sw[1] << 32 | sw[2] << 64 | sw[3] << 96
        if x == 0:
            self.ev.add("flat:open_tag-s==0")
        if x == M128:
            self.ev.add("flat:open_tag-s==2^128-1")
        return self.acc_finish(h, [0, 0, 0, 0]) == x.to_bytes(16, "little")


SEG_PATHS = {2: ["p2", "t2"], 4: ["p4", "t4"]}
ALL_PATHS = ["h", "p2", "p4", "t2", "t4"]


def vector_paths(v) -> list[str]:
    """the orders of evaluation a vector's events are recorded for"""
    return ["h"] + SEG_PATHS.get(v.get("seg_k", 0), [])


def vector_otk(v) -> bytes:
    key = bytes.fromhex(v["key"])
    if v["kind"] == "batch":
        return one_time_key(key, oracle.wg_nonce(v["counter"]))
    nonce = bytes.fromhex(v["nonce"])
    if v["kind"] == "xmsg":
        key, nonce = xchacha_inner(key, nonce)
    return one_time_key(key, nonce)


def model_events(v, mutant=None) -> tuple[list[str], dict[str, bytes]]:
    """(events as "path:event", tag per path) of a fixture vector under the model"""
    otk, aad, ct = vector_otk(v), bytes.fromhex(v["aad"]), bytes.fromhex(v["ct"])
    ev, tags = set(), {}
    for path in vector_paths(v):
        m = Limbs(mutant)
        tags[path] = m.tag(otk, aad, ct, path)
        ev |= {f"{path}:{e}" for e in m.ev}
    return sorted(ev), tags


def random_message(rng: random.Random):
    """a random packet for the model: a one-time key and 0..16 whole ciphertext blocks"""
    return rng.randbytes(32), rng.randbytes(16 * rng.randrange(0, 17))


def frame_batch(vectors, filler_seed=None):
    """The aligned, empty-AAD vectors as one batch of data frames [header 16][ciphertext][tag 16] over the
    include/rg_aead.h buffer contract, one key row per frame.  With filler_seed, 0..2 random frames of
    0..624 bytes (sealed by the C oracle) go in front of every vector.  Returns a dict: keys, receivers,
    counters, desc_seal (len = P), desc_open (len = P + 32), sealed (the buffer), plain (the same buffer
    opened by the C oracle), vec (indices of the vectors in the batch), vectors."""
    import numpy as np

    vs = [v for v in vectors if v["kind"] == "batch"]
    rng = np.random.default_rng(filler_seed)
    items = []
    for v in vs:
        if filler_seed is not None:
            items += [None] * int(rng.integers(0, 3))
        items.append(v)
    n = len(items)
    keys = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    counters = rng.integers(0, 2**62, n, dtype=np.uint64)
    receivers = rng.integers(1, 2**32, n, dtype=np.uint64).astype(np.uint32)
    sizes = np.array([16 * int(rng.integers(0, 40)) if v is None else len(v["ct"]) // 2 for v in items], np.int64)
    gaps = rng.integers(0, 3, n) * 16
    desc = np.zeros(n, oracle.DESC_DTYPE)
    desc["offset"] = np.concatenate([[0], np.cumsum(sizes + 32 + gaps)[:-1]])
    desc["len"] = sizes
    desc["key_idx"] = np.arange(n)
    buf = rng.integers(0, 256, int(desc["offset"][-1]) + int(sizes[-1]) + 32 + 64, dtype=np.uint8)
    fill = np.array([v is None for v in items])
    if fill.any():
        oracle.seal_batch(keys, receivers, desc[fill], counters[fill], buf)
    for i, v in enumerate(items):
        if v is None:
            continue
        keys[i] = np.frombuffer(bytes.fromhex(v["key"]), np.uint8)
        counters[i] = v["counter"]
        o, frame = int(desc["offset"][i]), b"".join([(4).to_bytes(4, "little"), int(receivers[i]).to_bytes(4, "little"),
                                                     v["counter"].to_bytes(8, "little"), bytes.fromhex(v["ct"]),
                                                     bytes.fromhex(v["tag"])])
        buf[o:o + len(frame)] = np.frombuffer(frame, np.uint8)
    od = desc.copy()
    od["len"] += 32
    plain = buf.copy()
    st, ctr = oracle.open_batch(keys, od, plain)
    assert (st == 0).all() and np.array_equal(ctr, counters)
    return {"keys": keys, "receivers": receivers, "counters": counters, "desc_seal": desc, "desc_open": od,
            "sealed": buf, "plain": plain, "vec": np.nonzero(~fill)[0], "vectors": vs}


# ------------------------------------------------------------------ generation
class Gen:
    def __init__(self):
        self.rng = random.Random(SEED)
        self.vectors = []
        self.tries = []

    def rs(self, otk):
        return clamp(int.from_bytes(otk[:16], "little")), int.from_bytes(otk[16:32], "little")

    def emit(self, cls, label, kind, key, ctr_or_nonce, aad, ct, extra=None):
        v = {"id": len(self.vectors), "class": cls, "label": label, "kind": kind, "key": key.hex()}
        if kind == "batch":
            v["counter"] = ctr_or_nonce
        else:
            v["nonce"] = ctr_or_nonce.hex()
        v["aad"], v["ct"] = aad.hex(), ct.hex()
        v.update(extra or {})
        otk = vector_otk(v)
        tag = ref_tag(otk, mac_input(aad, ct))
        v["tag"] = tag.hex()
        ev, tags = model_events(v)
        assert all(t == tag for t in tags.values()), (label, tags, tag.hex())
        v["events"] = [e for e in ev if ":T:" not in e]
        self.vectors.append(v)
        return v

    def batch(self, cls, label, nb, steps, extra=None, accept=None, fixed=None):
        """steps: [(free block k, F(r, s) -> functional, T(r, s) -> target, blocks to redraw)].  A try
        draws counter and filler; a step that names blocks to redraw retries on those alone."""
        rng = self.rng
        key = rng.randbytes(32)
        for t0 in range(256):
            for _ in range(4096):
                ctr = rng.getrandbits(rng.choice([8, 32, 48, 62]))
                r, s = self.rs(one_time_key(key, oracle.wg_nonce(ctr)))
                if accept is None or accept(r, s):
                    break
            else:
                raise RuntimeError(f"no counter with the wanted r: {label}")
            blocks = [rng.getrandbits(128) for _ in range(nb)] + [(16 * nb) << 64]
            for i, v in (fixed or {}).items():
                blocks[i] = v
            for k, F, T, redraw in steps:
                x = None
                for t1 in range(256 if redraw else 1):
                    if t1:
                        for i in redraw:
                            blocks[i] = rng.getrandbits(128)
                    x = solve_block(F(r, s), blocks, k, T(r, s) % P)
                    if x is not None:
                        break
                if x is None:
                    if redraw:
                        raise RuntimeError(f"target not met: {label}")
                    break
                blocks[k] = x
                assert F(r, s)(blocks) == T(r, s) % P
            else:
                self.tries.append(t0 + 1)
                ct = b"".join(b.to_bytes(16, "little") for b in blocks[:nb])
                return self.emit(cls, label, "batch", key, ctr, b"", ct, extra)
        raise RuntimeError(f"target not met: {label}")

    def message(self, cls, label, kind, aad_len, ct_len, T):
        """per-message shape: the free block is the AAD block (16-byte AAD) or the first ciphertext block"""
        rng = self.rng
        key = rng.randbytes(32)
        for t0 in range(256):
            nonce = rng.randbytes(12 if kind == "msg" else 24)
            k2, n2 = (key, nonce) if kind == "msg" else xchacha_inner(key, nonce)
            r, s = self.rs(one_time_key(k2, n2))
            aad, ct = rng.randbytes(aad_len), rng.randbytes(ct_len)
            blocks = to_blocks(mac_input(aad, ct))
            if aad_len == 16:
                k = 0
            else:
                assert ct_len >= 16
                k = len(pad16(aad)) // 16
            x = solve_block(F_state(r, len(blocks) - 1), blocks, k, T(r, s) % P)
            if x is None:
                continue
            blocks[k] = x
            raw = b"".join(b.to_bytes(16, "little") for b in blocks[:-1])
            na = len(pad16(aad))
            aad, ct = raw[:na][:aad_len], raw[na:][:ct_len]
            self.tries.append(t0 + 1)
            return self.emit(cls, label, kind, key, nonce, aad, ct)
        raise RuntimeError(f"target not met: {label}")


def final_targets(rng):
    """(label, T(r, s)) of the final state, after the lengths block"""
    c = lambda v: (lambda r, s: v)  # noqa: E731
    out = [(f"{t} (held as p+{t})", c(t)) for t in range(5)]
    out += [("5 (held as 2^130)", c(5)), ("6 (held as 2^130+1)", c(6)),
            ("2^32+4", c((1 << 32) + 4)), ("2^32+5", c((1 << 32) + 5))]
    out += [(f"p-{d}", c(P - d)) for d in range(1, 7)]
    out += [("2^128-1", c(HI - 1)), ("2^128", c(HI)), ("2^129-1", c(2 * HI - 1)), ("2^129", c(2 * HI)),
            ("3*2^128-1", c(3 * HI - 1))]
    for h0 in range(0xFFFFFFFB, 0x100000000):
        v = h0 | (M64 << 32) | rng.getrandbits(32) << 96 | rng.randrange(4) << 128
        if v >= P:
            v -= HI
        out.append((f"low words {h0:#x},ff..,ff.. random h3", c(v)))
    out += [("tag all-zero", lambda r, s: (-s) & M128), ("tag all-ones", lambda r, s: (M128 - s) & M128),
            ("T+s carries through all four words", lambda r, s: ((-s) & M128) + 1)]
    return out


SMALL = [(str(t), t) for t in range(6)] + [("p-1", P - 1)]


def generate() -> dict:
    g = Gen()
    rng = g.rng
    sizes = [32, 64, 96, 272]
    # ---- final state
    for i, (label, T) in enumerate(final_targets(rng)):
        nb = sizes[i % 4] // 16
        g.batch("final", f"final state = {label}", nb,
                [(rng.randrange(nb), lambda r, s, nb=nb: F_state(r, nb), T, [])])
    # ---- state before the lengths block
    pre = SMALL + [("3*2^128-1: low 128 bits + (P << 64) carry out of h3", 3 * HI - 1)]
    for i, (label, t) in enumerate(pre):
        nb = sizes[i % 4] // 16
        g.batch("pre_length", f"state after the last data block = {label}", nb,
                [(rng.randrange(nb), lambda r, s, nb=nb: F_state(r, nb - 1), lambda r, s, t=t: t, [])])
    # ---- state after a middle block, two or more random blocks after it
    for i, (label, t) in enumerate(SMALL):
        nb = [64, 96, 272][i % 3] // 16
        j = rng.randrange(0, nb - 2)
        g.batch("intermediate", f"state after block {j} of {nb} = {label}", nb,
                [(rng.randrange(j + 1), lambda r, s, j=j: F_state(r, j), lambda r, s, t=t: t, [])])
    # state 6 = 2^130 + 1 followed by an all-ones block: acc_add leaves h4 = 4 + 1 + carry = 6
    for nb in (6, 17):
        j = nb // 2
        g.batch("intermediate", f"state after block {j} of {nb} = 6, then an all-ones block", nb,
                [(j, lambda r, s, j=j: F_state(r, j), lambda r, s: 6, [])], fixed={j + 1: M128})
    # ---- segment partial sums
    n = 0
    for K in (2, 4):
        for nb in (16, 20, 33):
            live = [j for j in range(K) if split(nb, K, j)[1] > split(nb, K, j)[0]]
            pos = [("first", live[0]), ("last", live[-1])] if K == 2 else \
                  [("first", live[0]), ("middle", live[1]), ("last", live[-1])]
            for pname, j in pos:
                b0, b1, after = split(nb, K, j)
                for shifted in (False, True, n % 2 == 0):
                    label_t, t = SMALL[n % len(SMALL)]
                    n += 1
                    what = f"A_{j} r^{after}" if shifted else f"A_{j}"
                    g.batch("segment", f"K={K} nb={nb} {pname} segment (blocks {b0}..{b1 - 1}): {what} = {label_t}", nb,
                            [(rng.randrange(b0, b1), lambda r, s, nb=nb, K=K, j=j, sh=shifted: F_seg(r, nb, K, j, sh),
                              lambda r, s, t=t: t, [])], {"seg_k": K})
    # ---- shifted partials that cancel, sums that carry out of the fold
    for label, t in (("0", 0), ("p-1", P - 1)):
        g.batch("segment_sum", f"K=4 nb=16: A_0 r^12 + A_1 r^8 = {label}", 16,
                [(5, lambda r, s: F_sum(r, 16, 4, [0, 1]), lambda r, s, t=t: t, [])], {"seg_k": 4})
        g.batch("segment_sum", f"K=2 nb=20: A_0 r^8 + A_1 = {label} (state before the lengths block)", 20,
                [(14, lambda r, s: F_sum(r, 20, 2, [0, 1]), lambda r, s, t=t: t, [])], {"seg_k": 2})
    g.batch("segment_sum", "K=4 nb=33: tile running value (A_0 q_1 + A_1) q_2 + A_2 = p-1", 33,
            [(30, lambda r, s: F_tile_run(r, 33, 4, 2), lambda r, s: P - 1, [])], {"seg_k": 4})
    g.batch("segment_sum", "K=4 nb=20: tile running value A_0 q_1 + A_1 = 4", 20,
            [(9, lambda r, s: F_tile_run(r, 20, 4, 1), lambda r, s: 4, [])], {"seg_k": 4})
    # both shifted partials = p + 4 = 2^130 - 1: the sum 2^131 - 2 folds with a carry out of h3
    for nb in (16, 33):
        b = [split(nb, 2, j) for j in range(2)]
        g.batch("segment_sum", f"K=2 nb={nb}: A_0 r^{b[0][2]} = 4 and A_1 = 4 (sum 2^131-2: the fold carries)", nb,
                [(1, lambda r, s, nb=nb: F_seg(r, nb, 2, 0, True), lambda r, s: 4, list(range(b[0][0], b[0][1]))),
                 (b[1][0] + 1, lambda r, s, nb=nb: F_seg(r, nb, 2, 1, True), lambda r, s: 4,
                  list(range(b[1][0], b[1][1])))], {"seg_k": 2})
    # four shifted partials of p - 1 under a large r: without the folds h4 reaches 16 and acc_mul's w4 wraps
    def big_r(r, s):
        rw = words(r)
        return 17 * rw[0] + rw[1] + rw[2] + rw[3] >= (1 << 32) + (1 << 27)
    for nb in (16, 32):
        segs = [split(nb, 4, j) for j in range(4)]
        live = [j for j in range(4) if segs[j][1] > segs[j][0]]
        steps = [(segs[j][0], lambda r, s, nb=nb, j=j: F_seg(r, nb, 4, j, True), lambda r, s: P - 1,
                  list(range(segs[j][0], segs[j][1]))) for j in live]
        g.batch("segment_sum", f"K=4 nb={nb}: every shifted partial = p-1, large r (h4 = 16 without the folds)", nb,
                steps, {"seg_k": 4}, accept=big_r)
    # ---- per-message shapes (final-state targets only)
    shapes = [(16, 1), (16, 15), (16, 17), (16, 100), (0, 17), (0, 100), (12, 17), (12, 100)]
    fin = [("0 (held as p+0)", lambda r, s: 0), ("4 (held as p+4)", lambda r, s: 4), ("5 (held as 2^130)", lambda r, s: 5),
           ("p-1", lambda r, s: P - 1), ("tag all-zero", lambda r, s: (-s) & M128),
           ("T+s carries through all four words", lambda r, s: ((-s) & M128) + 1)]
    for kind in ("msg", "xmsg"):
        n = 0
        for aad_len, ct_len in shapes:
            for _ in range(3):
                label, T = fin[n % len(fin)]
                n += 1
                name = "ChaCha20-Poly1305" if kind == "msg" else "XChaCha20-Poly1305"
                g.message("message" if kind == "msg" else "xmessage",
                          f"{name} aad={aad_len} len={ct_len}: final state = {label}", kind, aad_len, ct_len, T)
    return {"generator": "tests/golden/make_poly_edges.py", "seed": SEED, "p": "2^130-5",
            "solver_tries": {"mean": round(sum(g.tries) / len(g.tries), 2), "max": max(g.tries)},
            "vectors": g.vectors}


# ------------------------------------------------- the flat kernel's own fixture
def flat_vector_ct(v) -> bytes:
    """the ciphertext of a flat vector: filler bytes from its seed, the solved blocks put over them"""
    ct = bytearray(random.Random(v["seed"]).randbytes(v["P"]))
    for i, hx in v["solved"]:
        ct[16 * i:16 * i + 16] = bytes.fromhex(hx)
    return bytes(ct)


def flat_vector_otk(v) -> bytes:
    return one_time_key(bytes.fromhex(v["key"]), oracle.wg_nonce(v["counter"]))


def flat_model(v, mutant=None, ct=None):
    """a flat vector under the model, both directions: {"seal": (events, tag), "open": (events, accepted)}"""
    otk, ct = flat_vector_otk(v), flat_vector_ct(v) if ct is None else ct
    out = {}
    for d in ("seal", "open"):
        m = Limbs(mutant)
        res = m.flat_tag(otk, ct, d, bytes.fromhex(v["tag"]))
        out[d] = (sorted(m.ev), res)
    return out


def flat_frame(v, pad=(48, 80), fill_seed=5):
    """The vector as a one-packet call over the include/rg_aead.h buffer contract: random bytes, the frame
    [header 16][ciphertext][tag 16] at offset pad[0], pad[1] random bytes behind it.  Returns a dict as
    frame_batch does (plain: the buffer opened by the C oracle)."""
    import numpy as np

    rng = np.random.default_rng(fill_seed + v["id"])
    ct, P_ = flat_vector_ct(v), v["P"]
    keys = np.frombuffer(bytes.fromhex(v["key"]), np.uint8).reshape(1, 32).copy()
    counters = np.array([v["counter"]], np.uint64)
    receivers = rng.integers(1, 2**32, 1, dtype=np.uint64).astype(np.uint32)
    desc = np.zeros(1, oracle.DESC_DTYPE)
    desc["offset"], desc["len"], desc["key_idx"] = pad[0], P_, 0
    buf = rng.integers(0, 256, pad[0] + P_ + 32 + pad[1], dtype=np.uint8)
    frame = b"".join([(4).to_bytes(4, "little"), int(receivers[0]).to_bytes(4, "little"),
                      v["counter"].to_bytes(8, "little"), ct, bytes.fromhex(v["tag"])])
    buf[pad[0]:pad[0] + len(frame)] = np.frombuffer(frame, np.uint8)
    od = desc.copy()
    od["len"] += 32
    plain = buf.copy()
    st, ctr = oracle.open_batch(keys, od, plain)
    assert (st == 0).all() and np.array_equal(ctr, counters)
    return {"keys": keys, "receivers": receivers, "counters": counters, "desc_seal": desc, "desc_open": od,
            "sealed": buf, "plain": plain, "at": pad[0], "P": P_}


class FlatGen:
    def __init__(self):
        self.rng = random.Random(FLAT_SEED)
        self.vectors = []
        self.tries = []

    def vector(self, label, P_, steps, want=()):
        """steps: [(lane, what, T)] with what = "h" (the lane's Horner piece from zero), "cv" (h r^pe, the value
        the lane publishes), "pre" (the packet's sum before the length block) or "final" (the state acc_finish
        gets), T an integer or f(r, s).  The free block is the first block of the lane's piece; a retry redraws
        the piece's second block (recorded with the solved ones), or, where the piece has one block, the
        counter.  "pre" and "final" come last and use a lane no other step uses.  want: events the model must
        record in both directions ("open:" in front: in the open alone)."""
        rng, L = self.rng, flat_pieces(P_)
        nb = L["nb"]
        key = rng.randbytes(32)
        for t0 in range(256):
            ctr = rng.getrandbits(rng.choice([8, 32, 48, 62]))
            otk = one_time_key(key, oracle.wg_nonce(ctr))
            r, s = clamp(int.from_bytes(otk[:16], "little")), int.from_bytes(otk[16:32], "little")
            seed = rng.getrandbits(32)
            blocks = to_blocks(random.Random(seed).randbytes(P_)) + [P_ << 64]
            solved = {}
            for lane, what, T in steps:
                ln = L["lanes"][lane]
                b0, b1, pe = ln["b0"], ln["b1"], ln["pe"]
                assert b1 > b0 and b0 not in solved
                F = {"h": lambda b: ref_state(r, b[b0:b1]),
                     "cv": lambda b: ref_state(r, b[b0:b1]) * pow(r, pe, P) % P,
                     "pre": lambda b: ref_state(r, b[:nb]),
                     "final": lambda b: ref_state(r, b)}[what]
                target = (T(r, s) if callable(T) else T) % P
                x = None
                for t1 in range(64):
                    x = solve_block(F, blocks, b0, target)
                    if x is not None or b1 - b0 < 2:
                        break
                    blocks[b0 + 1] = solved[b0 + 1] = rng.getrandbits(128)
                if x is None:
                    break
                blocks[b0] = solved[b0] = x
                assert F(blocks) == target
            else:
                self.tries.append(t0 + 1)
                return self.emit(label, P_, key, ctr, seed, solved, blocks[:nb], want)
        raise RuntimeError(f"target not met: {label}")

    def emit(self, label, P_, key, ctr, seed, solved, blocks, want):
        ct = b"".join(b.to_bytes(16, "little") for b in blocks)
        v = {"id": len(self.vectors), "label": label, "P": P_, "key": key.hex(), "counter": ctr, "seed": seed,
             "solved": [[i, solved[i].to_bytes(16, "little").hex()] for i in sorted(solved)]}
        assert flat_vector_ct(v) == ct
        tag = ref_tag(flat_vector_otk(v), mac_input(b"", ct))
        v["tag"] = tag.hex()
        res = flat_model(v, ct=ct)
        assert res["seal"][1] == tag and res["open"][1] is True, label
        ev = {d: {e for e in res[d][0] if not e.startswith("T:")} for d in res}
        for w in want:
            assert (w[5:] in ev["open"]) if w.startswith("open:") else (w in ev["seal"] and w in ev["open"]), (label, w)
        v["events"] = sorted(ev["seal"] & ev["open"])
        v["events_seal"] = sorted(ev["seal"] - ev["open"])
        v["events_open"] = sorted(ev["open"] - ev["seal"])
        self.vectors.append(v)
        return v


def flat_old_fixture_finish(vectors) -> dict:
    """The acc_finish branches that the batch vectors of poly1305_edges.json take in straight Horner order ("h")
    and as one-packet calls of the flat kernel ("flat"), by branch name -> number of vectors: the flat
    kernel's state before acc_finish is another representative of the same value mod p."""
    out = {"h": {}, "flat": {}}
    for v in vectors:
        if v["kind"] != "batch":
            continue
        otk, ct = vector_otk(v), bytes.fromhex(v["ct"])
        a, b = Limbs(), Limbs()
        assert a.tag(otk, b"", ct, "h") == b.flat_tag(otk, ct) == bytes.fromhex(v["tag"])
        for name, m in (("h", a), ("flat", b)):
            for e in m.ev:
                if e.startswith("acc_finish:"):
                    out[name][e] = out[name].get(e, 0) + 1
    return out


def generate_flat() -> dict:
    g = FlatGen()
    c = lambda v: (lambda r, s: v)  # noqa: E731
    small = [(str(t), t) for t in range(7)] + [("p-1", P - 1)]
    # ---- P = 128: two 4-block pieces (lanes 31 and 63), pe = 4: r, then two squarings
    for name, t in small:
        want = ["flat:piece_h>=p"] if t < 5 else ["flat:piece_h4==4", "to26:l4>=2^26"] if t < 7 else []
        g.vector(f"P=128: carrying piece h = {name}", 128, [(31, "h", t)], want + (["flat:piece_h==0(mod p)"] if t == 0 else []))
    for name, t in small[:6] + small[7:]:
        g.vector(f"P=128: carry h r^4 = {name}", 128, [(31, "cv", t)], [f"flat:cv=={name}(mod p)"])
    x = g.rng.getrandbits(129)
    g.vector("P=128: carry = x, last piece = p - x (the sum's limbs are exactly p)", 128,
             [(31, "cv", x), (63, "h", P - x)], ["flat:two_pieces_cancel", "flat:sum_limbs==p", "flat:sum==0(mod p)"])
    # ---- P = 80: a 4-block piece with pe = 1 and a 1-block piece
    g.vector("P=80: carrying piece h = 0, pe = 1", 80, [(31, "h", 0)], ["flat:pow_pe==1", "flat:piece_h==0(mod p)"])
    g.vector("P=80: carry h r = p-1", 80, [(31, "cv", P - 1)], ["flat:pow_pe==1", "flat:cv==p-1(mod p)"])
    g.vector("P=80: carry h r = 5 (h4 == 4 into the slots)", 80, [(31, "cv", 5)], ["flat:cv==5(mod p)"])
    g.vector("P=80: carry = 4, last piece = 4 (both held as 2^130 - 1)", 80, [(31, "cv", 4), (63, "h", 4)],
             ["flat:cv>=p"])
    # ---- the final state and the open's compare, through every layout
    fin = [(f"{t} (held as p+{t})", c(t), [f"flat:finish_held_p+{t}", "acc_finish:use_g"]) for t in range(5)]
    fin += [("5 (held as 2^130)", c(5), ["flat:finish_held_2^130+0", "acc_finish:fold_h4>=4"]),
            ("6 (held as 2^130+1)", c(6), ["flat:finish_held_2^130+1", "acc_finish:fold_h4>=4"]),
            ("p-1", c(P - 1), []),
            ("low words fffffffb,ff..,ff.. (h + 5 carries through three words)",
             c((1 << 96) - 5 | 0x12345678 << 96 | 2 << 128), []),
            ("tag = s (tag - s = 0)", c(0), ["open:flat:open_tag-s==0"]),
            ("2^128-1 (tag - s = 2^128 - 1)", c(M128), ["open:flat:open_tag-s==2^128-1"]),
            ("tag = 1 (T + s carries, tag - s borrows through every word)", lambda r, s: ((-s) & M128) + 1,
             ["open:flat:open_tag-s_borrows_every_word"])]
    sizes = [80, 128, 1504, 4096, 4112, 8208]
    for i, (name, T, want) in enumerate(fin):
        for P_ in (sizes[i % 6], sizes[(i + 3) % 6]):
            lanes = [l for l, ln in enumerate(flat_pieces(P_)["lanes"]) if ln["b1"] - ln["b0"] >= 2]
            g.vector(f"P={P_}: final state = {name}", P_, [(lanes[g.rng.randrange(len(lanes))], "final", T)], want)
    # ---- P = 1504 (24 pieces, exponents 90 .. 2, a 2-block last chunk)
    live = [l for l, ln in enumerate(flat_pieces(1504)["lanes"]) if ln["c_hi"] > ln["c_lo"]]
    assert len(live) == 24
    for name, t in (("0", 0), ("3", 3), ("5", 5), ("p-1", P - 1)):
        g.vector(f"P=1504: first lane's piece h = {name}, last carrying lane's carry h r^2 = {name}", 1504,
                 [(live[0], "h", t), (live[-2], "cv", t)],
                 ["flat:pow_squares_1_for>=2_steps", "flat:pow_first_takes_1", "flat:pow_first_takes_r"])
    g.vector("P=1504: sum of the 24 pieces = 0", 1504, [(live[11], "pre", 0)], ["flat:sum==0(mod p)", "flat:h4>=8"])
    g.vector("P=1504: every piece = p-1", 1504, [(l, "cv", P - 1) for l in live], ["flat:slot_carry>=2", "flat:h4>=64"])
    # ---- P = 4096: 64 pieces of one chunk
    g.vector("P=4096: every piece = p-1 (the largest slot sums and h4)", 4096, [(l, "cv", P - 1) for l in range(64)],
             ["flat:slot_carry>=32", "flat:h4>=64", "flat:cv==p-1(mod p)"])
    g.vector("P=4096: 63 pieces = p-1, the last = 377 (the fold of the large h4 carries out of h3)", 4096,
             [(l, "cv", P - 1) for l in range(63)] + [(63, "h", 377)], ["flat:fold_carry_out_of_h3_h4>=8"])
    g.vector("P=4096: every carry = 0 (held as p), last piece = 0", 4096, [(l, "cv", 0) for l in range(64)],
             ["flat:cv==0(mod p)", "flat:sum==0(mod p)"])
    g.vector("P=4096: every carrying piece h = 6 (held as 2^130 + 1)", 4096, [(l, "h", 6) for l in range(63)],
             ["flat:piece_h4==4"])
    # ---- P = 4112: lane 63 holds two chunks (the second of one block)
    g.vector("P=4112: the two-chunk last piece = p-1, lane 62's carry h r^5 = p-1", 4112,
             [(62, "cv", P - 1), (63, "h", P - 1)], ["flat:cv==p-1(mod p)"])
    g.vector("P=4112: sum of the 64 pieces = 0", 4112, [(63, "pre", 0)], ["flat:sum==0(mod p)"])
    # ---- P = 8208: two and three chunks per lane, 9-bit exponents
    for name, t in (("0", 0), ("4", 4), ("6", 6), ("p-1", P - 1)):
        g.vector(f"P=8208: lane 0's piece (two chunks, the top exponent bit) h = {name}; lane 31's carry (three "
                 f"chunks) = {name}", 8208, [(0, "h", t), (31, "cv", t)], ["flat:pow_top_bit_in_multi_chunk_lane"])
    g.vector("P=8208: every piece = p-1", 8208, [(l, "cv", P - 1) for l in range(64)], ["flat:slot_carry>=32"])
    # ---- P = 65536: 16 chunks a lane, 12-bit exponents
    g.vector("P=65536: every piece = p-1", 65536, [(l, "cv", P - 1) for l in range(64)], ["flat:h4>=64"])
    g.vector("P=65536: lane 0's piece h = 0, lane 62's carry = 5, final state = 0 (held as p+0)", 65536,
             [(0, "h", 0), (62, "cv", 5), (40, "final", 0)], ["flat:finish_held_p+0", "flat:piece_h==0(mod p)"])
    return {"generator": "tests/golden/make_poly_edges.py", "seed": FLAT_SEED, "p": "2^130-5",
            "unreachable": FLAT_UNREACHABLE,
            "solver_tries": {"mean": round(sum(g.tries) / len(g.tries), 2), "max": max(g.tries)},
            "vectors": g.vectors}


def dumps(data) -> str:
    return json.dumps(data, indent=0, separators=(",", ":")) + "\n"


def main():
    oracle.build()
    data = generate()
    with open(FIXTURE, "w") as f:
        f.write(dumps(data))
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes,", len(data["vectors"]), "vectors, solver tries",
          data["solver_tries"])
    flat = generate_flat()
    with open(FLAT_FIXTURE, "w") as f:
        f.write(dumps(flat))
    print("wrote", FLAT_FIXTURE, os.path.getsize(FLAT_FIXTURE), "bytes,", len(flat["vectors"]), "vectors, solver tries",
          flat["solver_tries"])
    print("acc_finish branches of the first fixture's batch vectors, straight and through the flat path:",
          flat_old_fixture_finish(data["vectors"]))


if __name__ == "__main__":
    main()
