"""The Python model of the Noise IKpsk2 responder path and the case builders of its tests.

X25519 is RFC 7748 §5 over Python integers; HMAC / HKDF are the reference's constructions over
hashlib.blake2s (rustyguard-crypto/src/prim.rs:41-72, :145-157); the AEAD is the CPU oracle's
(aead_seal / aead_open with an AAD).  The responder steps restate decrypt_handshake_init,
encrypt_handshake_resp (rustyguard-crypto/src/lib.rs:346-433) and HandshakeState::split (prim.rs:299-313)
with the statuses of include/rg_aead.h; the initiator steps are their mirror images, so that the tests can
make valid messages and finish the handshake on the other side.  tests/golden/handshake_full.json pins
this model to the reference's recorded messages.
"""
from __future__ import annotations

import functools
import hashlib

import numpy as np

from oracle import oracle

OK, DECRYPT_ERR, INVALID, REJECTED, UNALIGNED = 0, 1, 2, 3, 4
KEYEXCHANGE = 8
PEER_NONE = 0xFFFFFFFF
KEY_SKIP = 0xFFFFFFFF

P = 2**255 - 19
NONCE0 = b"\0" * 12


# ------------------------------------------------------------------- X25519
@functools.lru_cache(maxsize=None)
def x25519(k: bytes, u: bytes) -> bytes:
    """RFC 7748 §5: clamped scalar, bit 255 of u masked, non-canonical u accepted."""
    kb = bytearray(k)
    kb[0] &= 248
    kb[31] &= 127
    kb[31] |= 64
    kk = int.from_bytes(kb, "little")
    x1 = (int.from_bytes(u, "little") & ((1 << 255) - 1)) % P
    x2, z2, x3, z3, swap = 1, 0, x1, 1, 0
    for t in reversed(range(255)):
        kt = (kk >> t) & 1
        if swap ^ kt:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = kt
        a, b = (x2 + z2) % P, (x2 - z2) % P
        aa, bb = a * a % P, b * b % P
        e = (aa - bb) % P
        c, d = (x3 + z3) % P, (x3 - z3) % P
        da, cb = d * a % P, c * b % P
        x3 = (da + cb) ** 2 % P
        z3 = x1 * (da - cb) ** 2 % P
        x2 = aa * bb % P
        z2 = e * (aa + 121665 * e) % P
    if swap:
        x2, x3, z2, z3 = x3, x2, z3, z2
    return (x2 * pow(z2, P - 2, P) % P).to_bytes(32, "little")


BASE = (9).to_bytes(32, "little")


def pubkey(sk: bytes) -> bytes:
    return x25519(sk, BASE)


def le(x: int) -> bytes:
    return x.to_bytes(32, "little")


# u-coordinates the kernel must treat exactly as RFC 7748 says: the points of small order (all-zero
# result, RG_PKT_KEYEXCHANGE), their non-canonical encodings, and values around the modulus and the
# masked top bit.  2^256 - 1 masks to 2^255 - 1 = p + 18, i.e. u = 18.
ORDER8_A = bytes.fromhex("e0eb7a7c3b41b8ae1656e3faf19fc46ada098deb9c32b1fd866205165f49b800")
ORDER8_B = bytes.fromhex("5f9c95bca3508c24b1d0b1559c83ef5b04445cc4581c8e86d8224eddd09f1157")
EDGE_POINTS = [("0", le(0)), ("1", le(1)), ("order8_a", ORDER8_A), ("order8_b", ORDER8_B), ("p-1", le(P - 1)),
               ("p", le(P)), ("p+1", le(P + 1)), ("2^255-1", le(2**255 - 1)), ("2^256-1", le(2**256 - 1)),
               ("2^255", le(2**255)), ("18", le(18))]
RFC_SCALAR = bytes.fromhex("a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4")
EDGE_SCALARS = [RFC_SCALAR, bytes(32), b"\xff" * 32]


@functools.lru_cache(maxsize=None)
def rfc_iteration(n: int):
    """The (k, u) inputs of the first n steps of RFC 7748 §5.2's iteration and the value of k after them."""
    k = u = BASE
    pairs = []
    for _ in range(n):
        pairs.append((k, u))
        k, u = x25519(k, u), k
    return pairs, k


# ------------------------------------------------------- BLAKE2s, HMAC, HKDF
def h2(a: bytes, b: bytes = b"") -> bytes:
    return hashlib.blake2s(a + b).digest()


def mac(key: bytes, msg: bytes) -> bytes:
    return hashlib.blake2s(msg, key=key, digest_size=16).digest()


def hmac(key: bytes, msg: bytes) -> bytes:
    k = key.ljust(64, b"\0")
    inner = hashlib.blake2s(bytes(x ^ 0x36 for x in k) + msg).digest()
    return hashlib.blake2s(bytes(x ^ 0x5C for x in k) + inner).digest()


def hkdf(chain: bytes, msg: bytes, n: int):
    """hkdf_blake2s: (the new chain, n further outputs)."""
    prk = hmac(chain, msg)
    t = hmac(prk, b"\x01")
    chain2, out = t, []
    for i in range(n):
        t = hmac(prk, t + bytes([i + 2]))
        out.append(t)
    return chain2, out


def mac1_key(pk: bytes) -> bytes:
    return h2(b"mac1----", pk)


CONSTRUCTION = h2(b"Noise_IKpsk2_25519_ChaChaPoly_BLAKE2s")
IDENTIFIER = h2(CONSTRUCTION, b"WireGuard v1 zx2c4 Jason@zx2c4.com")


class HS:
    """HandshakeState (prim.rs:227-313)."""

    def __init__(self, chain: bytes = CONSTRUCTION, hash_: bytes = IDENTIFIER):
        self.chain, self.hash = chain, hash_

    def mix_hash(self, b):
        self.hash = h2(self.hash, b)

    def mix_chain(self, b):
        self.chain, _ = hkdf(self.chain, b, 0)

    def mix_key(self, b):
        self.chain, (k,) = hkdf(self.chain, b, 1)
        return k

    def mix_key_and_hash(self, b):
        self.chain, (t, k) = hkdf(self.chain, b, 2)
        self.mix_hash(t)
        return k

    def split(self):
        """(k1, k2): the initiator sends under k1 and the responder under k2."""
        chain, (k2,) = hkdf(self.chain, b"", 1)
        return chain, k2


def seal(key, aad, pt) -> bytes:
    ct, tag = oracle.aead_seal(key, NONCE0, aad, pt)
    return ct + tag


def open_(key, aad, field: bytes):
    return oracle.aead_open(key, NONCE0, aad, field[:-16], field[-16:])


# ------------------------------------------------------------ initiator side
def make_initiation(sk_i: bytes, pk_r: bytes, esk_i: bytes, ts: bytes, sender: int, static: bytes | None = None):
    """encrypt_handshake_init with mac2 zero.  static: the public key sealed in the static field (default:
    sk_i's own); the ss secret is always DH(sk_i, pk_r), so another value gives a message whose static field
    opens and whose timestamp tag fails -- unless the responder's DH with it fails first.
    Returns (the 148 bytes, the initiator's HS after them)."""
    epk = pubkey(esk_i)
    hs = HS()
    hs.mix_hash(pk_r)
    hs.mix_hash(epk)
    hs.mix_chain(epk)
    k = hs.mix_key(x25519(esk_i, pk_r))
    f_static = seal(k, hs.hash, pubkey(sk_i) if static is None else static)
    hs.mix_hash(f_static)
    k = hs.mix_key(x25519(sk_i, pk_r))
    f_ts = seal(k, hs.hash, ts)
    hs.mix_hash(f_ts)
    msg = (1).to_bytes(4, "little") + sender.to_bytes(4, "little") + epk + f_static + f_ts
    msg += mac(mac1_key(pk_r), msg) + bytes(16)
    assert len(msg) == 148
    return msg, hs


def finish_initiator(resp: bytes, hs: HS, sk_i: bytes, esk_i: bytes, psk: bytes):
    """decrypt_handshake_resp + split(true): (send key, receive key) of the initiator, or None when the
    response's empty field does not open."""
    epk_r = resp[12:44]
    hs = HS(hs.chain, hs.hash)
    hs.mix_chain(epk_r)
    hs.mix_hash(epk_r)
    hs.mix_chain(x25519(esk_i, epk_r))
    hs.mix_chain(x25519(sk_i, epk_r))
    k = hs.mix_key_and_hash(psk)
    if open_(k, hs.hash, resp[44:60]) is None:
        return None
    return hs.split()


# ------------------------------------------------------------ responder side
ZERO_ROW = bytes(108) + PEER_NONE.to_bytes(4, "little") + bytes(16)  # a failure's row: zeros, peer = RG_PEER_NONE


def result_row(chain, hash_, ephemeral, ts, peer: int, sender: bytes) -> bytes:
    """rg_hs_init_result: chain, hash, ephemeral, timestamp[12], peer, sender, pad[12]."""
    row = chain + hash_ + ephemeral + ts + peer.to_bytes(4, "little") + sender + bytes(12)
    assert len(row) == 128
    return row


def consume_initiation(msg: bytes, sk_r: bytes, peer_keys: list):
    """decrypt_handshake_init + Config::get_peer_idx on a 148-byte message whose type word is 1:
    (status, result row).  peer_keys: the peers' static public keys in row order."""
    pk_r = pubkey(sk_r)
    epk = msg[8:40]
    hs = HS()
    hs.mix_hash(pk_r)
    hs.mix_hash(epk)
    hs.mix_chain(epk)
    dh = x25519(sk_r, epk)
    if dh == bytes(32):
        return KEYEXCHANGE, ZERO_ROW
    k = hs.mix_key(dh)
    aad = hs.hash
    hs.mix_hash(msg[40:88])
    spk = open_(k, aad, msg[40:88])
    if spk is None:
        return DECRYPT_ERR, ZERO_ROW
    dh = x25519(sk_r, spk)
    if dh == bytes(32):
        return KEYEXCHANGE, ZERO_ROW
    k = hs.mix_key(dh)
    aad = hs.hash
    hs.mix_hash(msg[88:116])
    ts = open_(k, aad, msg[88:116])
    if ts is None:
        return DECRYPT_ERR, ZERO_ROW
    if spk not in peer_keys:
        return REJECTED, ZERO_ROW
    return OK, result_row(hs.chain, hs.hash, epk, ts, peer_keys.index(spk), msg[4:8])


def build_response(row: bytes, peers: list, esk_r: bytes, session_id: int, cookie: bytes | None):
    """encrypt_handshake_resp + split(false) from a result row: (status, the 92 bytes, send key || receive
    key).  peers: (public key, preshared key, mac1 key) rows.  A failure gives zero rows."""
    peer = int.from_bytes(row[108:112], "little")
    if peer >= len(peers):
        return INVALID, bytes(92), bytes(64)
    pk_i, psk, m1k = peers[peer]
    hs = HS(row[0:32], row[32:64])
    epk_r = pubkey(esk_r)
    hs.mix_chain(epk_r)
    hs.mix_hash(epk_r)
    for point in (row[64:96], pk_i):  # ee, se
        dh = x25519(esk_r, point)
        if dh == bytes(32):
            return KEYEXCHANGE, bytes(92), bytes(64)
        hs.mix_chain(dh)
    k = hs.mix_key_and_hash(psk)
    empty = seal(k, hs.hash, b"")
    hs.mix_hash(empty)
    msg = (2).to_bytes(4, "little") + session_id.to_bytes(4, "little") + row[112:116] + epk_r + empty
    msg += mac(m1k, msg)
    msg += mac(cookie, msg) if cookie is not None else bytes(16)
    assert len(msg) == 92
    k1, k2 = hs.split()
    return OK, msg, k2 + k1


# -------------------------------------------------------------- case builders
def peer_rows(peers: list) -> np.ndarray:
    """rg_hs_peer rows (96 bytes) of (public key, preshared key, mac1 key) tuples."""
    return np.frombuffer(b"".join(a + b + c for a, b, c in peers), np.uint8).reshape(len(peers), 96).copy()


def tai64n(sec: int, nano: int) -> bytes:
    return ((1 << 62) + sec).to_bytes(8, "big") + nano.to_bytes(4, "big")


INIT_KINDS = ["valid", "unknown_static", "static_ct_flipped", "ts_tag_flipped", "ts_tag_flipped_unknown", "eph_zero",
              "eph_one", "static_low_order", "type2", "len92", "offset8", "past_buf", "gated", "key_skip"]


class Responder:
    """A responder with npeers known peers, a pool of unknown initiators and neph initiator ephemerals,
    all drawn from one seeded generator."""

    def __init__(self, seed: int, npeers: int = 5, neph: int = 8, nunknown: int = 2):
        rng = np.random.default_rng(seed)
        rb = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
        self.rng = rng
        self.sk_r = rb(32)
        self.pk_r = pubkey(self.sk_r)
        self.sk_i = [rb(32) for _ in range(npeers)]
        self.peers = [(pubkey(sk), rb(32), mac1_key(pubkey(sk))) for sk in self.sk_i]
        self.peer_keys = [p[0] for p in self.peers]
        self.sk_unknown = [rb(32) for _ in range(nunknown)]
        self.esk_i = [rb(32) for _ in range(neph)]
        self.own = np.frombuffer(self.sk_r + self.pk_r, np.uint8).copy()

    def message(self, kind: str, i: int):
        """One message of the given kind: (bytes, len for the descriptor).  i picks the peer, the ephemeral
        and the timestamp."""
        rng = self.rng
        sk = self.sk_i[i % len(self.sk_i)]
        esk = self.esk_i[i % len(self.esk_i)]
        ts = tai64n(1_700_000_000 + i, 1000 * i)
        static = None
        if kind in ("unknown_static", "ts_tag_flipped_unknown"):
            sk = self.sk_unknown[i % len(self.sk_unknown)]
        if kind == "static_low_order":
            static = [le(0), le(1), ORDER8_A, ORDER8_B, le(P - 1), le(P), le(P + 1)][i % 7]
        msg = bytearray(make_initiation(sk, self.pk_r, esk, ts, int(rng.integers(0, 2**32)), static)[0])
        if kind == "static_ct_flipped":
            msg[40 + int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
        elif kind in ("ts_tag_flipped", "ts_tag_flipped_unknown"):
            msg[100 + int(rng.integers(0, 16))] ^= 1 << int(rng.integers(0, 8))
        elif kind == "eph_zero":
            msg[8:40] = le(0)
        elif kind == "eph_one":
            msg[8:40] = le(1)
        elif kind == "type2":
            msg[0:4] = (2).to_bytes(4, "little")
        return bytes(msg), (92 if kind == "len92" else 148)

    def expect(self, kind: str, msg: bytes):
        """(status, result row) by the table of include/rg_aead.h."""
        if kind == "offset8":
            return UNALIGNED, ZERO_ROW
        if kind in ("len92", "past_buf", "type2"):
            return INVALID, ZERO_ROW
        if kind in ("gated", "key_skip"):
            return REJECTED, ZERO_ROW
        return consume_initiation(msg, self.sk_r, self.peer_keys)


def init_batch(resp: Responder, kinds: list, desc_dtype):
    """The frames of one rg_handshake_init_batch_dev call: messages of the given kinds laid out with 0 / 16 /
    32-byte gaps (the `past_buf` frames last: their descriptors point across the end of the buffer).
    Returns (desc, gate, buf, msgs, want_status, want_rows)."""
    n = len(kinds)
    rng = resp.rng
    made = [resp.message(k, i) for i, k in enumerate(kinds)]
    gaps = rng.integers(0, 3, n) * 16
    off = np.zeros(n, np.uint64)
    pos = 0
    for i in range(n):
        off[i] = pos
        pos += 160 + int(gaps[i])
    buf = rng.integers(0, 256, pos, dtype=np.uint8)
    desc = np.zeros(n, desc_dtype)
    gate = np.zeros(n, np.uint8)
    for i, (k, (msg, ln)) in enumerate(zip(kinds, made)):
        buf[int(off[i]):int(off[i]) + 148] = np.frombuffer(msg, np.uint8)
        o = int(off[i])
        if k == "offset8":
            o += 8
        elif k == "past_buf":
            o = (pos - 147 + 15) // 16 * 16  # the last 16-byte boundary from which 148 bytes overrun the buffer
        desc[i] = (o, ln, KEY_SKIP if k == "key_skip" else int(rng.integers(0, 1000)))
        if k == "gated":
            gate[i] = [REJECTED, 7, INVALID, 6][i % 4]
    want = [resp.expect(k, m[0]) for k, m in zip(kinds, made)]
    status = np.array([w[0] for w in want], np.uint8)
    rows = np.frombuffer(b"".join(w[1] for w in want), np.uint8).reshape(n, 128)
    return desc, gate, buf, [m[0] for m in made], status, rows
