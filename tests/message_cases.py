"""The per-message drop-in's shapes, shared by test_message_cpu.py, test_gpu_message.py and the
`message` leg of tests/golden/make_golden.py.

The general kernel (rustyguard_amd/csrc/rg_kernels.hip) gives lane c of its one wave the 64-byte chunks
c, c + 64, ... of the text, so a lane's second trip needs a text of more than 64 * 64 = 4096 bytes; lane 0
runs Poly1305 over the AAD and the text in groups of eight 16-byte blocks (128 bytes) with a masked tail.
The lengths below are the smallest at which each of those loops changes its trip count or its tail.

Every input is derived from a label with SHAKE-256, so the same bytes come out on every machine; a shape
is written (aad_len, text_len) throughout."""
import functools
import hashlib

KINDS = ("msg", "xmsg")  # ChaCha20-Poly1305 (12-byte nonce), XChaCha20-Poly1305 (24-byte nonce)
NONCE_LEN = {"msg": 12, "xmsg": 24}
ROUND = 64 * 64  # bytes of text one round of the 64 lanes covers

TEXT_LENS = [
    0, 1, 15, 16, 17, 63, 64, 65,  # block and chunk edges
    127, 128, 129,  # one eight-block Poly1305 group
    4032, 4095, 4096, 4097, 4111, 4112, 4160, 4161,  # first lane round full / second begun, tail in lane 0's second chunk
    8191, 8192, 8193,  # third round
    12289,
    65536 + 17,  # every lane in its 17th round, ragged tail
]
AAD_LENS = [0, 1, 15, 16, 17, 32, 127, 128, 129, 145, 4097]
CORNER = (4097, 65536 + 17)


def _shapes():
    out = [(a, t) for t in TEXT_LENS for a in (0, 32)]
    out += [(a, t) for a in AAD_LENS for t in (0, 17, 4097)]
    out.append(CORNER)
    return sorted(set(out), key=lambda s: (s[1], s[0]))  # by text length, so a report names the first round that fails


SHAPES = [(kind, a, t) for kind in KINDS for (a, t) in _shapes()]


def bytes_for(label: str, n: int) -> bytes:
    return hashlib.shake_256(label.encode()).digest(n)


# nonces with every bit set: the 12-byte one fills state words 13..15, the 24-byte one the HChaCha20 input
# and the inner nonce's two words; both at shape (32, 4097)
NONCES = [("msg", b"\xff" * 12, 32, 4097), ("xmsg", b"\xff" * 24, 32, 4097)]


@functools.lru_cache(maxsize=None)
def inputs(kind: str, aad_len: int, text_len: int, nonce: bytes = None):
    """(key, nonce, aad, plaintext) of one case; `nonce` replaces the derived one (NONCES)"""
    tag = f"rustyguard-amd per-message {kind} {aad_len} {text_len} "
    if nonce is None:
        nonce = bytes_for(tag + "nonce", NONCE_LEN[kind])
    assert len(nonce) == NONCE_LEN[kind]
    return bytes_for(tag + "key", 32), nonce, bytes_for(tag + "aad", aad_len), bytes_for(tag + "text", text_len)


def case_id(kind: str, aad_len: int, text_len: int) -> str:
    return f"{kind}-aad{aad_len}-text{text_len}"


def first_diff(a: bytes, b: bytes):
    """offset of the first differing byte (the shorter length if one is a prefix of the other), None if equal;
    offset // 4096 is the lane round that wrote it, (offset // 64) % 64 the lane"""
    if a == b:
        return None
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


def flipped(b: bytes, at: int, bit: int = 0x01) -> bytes:
    out = bytearray(b)
    out[at] ^= bit
    return bytes(out)


# One context's call sequence (test_call_sequences_reuse_the_arena; the sanitizer driver runs the same
# lengths): (kind, what, aad_len, text_len).  "seal": seal and compare; "seal_open": seal, compare, open
# the result back; "open": open an oracle-sealed message; "forged_open": open one with a flipped tag bit.
SEQUENCES = [
    ("msg", "seal", 145, 12289),  # long first: the call that allocates the arena
    ("msg", "seal", 1, 1),  # the longer call's bytes lie behind this one's padding
    ("msg", "seal_open", 0, 0),
    ("msg", "seal", 4097, 17),  # the payload offset moves far out
    ("msg", "open", 0, 4097),  # and back to zero
    ("msg", "seal", 16, 65536 + 17),  # regrows the used arena
    ("xmsg", "seal_open", 15, 15),
    ("msg", "forged_open", 32, 4097),
    ("msg", "open", 32, 4097),  # a failed open disturbs nothing that follows
]

# four threads on one context: each its own interleaving of ten shapes from both sides of one lane round
THREAD_PLANS = [
    [("msg", 32, 4097), ("msg", 0, 1), ("xmsg", 17, 17), ("msg", 0, 8193), ("msg", 129, 0), ("xmsg", 0, 4096),
     ("msg", 32, 63), ("msg", 145, 4097), ("xmsg", 32, 4161), ("msg", 0, 16)],
    [("xmsg", 0, 15), ("msg", 0, 12289), ("msg", 16, 17), ("xmsg", 32, 4097), ("msg", 0, 64), ("msg", 4097, 17),
     ("msg", 32, 8192), ("xmsg", 1, 0), ("msg", 0, 4112), ("msg", 32, 129)],
    [("msg", 0, 4160), ("msg", 127, 17), ("xmsg", 0, 8191), ("msg", 32, 0), ("msg", 0, 4095), ("xmsg", 128, 4097),
     ("msg", 0, 65), ("msg", 32, 12289), ("xmsg", 15, 17), ("msg", 0, 4111)],
    [("xmsg", 32, 1), ("msg", 0, 4097), ("msg", 17, 0), ("xmsg", 0, 4032), ("msg", 32, 128), ("msg", 0, 8192),
     ("xmsg", 145, 17), ("msg", 32, 4096), ("msg", 0, 127), ("xmsg", 32, 8193)],
]
