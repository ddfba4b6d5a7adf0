"""The reference side of the per-message drop-in's long shapes (tests/message_cases.py), with no GPU: the
fixture tests/golden/per_message_long.json regenerates identically from OpenSSL, the C oracle reproduces every
entry, opens every message back and refuses a flip of the last AAD byte, the last ciphertext byte and tag
bytes 0 and 15; and the shape table still holds the lengths it exists for (texts past one, two and sixteen
rounds of the general kernel's lanes, AADs past one and many Poly1305 groups)."""
import hashlib
import sys

import pytest

import message_cases as mc
from conftest import GOLDEN, load_golden
from oracle import openssl_ref, oracle

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

FIX = load_golden("per_message_long.json")
BY_SHAPE = {(e["kind"], e["aad_len"], e["text_len"]): e for e in FIX["shapes"]}
SEAL = {"msg": oracle.aead_seal, "xmsg": oracle.xaead_seal}
OPEN = {"msg": oracle.aead_open, "xmsg": oracle.xaead_open}


def test_shape_table_keeps_its_edges():
    assert len(mc.SHAPES) == 152 and len(set(mc.SHAPES)) == 152
    assert [(e["kind"], e["aad_len"], e["text_len"]) for e in FIX["shapes"]] == mc.SHAPES
    for kind in mc.KINDS:
        shapes = [(a, t) for k, a, t in mc.SHAPES if k == kind]
        assert len(shapes) == 76
        texts, aads = {t for _, t in shapes}, {a for a, _ in shapes}
        assert texts == set(mc.TEXT_LENS) and aads == set(mc.AAD_LENS)
        for bound in (4096, 8192, 65536):
            assert any(t > bound for t in texts), bound
        for bound in (128, 4096):
            assert any(a > bound for a in aads), bound
        for t in mc.TEXT_LENS:
            assert (0, t) in shapes and (32, t) in shapes, t
        for a in mc.AAD_LENS:
            assert all((a, t) in shapes for t in (0, 17, 4097)), a
        assert mc.CORNER == (4097, 65553) and mc.CORNER in shapes
        # the first lengths at which a changed lane stride, and a changed tail in the AAD's second group, show
        assert (0, 4097) in shapes and (129, 17) in shapes
    assert [(k, len(nz), a, t) for k, nz, a, t in mc.NONCES] == [("msg", 12, 32, 4097), ("xmsg", 24, 32, 4097)]
    assert all(set(nz) == {0xFF} for _, nz, _, _ in mc.NONCES)
    assert [(e["kind"], e["nonce"]) for e in FIX["nonces"]] == [(k, nz.hex()) for k, nz, _, _ in mc.NONCES]
    assert [s[1:] for s in mc.SEQUENCES] == [("seal", 145, 12289), ("seal", 1, 1), ("seal_open", 0, 0), ("seal", 4097, 17),
                                             ("open", 0, 4097), ("seal", 16, 65553), ("seal_open", 15, 15),
                                             ("forged_open", 32, 4097), ("open", 32, 4097)]
    assert len(mc.THREAD_PLANS) == 4
    for plan in mc.THREAD_PLANS:
        assert len(plan) == 10 and any(t > 4096 for _, _, t in plan) and any(t <= 4096 for _, _, t in plan)


def test_inputs_are_the_labelled_bytes():
    """the derivation itself is pinned: an edit to the labels would otherwise only show as a fixture mismatch"""
    key, nonce, aad, pt = mc.inputs("msg", 1, 17)
    assert key == hashlib.shake_256(b"rustyguard-amd per-message msg 1 17 key").digest(32)
    assert nonce == hashlib.shake_256(b"rustyguard-amd per-message msg 1 17 nonce").digest(12)
    assert aad == hashlib.shake_256(b"rustyguard-amd per-message msg 1 17 aad").digest(1)
    assert pt == hashlib.shake_256(b"rustyguard-amd per-message msg 1 17 text").digest(17)
    assert len(mc.inputs("xmsg", 0, 0)[1]) == 24
    assert mc.inputs("msg", 32, 4097, b"\xff" * 12)[1] == b"\xff" * 12
    assert mc.inputs("msg", 32, 4097, b"\xff" * 12)[3] == mc.inputs("msg", 32, 4097)[3]


def test_fixture_regenerates_identically():
    if not (oracle.openssl_available() and openssl_ref.available()):
        pytest.skip("libcrypto not present")
    import make_golden

    assert make_golden.per_message_long() == FIX


def test_plain_python_hchacha20_matches_the_draft_and_the_oracle():
    import make_golden

    k = load_golden("xchacha.json")["hchacha20_kat"]
    assert make_golden.hchacha20_py(bytes.fromhex(k["key"]), bytes.fromhex(k["nonce"])).hex() == k["subkey"]
    for kind, a, t in mc.SHAPES[::19]:
        key = mc.inputs(kind, a, t)[0]
        nz = mc.bytes_for(f"hchacha {a} {t}", 16)
        assert make_golden.hchacha20_py(key, nz) == oracle.hchacha20(key, nz)


@pytest.mark.parametrize("kind", mc.KINDS)
def test_oracle_matches_fixture_opens_and_rejects(kind):
    shapes = [s for s in mc.SHAPES if s[0] == kind]
    cases = [(s, mc.inputs(*s)) for s in shapes] + \
            [((k, a, t), mc.inputs(k, a, t, nz)) for k, nz, a, t in mc.NONCES if k == kind]
    entries = [BY_SHAPE[s] for s in shapes] + [e for e in FIX["nonces"] if e["kind"] == kind]
    assert len(cases) == len(entries) == 77
    for (shape, (key, nonce, aad, pt)), e in zip(cases, entries):
        label = mc.case_id(*shape)
        assert (e["aad_len"], e["text_len"]) == (len(aad), len(pt)) == shape[1:], label
        ct, tag = SEAL[kind](key, nonce, aad, pt)
        assert len(ct) == len(pt) and tag.hex() == e["tag"], label
        assert hashlib.sha256(ct).hexdigest() == e["ct_sha256"], label
        assert OPEN[kind](key, nonce, aad, ct, tag) == pt, label
        if aad:
            assert OPEN[kind](key, nonce, mc.flipped(aad, -1), ct, tag) is None, label
        if ct:
            assert OPEN[kind](key, nonce, aad, mc.flipped(ct, -1, 0x80), tag) is None, label
        assert OPEN[kind](key, nonce, aad, ct, mc.flipped(tag, 0)) is None, label
        assert OPEN[kind](key, nonce, aad, ct, mc.flipped(tag, 15, 0x80)) is None, label
