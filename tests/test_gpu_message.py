"""The per-message drop-in (rg_chacha20poly1305_{enc,dec}, rg_xchacha20poly1305_{enc,dec} -> general_one ->
general_kernel) where its loops run more than once: texts past one, two and sixteen rounds of the kernel's 64
lanes, AADs past one and many eight-block Poly1305 groups, tails 1, 15 and 17 bytes past a block at the end
of long inputs (tests/message_cases.py).  Everything is byte-exact against the C oracle and against
tests/golden/per_message_long.json (OpenSSL EVP); test_message_cpu.py holds the reference side."""
import hashlib
import threading

import pytest

import message_cases as mc
from conftest import load_golden
from oracle import oracle
from rustyguard_amd import aead

pytestmark = pytest.mark.gpu

SEAL = {"msg": oracle.aead_seal, "xmsg": oracle.xaead_seal}


def _enc(engine, kind):
    return engine.chacha20poly1305_enc if kind == "msg" else engine.xchacha20poly1305_enc


def _dec(engine, kind):
    return engine.chacha20poly1305_dec if kind == "msg" else engine.xchacha20poly1305_dec


@pytest.fixture(scope="module")
def fixture_entries():
    g = load_golden("per_message_long.json")
    return {(e["kind"], e["aad_len"], e["text_len"]): e for e in g["shapes"]}, g["nonces"]


@pytest.fixture(scope="module")
def sealed():
    """the oracle's (ciphertext, tag) of every shape, computed once and never changed (bytes)"""
    return {s: SEAL[s[0]](*mc.inputs(*s)) for s in mc.SHAPES}


def _check_seal(engine, kind, ins, want_ct, want_tag, label):
    key, nonce, aad, pt = ins
    buf = bytearray(pt)
    tag = _enc(engine, kind)(key, nonce, aad, buf)
    at = mc.first_diff(bytes(buf), want_ct)
    assert at is None, f"{label}: ciphertext differs first at byte {at} (lane round {at // mc.ROUND}, lane {at // 64 % 64})"
    assert tag == want_tag, f"{label}: tag {tag.hex()}, want {want_tag.hex()}"
    return tag


def _check_open(engine, kind, ins, ct, tag, label):
    key, nonce, aad, pt = ins
    buf = bytearray(ct)
    _dec(engine, kind)(key, nonce, aad, buf, tag)
    at = mc.first_diff(bytes(buf), pt)
    assert at is None, f"{label}: opened text differs first at byte {at} (lane round {at // mc.ROUND})"


def _check_refused(engine, kind, ins, ct, tag, label, aad=None):
    key, nonce, good_aad, _ = ins
    buf = bytearray(ct)
    with pytest.raises(aead.DecryptionError):
        _dec(engine, kind)(key, nonce, good_aad if aad is None else aad, buf, tag)
        pytest.fail(f"{label}: a forged message was accepted")
    assert bytes(buf) == ct, f"{label}: a refused open changed the caller's buffer at byte {mc.first_diff(bytes(buf), ct)}"


@pytest.mark.parametrize("kind", mc.KINDS)
def test_seal_matches_fixture_and_oracle(engine, kind, sealed, fixture_entries):
    by_shape, _ = fixture_entries
    shapes = [s for s in mc.SHAPES if s[0] == kind]
    assert len(shapes) == 76
    for s in shapes:
        label = mc.case_id(*s)
        ct, tag = sealed[s]
        _check_seal(engine, kind, mc.inputs(*s), ct, tag, label)
        e = by_shape[s]
        assert tag.hex() == e["tag"] and hashlib.sha256(ct).hexdigest() == e["ct_sha256"], label


@pytest.mark.parametrize("kind", mc.KINDS)
def test_open_restores_and_rejects(engine, kind, sealed):
    for s in (s for s in mc.SHAPES if s[0] == kind):
        label = mc.case_id(*s)
        ins = mc.inputs(*s)
        ct, tag = sealed[s]
        _check_open(engine, kind, ins, ct, tag, label)
        _check_refused(engine, kind, ins, ct, mc.flipped(tag, 0, 0x01), label + " tag byte 0")
        _check_refused(engine, kind, ins, ct, mc.flipped(tag, 15, 0x80), label + " tag byte 15")
        if ct:
            _check_refused(engine, kind, ins, mc.flipped(ct, -1, 0x10), tag, label + " last ciphertext byte")
        if len(ct) > 4096:  # the first byte another lane round wrote
            _check_refused(engine, kind, ins, mc.flipped(ct, 4096, 0x04), tag, label + " ciphertext byte 4096")
        if ins[2]:
            _check_refused(engine, kind, ins, ct, tag, label + " last AAD byte", aad=mc.flipped(ins[2], -1, 0x02))


def test_call_sequences_reuse_the_arena():
    """One fresh context, so that the first (long) call is the one that allocates the arena: a shorter call
    after a longer one must not see the longer one's bytes behind its padding, offsets are those of the call
    at hand, a refused open leaves the next call alone, and the regrow of a used arena is correct."""
    engine = aead.Engine(0)
    try:
        for step, (kind, what, aad_len, text_len) in enumerate(mc.SEQUENCES):
            label = f"step {step + 1} {what} {mc.case_id(kind, aad_len, text_len)}"
            ins = mc.inputs(kind, aad_len, text_len)
            ct, tag = SEAL[kind](*ins)
            if what in ("seal", "seal_open"):
                got = _check_seal(engine, kind, ins, ct, tag, label)
                if what == "seal_open":
                    _check_open(engine, kind, ins, ct, got, label)
            elif what == "open":
                _check_open(engine, kind, ins, ct, tag, label)
            else:
                assert what == "forged_open"
                _check_refused(engine, kind, ins, ct, mc.flipped(tag, 7, 0x20), label)
    finally:
        engine.close()


def test_all_ff_nonces(engine, fixture_entries):
    _, entries = fixture_entries
    assert len(entries) == len(mc.NONCES) == 2
    for (kind, nonce, aad_len, text_len), e in zip(mc.NONCES, entries):
        label = mc.case_id(kind, aad_len, text_len) + " nonce ff.."
        ins = mc.inputs(kind, aad_len, text_len, nonce)
        assert ins[1] == nonce == bytes.fromhex(e["nonce"])
        ct, tag = SEAL[kind](*ins)
        assert tag.hex() == e["tag"] and hashlib.sha256(ct).hexdigest() == e["ct_sha256"], label
        _check_seal(engine, kind, ins, ct, tag, label)
        _check_open(engine, kind, ins, ct, tag, label)
        _check_refused(engine, kind, ins, ct, mc.flipped(tag, 0), label)


def test_four_threads_one_context(engine):
    """Four threads call one context at once (ctypes drops the GIL around each call, so they meet at the
    context's mutex), each with its own interleaving of shapes from both sides of one lane round; every seal,
    open and refusal is the oracle's."""
    want = {s: SEAL[s[0]](*mc.inputs(*s)) for plan in mc.THREAD_PLANS for s in plan}
    errors = []
    start = threading.Barrier(len(mc.THREAD_PLANS))

    def run(t, plan):
        try:
            start.wait(timeout=30)
            for n, s in enumerate(plan):
                label = f"thread {t} call {n} {mc.case_id(*s)}"
                ins = mc.inputs(*s)
                ct, tag = want[s]
                _check_seal(engine, s[0], ins, ct, tag, label)
                if n % 3 == 1:
                    _check_refused(engine, s[0], ins, ct, mc.flipped(tag, 15), label)
                _check_open(engine, s[0], ins, ct, tag, label)
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append(f"thread {t}: {type(e).__name__}: {e}")

    threads = [threading.Thread(target=run, args=(t, plan)) for t, plan in enumerate(mc.THREAD_PLANS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, "\n".join(errors)
