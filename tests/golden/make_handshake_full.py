#!/usr/bin/env python3
"""Regenerate tests/golden/handshake_full.json: the inputs and expected bytes of the batched IKpsk2 responder.

TEST INFRASTRUCTURE ONLY (run in the build container; the output is committed).

Builds on make_handshake.py (the rand 0.9 StdRng restatement and the .snap parser) and on the model of
tests/handshake_cases.py.  It records

  * the RFC 7748 vectors the X25519 tests use (§5.2 vectors 1 and 2, the iterated test after 1 and 1000
    steps, §6.1 Alice's key pair), each first reproduced by the model;
  * for the reference's test `snapshot` (StdRng seed 1, rustyguard-core/src/lib.rs:846-925): both static
    private keys, the preshared key (words 16-23 of the seed-1 stream), the responder's session id and
    ephemeral private key (its inner RNG is ChaCha12 keyed by words 110-117), the recorded 148-byte
    initiation and 92-byte response, the decrypted timestamp and both transport keys;
  * for test `handshake` (seed 3, rustyguard-crypto/src/lib.rs:494-537): the five secrets, the resp.empty
    tag and the transport keys K1 / K2.

Every value is asserted against the reference's .snap files (parsed as data) or SURVEY.md Appendix A before
anything is written: the model's response to the recorded initiation must be the recorded response, byte for
byte.  No reference code is used or copied.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

import handshake_cases as hc  # noqa: E402
from make_handshake import REF, StdRng, snap_bytes  # noqa: E402

RFC_VECTORS = [
    ("rfc7748 5.2 vector 1", "a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4",
     "e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c",
     "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552"),
    ("rfc7748 5.2 vector 2", "4b66e9d4d1b4673c5ad22691957d6af5c11b6421e0ea01d42ca4169e7918ba0d",
     "e5210f12786811d3f4b7959d0538ae2c31dbe7106fc03c3efc4cd549c715a493",
     "95cbde9476e8907d7aade45cb4b873f88b595a68799fa152e6f8f7647aac7957"),
    ("rfc7748 6.1 Alice's public key", "77076d0a7318a57d3c16c17251b26645df4c2f87ebc0992ab177fba51db92c2a",
     hc.BASE.hex(), "8520f0098930a754748b7ddcb43ef75a0dbf3a0d26381af4eba4a98eaa9b4e6a"),
]
ITER_1 = "422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079"
ITER_1000 = "684cf59ba83309552800ef566f2f4d3c1c3887c49360e3875f2eb94d99532c51"


def rfc7748() -> dict:
    for name, k, u, out in RFC_VECTORS:
        assert hc.x25519(bytes.fromhex(k), bytes.fromhex(u)).hex() == out, name
    assert hc.rfc_iteration(1)[1].hex() == ITER_1
    assert hc.rfc_iteration(1000)[1].hex() == ITER_1000
    return {"vectors": [{"name": n, "scalar": k, "u": u, "out": o} for n, k, u, o in RFC_VECTORS],
            "iter_1": ITER_1, "iter_1000": ITER_1000}


def words(ws) -> bytes:
    return b"".join(w.to_bytes(4, "little") for w in ws)


def snapshot() -> dict:
    outer = StdRng(1)
    w = [outer.next_u32() for _ in range(128)]
    ssk_i, ssk_r, psk = words(w[0:8]), words(w[8:16]), words(w[16:24])
    inner = StdRng(key=words(w[110:118]))
    session_id = inner.next_u32()
    esk_r = inner.fill(32)
    snaps = f"{REF}/rustyguard-core/src/snapshots/rustyguard_core__tests__"
    init, resp = snap_bytes(snaps + "snapshot.snap"), snap_bytes(snaps + "snapshot-2.snap")
    assert len(init) == 148 and len(resp) == 92
    assert session_id == 0x630DC0F5 and resp[4:8] == session_id.to_bytes(4, "little")
    pk_i = hc.pubkey(ssk_i)
    st, row = hc.consume_initiation(init, ssk_r, [pk_i])
    assert st == hc.OK
    ts = row[96:108]
    assert ts.hex() == "400000000000000a00000000"
    st, got, keys = hc.build_response(row, [(pk_i, psk, hc.mac1_key(pk_i))], esk_r, session_id, None)
    assert st == hc.OK and got == resp, "the model's response is not the recorded one"
    send, recv = keys[:32], keys[32:]
    # the key under the reference's recorded data packet (initiator -> responder)
    assert recv.hex() == "5c1ba0299237c9d32ff307464bebce9e055f1fb481cf6a05ce83ee11590ec95b"
    return {"source": "rustyguard-core/src/lib.rs:846-925 (test `snapshot`, StdRng seed 1) -> "
                      "rustyguard-core/src/snapshots/rustyguard_core__tests__snapshot{,-2}.snap",
            "static_private_i": ssk_i.hex(), "static_private_r": ssk_r.hex(), "preshared_key": psk.hex(),
            "esk_r": esk_r.hex(), "session_id": session_id, "initiation": init.hex(), "response": resp.hex(),
            "timestamp": ts.hex(), "result_row": row.hex(), "send_key": send.hex(), "recv_key": recv.hex()}


def handshake() -> dict:
    rng = StdRng(3)
    sk_i, sk_r, psk = rng.fill(32), rng.fill(32), rng.fill(32)
    rng.fill(32)  # CookieState::new
    esk_i = rng.fill(32)
    ts = (1).to_bytes(8, "big") + (2).to_bytes(4, "big")
    msg, hs_i = hc.make_initiation(sk_i, hc.pubkey(sk_r), esk_i, ts, 0)
    esk_r = rng.fill(32)
    pk_i = hc.pubkey(sk_i)
    st, row = hc.consume_initiation(msg, sk_r, [pk_i])
    assert st == hc.OK and row[96:108] == ts
    st, resp, keys = hc.build_response(row, [(pk_i, psk, hc.mac1_key(pk_i))], esk_r, 0, None)
    assert st == hc.OK
    snaps = f"{REF}/rustyguard-crypto/src/snapshots/rustyguard_crypto__tests__"
    assert resp[44:60] == snap_bytes(snaps + "handshake-3.snap"), "resp.empty"
    k1, k2 = keys[32:], keys[:32]
    assert k1.hex() == "955d913caa335dd622bf01f5fc41a2912a6251f2a2175c3a5d31eeb04ab1128c", "K1"
    assert k2.hex() == "d8e75b244748b792f7d878519a61f4183cfac9718005dbc7ea69522873db9146", "K2"
    assert hc.finish_initiator(resp, hs_i, sk_i, esk_i, psk) == (k1, k2)
    return {"source": "rustyguard-crypto/src/lib.rs:494-537 (test `handshake`, StdRng seed 3) -> "
                      "rustyguard-crypto/src/snapshots/rustyguard_crypto__tests__handshake-3.snap",
            "static_private_i": sk_i.hex(), "static_private_r": sk_r.hex(), "preshared_key": psk.hex(),
            "esk_i": esk_i.hex(), "esk_r": esk_r.hex(), "timestamp": ts.hex(), "empty_tag": resp[44:60].hex(),
            "transport_k1": k1.hex(), "transport_k2": k2.hex()}


def main():
    out = {"generator": "tests/golden/make_handshake_full.py (the model of tests/handshake_cases.py; every value "
                        "checked against the reference's .snap files)",
           "rfc7748": rfc7748(), "snapshot": snapshot(), "handshake": handshake()}
    with open(os.path.join(HERE, "handshake_full.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote handshake_full.json")


if __name__ == "__main__":
    main()
