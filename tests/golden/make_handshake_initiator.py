#!/usr/bin/env python3
"""Regenerate tests/golden/handshake_initiator.json: the inputs of the reference's recorded initiation.

TEST INFRASTRUCTURE ONLY (run in the build container; the output is committed).

Builds on make_handshake.py (the rand 0.9 StdRng restatement and the .snap parser) and on the initiator model
of tests/initiator_cases.py.  The reference's test `snapshot` (StdRng seed 1, rustyguard-core/src/lib.rs:
846-925) records the 148-byte initiation of its first peer; what the snapshot does not show is the initiator's
ephemeral private key, which comes out of that peer's own RNG.  That RNG is keyed by eight words of the seed-1
stream (as the responder's is, by words 110-117: make_handshake_full.py), so this script tries every word offset
w: StdRng(key = words[w:w+8]) gives the session id (next_u32) and then the ephemeral key (32 bytes); the offset
at which the id equals initiation[4:8] and the key's public key equals initiation[8:40] is the one.  With it the
model must reproduce the recorded 148 bytes, and the block `snapshot_initiation` is written: the ephemeral key,
the sender, the timestamp, both static keys and the recorded bytes.  When no offset matches the file is written
without that block.

The .snap files are parsed as data; no reference code is used or copied.
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
import initiator_cases as ic  # noqa: E402
from make_handshake import REF, StdRng, snap_bytes  # noqa: E402

STREAM_WORDS = 256  # the seed-1 words searched for the initiator's RNG key
TIMESTAMP = "400000000000000a00000000"


def words(ws) -> bytes:
    return b"".join(w.to_bytes(4, "little") for w in ws)


def snapshot_initiation():
    outer = StdRng(1)
    w = [outer.next_u32() for _ in range(STREAM_WORDS)]
    ssk_i, ssk_r = words(w[0:8]), words(w[8:16])
    init = snap_bytes(f"{REF}/rustyguard-core/src/snapshots/rustyguard_core__tests__snapshot.snap")
    assert len(init) == 148
    sender = int.from_bytes(init[4:8], "little")
    for off in range(STREAM_WORDS - 7):
        inner = StdRng(key=words(w[off:off + 8]))
        if inner.next_u32() != sender:
            continue
        esk_i = inner.fill(32)
        if hc.pubkey(esk_i) != init[8:40]:
            continue
        pk_r = hc.pubkey(ssk_r)
        st, msg, pend = ic.initiate(ssk_i, [(pk_r, bytes(32), hc.mac1_key(pk_r))], 0, esk_i, bytes.fromhex(TIMESTAMP),
                                    sender)
        assert st == ic.OK and msg[:148] == init, "the model's initiation is not the recorded one"
        return {"source": "rustyguard-core/src/lib.rs:846-925 (test `snapshot`, StdRng seed 1) -> "
                          "rustyguard-core/src/snapshots/rustyguard_core__tests__snapshot.snap",
                "rng_key_word_offset": off, "static_private_i": ssk_i.hex(), "static_private_r": ssk_r.hex(),
                "esk_i": esk_i.hex(), "sender": sender, "timestamp": TIMESTAMP, "initiation": init.hex(),
                "pending_row": pend.hex()}
    return None


def main():
    out = {"generator": "tests/golden/make_handshake_initiator.py (the model of tests/initiator_cases.py; checked "
                        "against the reference's .snap files)"}
    block = snapshot_initiation()
    if block is None:
        out["note"] = (f"no word offset below {STREAM_WORDS} of the seed-1 stream keys an RNG that gives the recorded "
                       "sender and ephemeral key: no snapshot_initiation block")
    else:
        out["snapshot_initiation"] = block
    with open(os.path.join(HERE, "handshake_initiator.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote handshake_initiator.json", "with" if block else "WITHOUT", "the snapshot_initiation block")


if __name__ == "__main__":
    main()
