"""CPU-only checks of the device-resident peer handshake state: the public struct's layout, the exported symbols,
the workspace function, and the model's two formulations of the timestamp check against each other (the loop the
reference runs and the prefix maximum the device computes)."""
import os
import subprocess
import textwrap

import numpy as np
import pytest

import peerstate_cases as pc
from conftest import REPO
from rustyguard_amd import _lib, aead

HEADER_DIR = os.path.join(REPO, "include")
NEW = ["rg_peer_ts_workspace_size", "rg_peer_ts_batch_dev", "rg_peer_cookie_consume_batch_dev",
       "rg_peer_cookies_batch_dev", "rg_peer_mac1_batch_dev"]


def test_peer_state_layout_with_gcc(tmp_path):
    src = tmp_path / "peerstate_layout.c"
    src.write_text(textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "rg_aead.h"
        int main(void) {
            printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(rg_hs_peer_state), offsetof(rg_hs_peer_state, latest_ts),
                   offsetof(rg_hs_peer_state, has_cookie), offsetof(rg_hs_peer_state, cookie),
                   offsetof(rg_hs_peer_state, last_sent_mac1), offsetof(rg_hs_peer_state, pad), RG_ABI_VERSION);
            return 0;
        }
    """))
    exe = tmp_path / "peerstate_layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", HEADER_DIR, str(src), "-o", str(exe)], check=True)
    vals = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert vals == [64, 0, 12, 16, 32, 48, 6]
    assert aead.PEER_STATE_BYTES == 64 and len(pc.state_row()) == 64
    row = pc.state_row(bytes(range(12)), cookie=bytes(range(16, 32)), mac1=bytes(range(32, 48)))
    assert row[12:16] == b"\x01\0\0\0" and row[16:32] == bytes(range(16, 32)) and row[32:48] == bytes(range(32, 48))


def test_both_libraries_export_the_symbols():
    from rustyguard_amd import build

    build.build()
    assert "rg_peerstate.hip" in build.KERNELS and "rg_peerstate.hip" not in build.HOST
    for lib in (build.LIB, build.TEST_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert f" T {name}\n" in out, (lib, name)
    assert set(NEW) <= set(_lib.SIGNATURES)


def test_host_units_name_no_peerstate_launcher():
    """the host units are also linked against a fixed CPU stand-in of the launchers: the new entry points live
    beside their kernels and the host units do not know them"""
    from rustyguard_amd import build

    for unit in build.HOST:
        text = open(os.path.join(build.CSRC, unit)).read()
        assert "rg_peer_ts" not in text and "rg_peer_cookie" not in text and "rg_peer_mac1" not in text, unit


def test_ts_workspace_size_is_monotone_and_refuses_absurd_batches():
    L = _lib.lib()
    size = lambda n, p: int(L.rg_peer_ts_workspace_size(n, p))  # noqa: E731
    ns = [0, 1, 255, 256, 2047, 2048, 2049, 4096 + 77, 65536, 1 << 20, (1 << 32) - 1]
    ps = [0, 1, 2, 256, 257, 65536, 65537, 1 << 24, (1 << 24) + 1, 0xFFFFFFFF]
    for p in ps:
        col = [size(n, p) for n in ns]
        assert all(a <= b for a, b in zip(col, col[1:])) and col[0] >= 256, (p, col)
    for n in ns:
        row = [size(n, p) for p in ps]
        assert all(a <= b for a, b in zip(row, row[1:])), (n, row)
    assert all(size(n, p) % 256 == 0 for n in ns for p in ps)
    assert size(1 << 32, 4) == 0 and size((1 << 63) + 5, 1) == 0
    # the rows array, the 16-byte running maximum per row and one 16-byte aggregate per tile at the least
    assert size(2049, 1) >= 2049 * 4 + 2049 * 16 + 2 * 16


@pytest.mark.parametrize("name", [e[0] for e in pc.EDGE_TS])
def test_ts_edge_cases_in_both_formulations(name):
    state, results, status, want = pc.edge_ts_case(name)
    loop = pc.ts_loop(state, results, status)
    assert loop[2] == want
    assert pc.ts_by_max(state, results, status) == loop
    for i, s in enumerate(loop[2]):
        assert (loop[1][i] == pc.ZERO_RESULT) == (s != pc.OK)
        assert loop[3][i] == (int.from_bytes(results[i][108:112], "little") if s == pc.OK else pc.PEER_NONE)
    assert loop[0][0][12:] == state[0][12:] and loop[0][1] == state[1]  # the other fields stay


def test_ts_loop_equals_prefix_maximum_on_random_batches():
    rng = np.random.default_rng(20261020)
    rejected = accepted = ties = 0
    for trial in range(60):
        npeers = int(rng.integers(1, 6))
        n = int(rng.integers(1, 120))
        results, status = pc.random_ts_batch(rng, n, npeers, nts=int(rng.integers(1, 6)))
        tss = [bytes(rng.integers(0, 256, 12, dtype=np.uint8)), bytes(12), results[0][96:108]]
        state = [pc.state_row(tss[int(rng.integers(0, 3))], mac1=bytes([p]) * 16) for p in range(npeers)]
        loop = pc.ts_loop(state, results, status)
        assert pc.ts_by_max(state, results, status) == loop, trial
        rejected += sum(1 for a, b in zip(status, loop[2]) if a == pc.OK and b == pc.REJECTED)
        accepted += sum(1 for b in loop[2] if b == pc.OK)
        seen = set()
        for r, s in zip(results, status):
            if s == pc.OK:
                ties += (r[96:112] in seen)
                seen.add(r[96:112])
    assert rejected > 100 and accepted > 100 and ties > 100  # the batches exercise both verdicts and ties


def test_consume_gather_record_models():
    """the last valid cookie of a peer stays, a forged message behind it changes nothing; gather and record"""
    rng = np.random.default_rng(5)
    rb = lambda k: bytes(rng.integers(0, 256, k, dtype=np.uint8))  # noqa: E731
    keys = [pc.cookie_key(rb(32)) for _ in range(2)]
    state = [pc.state_row(mac1=rb(16)), pc.state_row(mac1=rb(16), cookie=rb(16))]
    table = {100: 0, 101: 1, 102: 7}
    c1, c2 = rb(16), rb(16)
    good1 = pc.cookie_message(100, rb(24), keys[0], state[0][32:48], c1)
    good2 = pc.cookie_message(100, rb(24), keys[0], state[0][32:48], c2)
    forged = bytearray(good2)
    forged[50] ^= 4
    stale = pc.cookie_message(101, rb(24), keys[1], rb(16), rb(16))
    far = pc.cookie_message(102, rb(24), keys[1], state[1][32:48], rb(16))
    msgs = [good1, good2, bytes(forged), stale, far, good1]
    after, st, out = pc.consume_loop(state, keys, table, msgs, [{}] * 5 + [dict(gated=True)])
    assert st == [pc.OK, pc.OK, pc.DECRYPT_ERR, pc.DECRYPT_ERR, pc.INVALID, pc.REJECTED]
    assert out == [c1, c2] + [bytes(16)] * 4
    assert after[0] == pc.state_row(mac1=state[0][32:48], cookie=c2) and after[1] == state[1]
    assert pc.gather(after, [0, 1, 2, pc.PEER_NONE, 0]) == ([c2, state[1][16:32], bytes(16), bytes(16), c2], [1, 1, 0, 0, 1])
    assert pc.gather(state, [0]) == ([bytes(16)], [0])
    sent = [rb(160) for _ in range(4)]
    rec = pc.record_loop(after, [0, 1, 0, 5], [pc.OK, pc.REJECTED, pc.OK, pc.OK], sent, 116)
    assert rec[0][32:48] == sent[2][116:132] and rec[1] == after[1] and rec[0][:32] == after[0][:32]
