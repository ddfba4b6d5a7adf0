"""Cryptokey routing, the part that needs no GPU: the ABI surface (header, both libraries, ctypes table), the
layout of rg_route_prefix, the route table's builder and host lookup against a brute-force longest-prefix match
(route_cases.brute), their error returns, rg_route_workspace_size, and rustyguard_amd/csrc/rg_route.h alone
under AddressSanitizer and UBSan (tests/route_host/driver.cpp, a stand-alone program)."""
import ctypes
import os
import re
import subprocess
import textwrap

import numpy as np
import pytest

import route_cases as rc
from conftest import REPO
from rustyguard_amd import _lib, build, route

NAMES = ("rg_route_table_words", "rg_route_table_build", "rg_route_lookup", "rg_route_workspace_size",
         "rg_route_batch_dev", "rg_route_check_batch_dev", "rg_send_batch_dev_routed")
CASES = rc.table_cases()
EINVAL, EFULL = -1, -5


def test_header_libraries_and_binding_have_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "rg_aead.h")).read(), flags=re.S)
    build.build()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _lib.SIGNATURES
        for path in (build.LIB, build.TEST_LIB):
            out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
            assert f" T {name}\n" in out, (name, path)
    assert re.search(r"#define\s+RG_ABI_VERSION\s+6\b", text)
    assert len(_lib.SIGNATURES["rg_route_batch_dev"][1]) == 14
    assert len(_lib.SIGNATURES["rg_route_check_batch_dev"][1]) == 13
    assert len(_lib.SIGNATURES["rg_send_batch_dev_routed"][1]) == 21
    assert "rg_route.hip" in build.KERNELS and "rg_route.hip" not in build.HOST


def test_prefix_layout_and_status_value_with_gcc(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "rg_aead.h"
        int main(void) {
            printf("%zu %zu %zu %zu %d %d\\n", sizeof(rg_route_prefix), offsetof(rg_route_prefix, addr),
                   offsetof(rg_route_prefix, prefix_len), offsetof(rg_route_prefix, peer), (int)RG_PKT_UNROUTABLE,
                   RG_ABI_VERSION);
            return 0;
        }
    """))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                   check=True)
    vals = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert vals == [12, 0, 4, 8, 9, 6]
    assert route.PKT_UNROUTABLE == rc.UNROUTABLE == 9 and route.PREFIX_DTYPE.itemsize == 12


def test_cases_cover_what_they_claim():
    """Every prefix length on both sides of each stride boundary, nesting, siblings, duplicates with another
    peer, host bits below the prefix length -- read off the rows, not off the code under test."""
    rows = [r for _, t in CASES for r in t]
    assert {plen for _, plen, _ in rows} >= set(rc.PREFIX_LENGTHS)
    assert any(net & ~rc.mask(plen) & 0xFFFFFFFF for net, plen, _ in rows)  # host bits set
    nested = dict(CASES)["nested"]
    keyed = {}
    for net, plen, peer in nested:
        keyed.setdefault((net & rc.mask(plen), plen), []).append(peer)
    assert sum(len(set(v)) > 1 for v in keyed.values()) >= 3  # the same prefix with two peers
    nets = sorted(keyed)
    assert any(a != b and pb > pa and (b & rc.mask(pa)) == a for a, pa in nets for b, pb in nets)  # nesting
    assert (rc.ip(10, 1, 2, 0), 25) in keyed and (rc.ip(10, 1, 2, 128), 25) in keyed  # siblings
    # the scenario of the packet tests
    for peer, addr in rc.SRC_OF.items():
        assert int(rc.brute(rc.ROWS, [addr])[0]) == peer
    slot = rc.peer_slots()
    for dst in rc.DST_OK:
        p = int(rc.brute(rc.ROWS, [dst])[0])
        assert p < rc.NPEERS and slot[p] != rc.SKIP
    assert all(int(rc.brute(rc.ROWS, [d])[0]) == rc.NO_SESSION for d in rc.DST_NO_SESSION)
    assert all(int(rc.brute(rc.ROWS, [d])[0]) == rc.NONE for d in rc.DST_NONE)
    assert all(rc.NPEERS <= int(rc.brute(rc.ROWS, [d])[0]) < rc.NONE for d in rc.DST_BEYOND)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_table_size_is_exact_and_lookup_is_longest_prefix_match(case):
    name, rows = case
    L = _lib.lib()
    pre = rc.prefix_rows(rows)
    ptr = pre.ctypes.data_as(ctypes.c_void_p) if len(pre) else None
    words = L.rg_route_table_words(ptr, len(pre))
    assert words == rc.expected_words(rows) and words >= 65536
    guard = 0xDEADBEEF
    table = np.full(words + 8, guard, np.uint32)
    assert L.rg_route_table_build(ptr, len(pre), table.ctypes.data_as(ctypes.c_void_p), words) == 0
    assert (table[words:] == guard).all() and not (table[:words] == guard).any()
    short = np.full(words + 8, guard, np.uint32)
    assert L.rg_route_table_build(ptr, len(pre), short.ctypes.data_as(ctypes.c_void_p), words - 1) == EFULL
    assert b"cap_words" in L.rg_last_error() and (short == guard).all()  # nothing written
    again = route.build_table(pre)  # the wrapper; deterministic
    assert again.size == words and np.array_equal(again, table[:words])
    table = np.ascontiguousarray(table[:words])
    addrs = rc.probes(rows)
    want = rc.brute(rows, addrs)
    got = np.array([route.lookup(table, int(a).to_bytes(4, "big")) for a in addrs], np.uint32)
    assert np.array_equal(got, want), [(hex(a), g, w) for a, g, w in zip(addrs, got, want) if g != w][:5]
    if name == "empty":
        assert words == 65536 and (table == rc.NONE).all()
    if name == "default_only":
        assert (got == 7).all()
    if name == "nested":
        assert route.lookup(table, "10.1.2.200") == 12 and route.lookup(table, "10.1.2.77") == 10
        assert route.lookup(table, "10.1.2.130") == 14 and route.lookup(table, "10.200.0.9") == 16
        assert route.lookup(table, "10.200.0.8") == 1 and route.lookup(table, "11.0.0.0") == rc.NONE
        # every peer a probe can reach; 7's /23 lies wholly under its two /24s, as 3, 4, 5 and 11 under later rows
        assert {int(g) for g in got} == {1, 2, 6, 8, 9, 10, 12, 13, 14, 15, 16, 17, 18, 19, rc.NONE}


def test_wrapper_takes_cidr_strings():
    table = route.build_table([("10.0.0.0/8", 1), ("10.1.2.77/24", 3), ("0.0.0.0/0", 9), ("10.1.2.3", 4)])
    assert [route.lookup(table, a) for a in ("10.9.9.9", "10.1.2.200", "8.8.8.8", "10.1.2.3")] == [1, 3, 9, 4]


def test_error_returns():
    L = _lib.lib()
    good = rc.prefix_rows([(rc.ip(10, 0, 0, 0), 8, 1)])
    table = np.zeros(70000, np.uint32)
    tp = table.ctypes.data_as(ctypes.c_void_p)
    for field, value in (("prefix_len", 33), ("peer", 0x80000000), ("peer", 0xFFFFFFFF)):
        bad = rc.prefix_rows([(rc.ip(10, 0, 0, 0), 8, 1), (rc.ip(10, 1, 0, 0), 16, 2)])
        bad[field][1] = value
        bp = bad.ctypes.data_as(ctypes.c_void_p)
        assert L.rg_route_table_words(bp, 2) == 0
        assert L.rg_route_table_build(bp, 2, tp, table.size) == EINVAL
    assert not table.any()
    gp = good.ctypes.data_as(ctypes.c_void_p)
    assert L.rg_route_table_build(gp, 1, None, 70000) == EINVAL  # null table
    assert L.rg_route_table_build(None, 1, tp, 70000) == EINVAL and L.rg_route_table_words(None, 1) == 0  # null rows
    assert L.rg_route_table_build(gp, 1, tp, 65535) == EFULL and L.rg_route_table_build(gp, 1, tp, 0) == EFULL
    assert not table.any()
    assert L.rg_route_table_words(None, 0) == 65536 and L.rg_route_table_build(None, 0, tp, 65536) == 0  # np == 0
    assert (table[:65536] == rc.NONE).all() and not table[65536:].any()
    # the host lookup refuses what it cannot walk
    a = np.array([10, 0, 0, 1], np.uint8)
    ap = a.ctypes.data_as(ctypes.c_void_p)
    assert L.rg_route_lookup(None, 65536, ap) == rc.NONE and L.rg_route_lookup(tp, 65535, ap) == rc.NONE
    assert L.rg_route_lookup(tp, 65536, None) == rc.NONE
    # the device calls refuse a null context before anything else
    assert L.rg_route_batch_dev(None, None, 0, None, 0, None, 1, None, 0, None, None, None, None, None) == EINVAL


def test_workspace_size():
    size = _lib.lib().rg_route_workspace_size
    send = _lib.lib().rg_send_workspace_size
    assert size(1, 1) > 0
    assert size(1 << 32, 1) == 0 and size(1 << 63, 1) == 0  # n > 2^32 - 1 is refused by the calls
    for nkeys in (0, 1, 2, 256, 257, 65536, 65537, 0xFFFFFFFF):
        sizes = [size(n, nkeys) for n in (0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 65536, 1 << 20, (1 << 32) - 1)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (nkeys, sizes)
        assert sizes[1] > 0 and sizes[-1] > 0
    for n in (1, 1000, 1 << 20):
        sizes = [size(n, nkeys) for nkeys in (0, 1, 2, 3, 255, 256, 257, 65536, 65537, 1 << 24, (1 << 24) + 1, 0xFFFFFFFF)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (n, sizes)
    for n, nkeys in ((1, 1), (257, 5), (65536, 256)):  # the route's arrays (16 + 4 + 1 bytes a packet) and the send's
        assert size(n, nkeys) >= send(n, nkeys) + 21 * n


# ---- rg_route.h alone, on the host, under AddressSanitizer and UBSan
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("route") / "driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "rustyguard_amd", "csrc"),
                    "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "route_host", "driver.cpp"),
                    "-o", exe], check=True)

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        return r.stdout.split("\n")[:-1]

    return run


def test_header_alone_under_sanitizers(driver):
    lines, want = [], []
    for _, rows in CASES:
        addrs = rc.probes(rows)
        lines += [f"t {len(rows)}"] + [f"{net:08x} {plen} {peer}" for net, plen, peer in rows]
        lines += [f"p {len(addrs)}"] + [f"{int(a):08x}" for a in addrs]
        want += [f"{rc.expected_words(rows)} 0 1 {EFULL}", " ".join(f"{int(x):x}" for x in rc.brute(rows, addrs))]
    out = driver(lines)
    assert out == want, [(o, w) for o, w in zip(out, want) if o != w][:2]


def test_corrupt_table_never_reads_outside(driver):
    """Pointers to blocks at and past the table's end on every level, in exactly sized heap buffers: every lookup
    is RG_PEER_NONE and the sanitizers saw no read outside the table."""
    out = driver(["c"])
    lookups, bad = map(int, out[0].split())
    assert lookups >= 100 and bad == 0
