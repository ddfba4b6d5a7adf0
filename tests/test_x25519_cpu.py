"""rustyguard_amd/csrc/rg_x25519.h on the host, under AddressSanitizer and UBSan: the field arithmetic and the
ladder that rg_handshake.hip runs per lane are the same source, so their carry edges are checked here, on a
CPU, against Python integers and the RFC 7748 vectors.  The driver (tests/x25519_host/driver.cpp) is a
stand-alone program with its own main; it is compiled with g++ and run as a program."""
import os
import subprocess

import numpy as np
import pytest

import handshake_cases as hc
from conftest import REPO, load_golden

P = hc.P
SRC = os.path.join(REPO, "tests", "x25519_host", "driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("x25519") / "driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "rustyguard_amd", "csrc"), SRC, "-o", exe],
                   check=True)

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        out = r.stdout.split("\n")[:-1]
        assert len(out) == len(lines)
        return out

    return run


def _limb_ones():
    """every single-limb-all-ones pattern of the ten-limb layout (limb i: 26 / 25 bits at bit ceil(25.5 i))"""
    return [((1 << (25 if i & 1 else 26)) - 1) << ((51 * i + 1) // 2) for i in range(10)]


def _operands():
    rng = np.random.default_rng(25519)
    rand = [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") >> 1 for _ in range(200)]
    edge = [0, 1, 2, 18, 19, P - 1, P, P + 1, 2**255 - 1] + _limb_ones()
    assert 2**255 - 20 == P - 1 and 2**255 - 18 == P + 1
    return edge, rand


def _hx(x: int) -> str:
    return x.to_bytes(32, "little").hex()


def _form(mode, a, b):
    return {"n": a, "s": a + b, "d": a - b}[mode] % P


def test_rfc7748_vectors(driver):
    g = load_golden("handshake_full.json")["rfc7748"]
    lines = [f"x {v['scalar']} {v['u']}" for v in g["vectors"]] + ["iter 1", "iter 1000"]
    out = driver(lines)
    for v, o in zip(g["vectors"], out):
        assert o == v["out"] + " 1", v
    assert out[-2] == g["iter_1"] and out[-1] == g["iter_1000"]
    # the model agrees with the fixture (it is what the GPU tests compare with)
    for v in g["vectors"]:
        assert hc.x25519(bytes.fromhex(v["scalar"]), bytes.fromhex(v["u"])).hex() == v["out"]
    assert hc.rfc_iteration(1)[1].hex() == g["iter_1"]


def test_field_operations_vs_python_integers(driver):
    """multiply, square, invert and the x 121665 step on the edge values, every single-limb-all-ones pattern
    and 200 random values, each also on an unreduced sum and an unreduced difference as the ladder forms
    them; outputs are canonical bytes."""
    edge, rand = _operands()
    allv = edge + rand
    pairs = [(x, y) for x in edge for y in edge]
    pairs += [(r, rand[(i + 1) % len(rand)]) for i, r in enumerate(rand)]
    pairs += [(r, edge[i % len(edge)]) for i, r in enumerate(rand)] + [(edge[i % len(edge)], r) for i, r in enumerate(rand)]
    lines, want = [], []
    for n, (a, c) in enumerate(pairs):
        b, d = allv[(n * 7 + 3) % len(allv)], allv[(n * 11 + 5) % len(allv)]
        for m in ("nn", "ss", "dd", "sd", "ds"):
            lines.append(f"mul {m} {_hx(a)} {_hx(b)} {_hx(c)} {_hx(d)}")
            want.append(_form(m[0], a, b) * _form(m[1], c, d) % P)
    for n, a in enumerate(allv):
        for b in (allv[(n * 5 + 1) % len(allv)], edge[n % len(edge)]):
            for m in "nsd":
                x = _form(m, a, b)
                lines += [f"sq {m} {_hx(a)} {_hx(b)}", f"inv {m} {_hx(a)} {_hx(b)}", f"a24 {m} {_hx(a)} {_hx(b)}"]
                want += [x * x % P, pow(x, P - 2, P), 121665 * x % P]
    out = driver(lines)
    bad = [(ln, o, _hx(w)) for ln, o, w in zip(lines, out, want) if o != _hx(w)]
    assert not bad, (len(bad), bad[:3])


def test_edge_points(driver):
    """the points of small order, the values around p and around the masked top bit, under the RFC scalar and
    the all-zero and all-0xFF scalars: the model says which results are zero; 2^256 - 1 equals u = 18."""
    lines, want = [], []
    for k in hc.EDGE_SCALARS:
        for _, u in hc.EDGE_POINTS:
            lines.append(f"x {k.hex()} {u.hex()}")
            r = hc.x25519(k, u)
            want.append(f"{r.hex()} {int(r != bytes(32))}")
    out = driver(lines)
    assert out == want
    res = dict(zip([(ki, name) for ki in range(3) for name, _ in hc.EDGE_POINTS], out))
    for ki in range(3):
        assert res[(ki, "2^256-1")] == res[(ki, "18")] and res[(ki, "18")].endswith(" 1")
        for name in ("0", "1", "order8_a", "order8_b", "p-1", "p", "p+1"):
            assert res[(ki, name)] == "00" * 32 + " 0", name
        assert res[(ki, "2^255")] == "00" * 32 + " 0"  # bit 255 is masked: u = 0
        assert res[(ki, "2^255-1")].endswith(" 1")
