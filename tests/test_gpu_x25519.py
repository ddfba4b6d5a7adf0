"""rg_x25519_batch_dev on the GPU against RFC 7748 and the Python model (tests/handshake_cases.py): the same
field arithmetic tests/test_x25519_cpu.py checks on the host, now as the kernel runs it.  All comparisons are
byte-exact."""
import ctypes

import numpy as np
import pytest

import handshake_cases as hc
from conftest import load_golden
from rustyguard_amd import aead

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL = 0xA5
WG = 64  # the kernels' workgroup size (rg_handshake.hip kHsWG)


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _rows(bs):
    return np.frombuffer(b"".join(bs), np.uint8).reshape(len(bs), 32)


def _run(engine, scalars, points, extra=3):
    """out and status of one call; `extra` rows beyond n are preset to 0xA5 and must come back unchanged."""
    n = len(scalars)
    out = torch.full((n + extra, 32), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((n + extra,), FILL, dtype=torch.uint8, device="cuda")
    engine.x25519_dev(_dev(_rows(scalars)), None if points is None else _dev(_rows(points)), out[:n], status[:n])
    torch.cuda.synchronize()
    out, status = out.cpu().numpy(), status.cpu().numpy()
    assert (out[n:] == FILL).all() and (status[n:] == FILL).all()
    return [o.tobytes() for o in out[:n]], list(status[:n])


def test_rfc7748_iteration_as_one_batch(engine):
    """all 1000 (k, u) pairs of the RFC's iterated test in one batch: row i's output is row i + 1's scalar,
    and the last output is the RFC's value after 1000 steps."""
    g = load_golden("handshake_full.json")["rfc7748"]
    pairs, last = hc.rfc_iteration(1000)
    assert last.hex() == g["iter_1000"]
    out, st = _run(engine, [p[0] for p in pairs], [p[1] for p in pairs])
    assert st == [aead.PKT_OK] * 1000
    assert out[0].hex() == g["iter_1"] and out[-1].hex() == g["iter_1000"]
    assert out[:-1] == [p[0] for p in pairs[1:]]


def test_rfc7748_vectors_and_base_point(engine):
    g = load_golden("handshake_full.json")["rfc7748"]["vectors"]
    v = [x for x in g if x["u"] != hc.BASE.hex()]
    out, st = _run(engine, [bytes.fromhex(x["scalar"]) for x in v], [bytes.fromhex(x["u"]) for x in v])
    assert [o.hex() for o in out] == [x["out"] for x in v] and st == [aead.PKT_OK] * len(v)
    alice = [x for x in g if x["u"] == hc.BASE.hex()]
    assert len(v) == 2 and len(alice) == 1
    out, st = _run(engine, [bytes.fromhex(alice[0]["scalar"])], None)  # points = NULL: the base point
    assert out[0].hex() == alice[0]["out"] and st == [aead.PKT_OK]


def test_edge_points_with_statuses(engine):
    cases = [(k, u) for k in hc.EDGE_SCALARS for _, u in hc.EDGE_POINTS]
    want = [hc.x25519(k, u) for k, u in cases]
    out, st = _run(engine, [c[0] for c in cases], [c[1] for c in cases])
    assert out == want
    assert st == [aead.PKT_KEYEXCHANGE if w == bytes(32) else aead.PKT_OK for w in want]
    names = [n for _, n in [(k, n) for k in hc.EDGE_SCALARS for n, _ in hc.EDGE_POINTS]]
    zero = {n for n, w in zip(names, want) if w == bytes(32)}
    assert zero == {"0", "1", "order8_a", "order8_b", "p-1", "p", "p+1", "2^255"}
    by = dict(zip(zip([ki for ki in range(3) for _ in hc.EDGE_POINTS], names), out))
    for ki in range(3):
        assert by[(ki, "2^256-1")] == by[(ki, "18")]


@pytest.mark.parametrize("n", [1, 63, 64, 65, WG + 1, 4 * WG + 1])
def test_random_rows_vs_model(engine, n):
    rng = np.random.default_rng(7748)  # the same stream for every n: the model's results are cached
    rows = [(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, 32, dtype=np.uint8).tobytes())
            for _ in range(n)]
    out, st = _run(engine, [r[0] for r in rows], [r[1] for r in rows])
    assert out == [hc.x25519(k, u) for k, u in rows] and st == [aead.PKT_OK] * n
    if n == 65:
        out, st = _run(engine, [r[0] for r in rows], None)
        assert out == [hc.pubkey(k) for k, _ in rows]


def test_argument_refusals(engine):
    L, h = engine.library, engine.handle
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    k = _dev(np.zeros((4, 32), np.uint8))
    out = torch.full((4, 32), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((4,), FILL, dtype=torch.uint8, device="cuda")
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    assert L.rg_x25519_batch_dev(h, p(k), None, p(out), p(status), 0, s) == 0
    assert L.rg_x25519_batch_dev(h, None, None, p(out), p(status), 4, s) == -1
    assert L.rg_x25519_batch_dev(h, p(k), None, None, p(status), 4, s) == -1
    assert L.rg_x25519_batch_dev(h, p(k), None, p(out), None, 4, s) == -1
    assert L.rg_x25519_batch_dev(h, p(k, 2), None, p(out), p(status), 3, s) == -1
    assert L.rg_x25519_batch_dev(h, p(k), p(k, 1), p(out), p(status), 3, s) == -1
    assert L.rg_x25519_batch_dev(h, p(k), None, p(out, 2), p(status), 3, s) == -1
    assert L.rg_x25519_batch_dev(h, p(k), None, p(out), p(status), 1 << 32, s) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == FILL).all() and (status.cpu().numpy() == FILL).all()
