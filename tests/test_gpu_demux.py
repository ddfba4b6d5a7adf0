"""The inbound demultiplexer on the GPU (rg_demux_batch_dev, rg_demux_verdict_batch_dev) against the in-order model
(tests/demux_cases.py): every output array starts a call filled with a fill byte, has a guard row behind it and is
compared whole.  The demux never writes buf, so every descriptor points into one buf of a kilobyte and the large
batches stay cheap.  The composition of the split with the chains it feeds is tests/test_gpu_demux_chain.py."""
import ctypes

import numpy as np
import pytest

import demux_cases as dc
from rustyguard_amd import demux
from rustyguard_amd._lib import RgError

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL = 0xA5
SIZES = (1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 5)
OUTPUTS = ("hs_desc", "hs_addrs", "init_desc", "resp_desc", "ck_desc", "data_desc", "data_addrs")
WIDTH = dict(hs_desc=16, hs_addrs=24, init_desc=16, resp_desc=16, ck_desc=16, data_desc=16, data_addrs=24)


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _bytes(a):
    """a model array as the bytes the device holds"""
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class Guarded(demux.Demux):
    """a Demux whose every output is filled with FILL and has a guard row (or word) behind it"""

    def __init__(self, engine, n, caps):
        super().__init__(engine, n, *caps)
        self.caps = caps
        cap_of = dict(hs_desc=caps[0], hs_addrs=caps[0], init_desc=caps[0], resp_desc=caps[0], ck_desc=caps[1],
                      data_desc=caps[2], data_addrs=caps[2])
        self.whole = {k: torch.empty((c + 1, WIDTH[k]), dtype=torch.uint8, device="cuda") for k, c in cap_of.items()}
        self.whole.update(status=torch.empty(n + 1, dtype=torch.uint8, device="cuda"),
                          cls=torch.empty(n + 1, dtype=torch.uint8, device="cuda"),
                          pos=torch.empty(n + 1, dtype=torch.int32, device="cuda"),
                          counts=torch.empty(7, dtype=torch.int32, device="cuda"))
        for k, t in self.whole.items():
            setattr(self, k, t[:-1])
        self.refill()

    def refill(self):
        for t in self.whole.values():
            t.view(torch.uint8).fill_(FILL)

    def untouched(self):
        return all(bool((t.view(torch.uint8) == FILL).all()) for t in self.whole.values())

    def check(self, want, n, what):
        """every byte of every output against the model's; per-datagram arrays past n and every guard keep FILL"""
        torch.cuda.synchronize()
        for k, t in self.whole.items():
            got = t.view(torch.uint8).cpu().numpy().reshape(len(t), -1)
            w = _bytes(want[k]).reshape(len(want[k]), got.shape[1])
            bad = np.nonzero((got[:len(w)] != w).any(axis=1))[0]
            assert len(bad) == 0, (what, k, len(bad), bad[:8], got[bad[0]].tobytes().hex(), w[bad[0]].tobytes().hex())
            assert (got[len(w):] == FILL).all(), (what, k, "past the end")


def _run(engine, n, mix, caps, seed=0, buf=None):
    buf = dc.make_buf() if buf is None else buf
    desc, addrs = dc.mixed_desc(n, mix, seed), dc.rand_addrs(n, seed)
    want = dc.demux_model(desc, addrs, buf, caps)
    d = Guarded(engine, n, caps)
    d_desc, d_addrs, d_buf = _dev(desc.view(np.uint8).reshape(-1, 16)), _dev(addrs), _dev(buf)
    d.batch_dev(d_desc, d_addrs, d_buf)
    d.check(want, n, (n, mix, caps))
    assert np.array_equal(d_buf.cpu().numpy(), buf) and np.array_equal(d_addrs.cpu().numpy(), addrs)
    return d, want, (d_desc, d_addrs, d_buf)


@pytest.mark.parametrize("n", SIZES)
def test_sizes_across_lane_wave_and_tile_edges(engine, n):
    """every class and every kind of junk at random, lists with room for everything and then lists half as long as
    what arrives; the small sizes also through the literal loop"""
    _, want, _ = _run(engine, n, "random", (n, n, n))
    if n <= 2049:
        desc, addrs = dc.mixed_desc(n, "random"), dc.rand_addrs(n)
        loop = dc.demux_loop(desc, addrs, dc.make_buf(), (n, n, n))
        assert all(np.array_equal(loop[k], want[k]) for k in want)
    seen = [int(x) for x in want["counts"][3:]]
    _run(engine, n, "random", tuple(s // 2 for s in seen), seed=1)


def test_carry_loop_runs_more_than_once(engine):
    """256 * 2048 + 1 datagrams: 257 tiles, so each lane of the carry pass walks more than one tile's sum"""
    n = 256 * dc.TILE + 1
    _, want, _ = _run(engine, n, "random", (50000, 20000, 30000))
    assert all(int(want["counts"][3 + j]) > int(want["counts"][j]) > 0 for j in range(3))  # every list overflows


@pytest.mark.parametrize("mix", [m for m in dc.MIXES if m != "random"])
def test_class_mixes(engine, mix):
    """all one class, strict alternation 1, 2, 3, 4, junk, one class only in the last tile, and all junk, which
    leaves every list entirely inert"""
    n = 3 * dc.TILE + 5
    _, want, _ = _run(engine, n, mix, (n, 77, n))
    seen = [int(x) for x in want["counts"][3:]]
    if mix == "junk":
        assert seen == [0, 0, 0] and (want["status"] != dc.PENDING).all()
    if mix == "last_tile":
        first = int(np.nonzero(want["cls"] == 3)[0][0])
        assert first >= 3 * dc.TILE and seen[1] > 0
    if mix == "alternate":
        assert seen[0] == 2 * seen[1] and list(want["cls"][:4]) == [1, 2, 3, 4]


def test_capacities(engine):
    n = 2 * dc.TILE + 77
    desc, addrs, buf = dc.mixed_desc(n, "random"), dc.rand_addrs(n), dc.make_buf()
    seen = [int(x) for x in dc.demux_model(desc, addrs, buf, (n, n, n))["counts"][3:]]
    base = dc.demux_model(desc, addrs, buf, tuple(seen))
    assert not (base["status"] == dc.FULL).any()
    _run(engine, n, "random", tuple(seen))  # cap == seen
    for j in range(3):  # cap == seen - 1: the last message of the class reads RG_PKT_FULL and nothing else moves
        caps = tuple(s - (k == j) for k, s in enumerate(seen))
        _, want, _ = _run(engine, n, "random", caps)
        full = np.nonzero(want["status"] == dc.FULL)[0]
        last = np.nonzero(np.isin(want["cls"], ((1, 2), (3,), (4,))[j]))[0][-1]
        assert list(full) == [last]
        rest = np.arange(n) != last
        assert np.array_equal(want["status"][rest], base["status"][rest]) and np.array_equal(want["pos"][rest], base["pos"][rest])
        caps0 = tuple(0 if k == j else s for k, s in enumerate(seen))  # cap == 0 for one class: its arrays may be NULL
        _, want, _ = _run(engine, n, "random", caps0)
        assert int(want["counts"][j]) == 0 and int(want["counts"][3 + j]) == seen[j]
    _run(engine, n, "random", (n + 1000, n + 1, 3 * n))  # cap > n
    _run(engine, n, "random", (0, 0, 0))


def test_inert_tail_on_a_second_call(engine):
    """a full first batch, then a short mixed one into the same arrays: every row behind the new counts is inert,
    and the per-datagram outputs past the second batch keep the first one's bytes"""
    n1, n2 = 5000, 300
    caps = (n1, n1, n1)
    d, first, _ = _run(engine, n1, "alternate", caps)
    desc, addrs, buf = dc.mixed_desc(n2, "random", 9), dc.rand_addrs(n2, 9), dc.make_buf()
    want = dc.demux_model(desc, addrs, buf, caps)
    d.batch_dev(_dev(desc.view(np.uint8).reshape(-1, 16)), _dev(addrs), _dev(buf))
    for k in ("status", "cls", "pos"):
        want[k] = np.concatenate([want[k], first[k][n2:]])
    d.check(want, n1, "second call")
    assert int(want["counts"][0]) < int(first["counts"][0])


def test_argument_checks_leave_everything_untouched(engine):
    n = 100
    caps = (n, n, n)
    d = Guarded(engine, n, caps)
    desc, addrs, buf = dc.mixed_desc(n, "random"), dc.rand_addrs(n), dc.make_buf()
    d_desc, d_addrs, d_buf = _dev(desc.view(np.uint8).reshape(-1, 16)), _dev(addrs), _dev(buf)
    L, h = engine.library, engine.handle
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert int(L.rg_demux_workspace_size(1 << 32)) == 0 and int(L.rg_demux_workspace_size((1 << 32) - 1)) > 0
    assert int(L.rg_demux_workspace_size(0)) > 0

    def call(desc=p(d_desc), addrs=p(d_addrs), n=n, buf=p(d_buf), lists=None, status=p(d.status), cls=p(d.cls),
             pos=p(d.pos), counts=p(d.counts), ws=p(d.workspace), ws_len=d.workspace.numel(), ctx=h):
        lists = d.lists() if lists is None else lists
        return L.rg_demux_batch_dev(ctx, desc, addrs, n, buf, len(dc.make_buf()), ctypes.byref(lists) if lists else None,
                                    status, cls, pos, counts, ws, ws_len, None)

    off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)  # noqa: E731
    assert call(ctx=None) == -1
    for name in ("desc", "addrs", "buf", "status", "cls", "pos", "counts", "ws"):
        assert call(**{name: None}) == -1, name
    assert call(lists=False) == -1
    for field in ("hs_desc", "hs_addrs", "init_desc", "resp_desc", "ck_desc", "data_desc", "data_addrs"):
        lists = d.lists()
        setattr(lists, field, None)
        assert call(lists=lists) == -1, field
        lists = d.lists()
        setattr(lists, field, getattr(lists, field) + 4)
        assert call(lists=lists) == -1, (field, "misaligned")
    assert call(n=1 << 32) == -1
    assert call(desc=off(d_desc, 8)) == -1 and call(addrs=off(d_addrs, 4)) == -1 and call(pos=off(d.pos, 2)) == -1
    assert call(counts=off(d.counts, 1)) == -1 and call(buf=off(d_buf, 2)) == -1 and call(ws=off(d.workspace, 8)) == -1
    assert call(ws_len=int(L.rg_demux_workspace_size(n)) - 1) == -1
    assert call(n=0, desc=None) == 0  # n == 0: RG_OK, nothing written
    torch.cuda.synchronize()
    assert d.untouched()
    # the way back
    def back(cls=p(d.cls), pos=p(d.pos), n=n, status=p(d.status), ctx=h):  # noqa: E306
        return L.rg_demux_verdict_batch_dev(ctx, cls, pos, n, None, None, None, n, None, n, None, n, status, None)

    assert back(ctx=None) == -1 and back(cls=None) == -1 and back(pos=None) == -1 and back(status=None) == -1
    assert back(n=1 << 32) == -1 and back(pos=off(d.pos, 2)) == -1 and back(n=0, cls=None) == 0
    torch.cuda.synchronize()
    assert d.untouched()
    with pytest.raises(RgError):
        engine._check(call(n=1 << 32), "rg_demux_batch_dev")
    assert call() == 0  # and the same arguments, all in order, run
    d.check(dc.demux_model(desc, addrs, buf, caps), n, "after the refusals")


def _chains(caps, seed):
    rng = np.random.default_rng(seed)
    verdicts = np.array([dc.OK, dc.OK, dc.REJECTED, dc.INVALID, dc.COOKIE, dc.DECRYPT_ERR], np.uint8)
    return {k: rng.choice(verdicts, c) for k, c in (("filter", caps[0]), ("init", caps[0]), ("finish", caps[0]),
                                                    ("cookie", caps[1]), ("data", caps[2]))}


def _verdict(d, n, chains):
    dev = {k: (None if v is None else _dev(v)) for k, v in chains.items()}
    d.verdict_batch_dev(n, dev["filter"], dev["init"], dev["finish"], dev["cookie"], dev["data"])
    torch.cuda.synchronize()
    return d.whole["status"].cpu().numpy()


@pytest.mark.parametrize("n", (65, 2 * 2048 + 3))
def test_verdict_against_the_model(engine, n):
    caps = (n // 3, 5, n // 4)
    d, want, _ = _run(engine, n, "random", caps)
    chains = _chains(caps, n)
    status0 = d.status.clone()
    got = _verdict(d, n, chains)
    final = dc.verdict_model(want["status"], want["cls"], want["pos"], caps, chains)
    assert np.array_equal(got[:n], final) and got[n] == FILL and not (final == dc.PENDING).any()
    for gone in chains:  # a chain that did not run leaves its datagrams pending
        d.status.copy_(status0)
        part = {k: (None if k == gone else v) for k, v in chains.items()}
        got = _verdict(d, n, part)
        assert np.array_equal(got[:n], dc.verdict_model(want["status"], want["cls"], want["pos"], caps, part)), gone
    # a pos out of range and a cls outside 1-4 stay pending and are never used as an index
    cls, pos = want["cls"].copy(), want["pos"].copy()
    pend = np.nonzero(want["status"] == dc.PENDING)[0]
    for i in pend[:12]:
        pos[i] = caps[dc.LISTS.index(dc.list_of(int(cls[i])))] + (0 if i % 2 else 0x7FFFFFFF)
    for i in pend[12:16]:
        cls[i] = (0, 5, 255, 17)[i % 4]
    d.status.copy_(status0)
    d.cls.copy_(_dev(cls))
    d.pos.copy_(_dev(pos.view(np.int32)))
    got = _verdict(d, n, chains)
    model = dc.verdict_model(want["status"], cls, pos, caps, chains)
    assert np.array_equal(got[:n], model) and (model[pend[:16]] == dc.PENDING).all()


def test_demux_and_verdict_captured_and_replayed(engine):
    """demux -> verdict captured into a graph with no memset node; replayed, then replayed with the type words of
    buf changed, so that every class lands elsewhere"""
    n = dc.TILE + 100
    caps = (500, 40, 900)
    desc, addrs, buf = dc.mixed_desc(n, "random", 4), dc.rand_addrs(n, 4), dc.make_buf()
    d = Guarded(engine, n, caps)
    d_desc, d_addrs, d_buf = _dev(desc.view(np.uint8).reshape(-1, 16)), _dev(addrs), _dev(buf)
    chains = _chains(caps, 5)
    dev = {k: _dev(v) for k, v in chains.items()}

    def chain(stream=None):
        d.batch_dev(d_desc, d_addrs, d_buf, stream=stream)
        d.verdict_batch_dev(n, dev["filter"], dev["init"], dev["finish"], dev["cookie"], dev["data"], stream=stream)

    chain()  # the shape once, outside the capture
    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        chain(stream=s)
    torch.cuda.synchronize()
    swapped = buf.copy()
    for a, b in ((1, 4), (2, 3), (0, 5)):  # the type words trade places
        for x, y in ((a, b), (b, a)):
            swapped[dc.SLOTS[x]:dc.SLOTS[x] + 4] = np.frombuffer(np.uint32(y).tobytes(), np.uint8)
    for image in (buf, swapped, buf):
        d.refill()
        d_buf.copy_(_dev(image))
        torch.cuda.synchronize()
        g.replay()
        want = dc.demux_model(desc, addrs, image, caps)
        want["status"] = dc.verdict_model(want["status"], want["cls"], want["pos"], caps, chains)
        d.check(want, n, "replay")
    assert not np.array_equal(dc.demux_model(desc, addrs, swapped, caps)["cls"], dc.demux_model(desc, addrs, buf, caps)["cls"])
