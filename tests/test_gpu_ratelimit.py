"""The device-resident handshake rate limiter on the GPU (rg_rate_count_batch_dev, rg_rate_turn_dev) against the
in-order Python model (tests/ratelimit_cases.py), and in the loop it exists for: turn -> count -> the under-load
filter on one stream, captured into a graph, with the count's flags as the filter's `overload` and no host step
between them.  Every output array has a guard entry behind it, and every bucket, seed and last_reset_ns byte is
compared with the model."""
import numpy as np
import pytest

import ratelimit_cases as rc
from oracle import oracle
from rustyguard_amd import _lib, aead, ratelimit
from rustyguard_amd.workloads import DESC_DTYPE

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL = 0xA5
GUARD = 0xA5A5A5A5
M32 = rc.M32
OK, COOKIE = aead.PKT_OK, aead.PKT_COOKIE
SEC = 10**9


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _clock(now):
    return _dev(np.array([now], np.uint64).view(np.int64))


def _fill(shape, dtype=torch.uint8):
    if dtype == torch.uint8:
        return torch.full(shape, FILL, dtype=dtype, device="cuda")
    return torch.full(shape, GUARD - (1 << 32), dtype=torch.int32, device="cuda")  # the same bytes


def _u32(t):
    return [int(x) for x in t.cpu().numpy().view(np.uint32).reshape(-1)]


def _u8(t):
    return [int(x) for x in t.cpu().numpy().reshape(-1)]


def _same(name, got, want):
    assert len(got) == len(want), name
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (name, len(bad), bad[:8], [(got[i], want[i]) for i in bad[:2]])


def _seed_rows(seeds):
    return _dev(np.array(seeds, np.uint64).reshape(-1, 2).view(np.uint8).reshape(-1, 16))


def _desc_dev(desc):
    return _dev(np.array(desc, DESC_DTYPE).view(np.uint8).reshape(-1, 16))


def _addrs_dev(addrs):
    return _dev(np.frombuffer(b"".join(addrs), np.uint8).reshape(len(addrs), 24))


def put_sketch(engine, s):
    """the model's sketch on the device"""
    depth, width = len(s["buckets"]), len(s["buckets"][0])
    T = ratelimit.RateTables(engine, width, depth)
    T.buckets[:] = _dev(np.array(s["buckets"], np.uint32).view(np.int32))
    T.seeds[:] = _seed_rows(s["seeds"])
    T.last_reset_ns[:] = _clock(s["last_reset_ns"])
    return T


def get_sketch(T):
    seeds = T.seeds.cpu().numpy().view(np.uint64).reshape(-1, 2)
    return {"buckets": [[int(x) for x in row] for row in T.buckets.cpu().numpy().view(np.uint32)],
            "seeds": [(int(a), int(b)) for a, b in seeds],
            "last_reset_ns": int(T.last_reset_ns.cpu().numpy().view(np.uint64)[0])}


def check_sketch(T, want):
    got = get_sketch(T)
    assert got["seeds"] == want["seeds"] and got["last_reset_ns"] == want["last_reset_ns"]
    for r, (g, w) in enumerate(zip(got["buckets"], want["buckets"])):
        _same(f"buckets[{r}]", g, w)


class Counted:
    """one count call: the inputs on the device, the two output arrays with a guard entry behind each"""

    def __init__(self, desc, addrs, buf, counts=True):
        self.n = n = len(desc)
        self.desc, self.addrs = _desc_dev(desc), _addrs_dev(addrs)
        self.buf = _dev(np.frombuffer(buf, np.uint8))
        self.buf_before = bytes(buf)
        self.counts = _fill((n + 1,), torch.int32) if counts else None
        self.flags = _fill((n + 1,))

    def run(self, engine, T, limit=rc.LIMIT, ws=None, stream=None):
        n = self.n
        return ratelimit.count_dev(engine, T, self.desc, self.addrs, self.buf, self.flags[:n],
                                   None if self.counts is None else self.counts[:n], limit, workspace=ws, stream=stream)

    def read(self):
        torch.cuda.synchronize()
        n, flags = self.n, _u8(self.flags)
        assert flags[n] == FILL and self.buf.cpu().numpy().tobytes() == self.buf_before  # buf is never written
        if self.counts is None:
            return None, flags[:n]
        counts = _u32(self.counts)
        assert counts[n] == GUARD
        return counts[:n], flags[:n]


def count_vs_model(engine, s, desc, addrs, buf, limit=rc.LIMIT, counts=True):
    T, c = put_sketch(engine, s), Counted(desc, addrs, buf, counts)
    c.run(engine, T, limit)
    want, w_counts, w_flags = rc.count_loop(s, desc, addrs, buf, limit)
    got_counts, got_flags = c.read()
    if counts:
        _same("counts_out", got_counts, w_counts)
    _same("overload_out", got_flags, w_flags)
    check_sketch(T, want)
    return want, w_counts, w_flags


# ------------------------------------------------------------------- count
@pytest.mark.parametrize("n", rc.SIZES)
def test_count_sizes_against_the_model(engine, n):
    """wave edges, the scan-tile edge and more than two tiles of the n * depth item space; one bucket for everything,
    heavy collisions, a bucket range that needs a second radix pass and the default sketch; one address, three in
    turn and all distinct; from random nonzero buckets"""
    for shape in rc.SHAPES:
        for kind in rc.KINDS:
            s, desc, addrs, buf = rc.size_case(n, shape, kind)
            want, counts, flags = count_vs_model(engine, s, desc, addrs, buf)
            assert all(c > 0 for c in counts)
            if n >= 2047:  # a condition on the inputs: the model puts messages on both sides of the limit
                assert 0 < sum(flags) < n, (shape, kind)


def test_uncounted_messages_move_nothing(engine):
    """an unaligned offset, a frame past buf_len, len 147, a type word that disagrees with len and RG_KEY_SKIP, each
    between counted messages of its address: count 0, flag 0, no bucket moved, the neighbours' counts as without
    them; counts_out may be NULL"""
    rng = np.random.default_rng(8)
    desc, addrs, buf, skipped = rc.uncounted_case(rng)
    for shape, limit in (((3, 2), 12), ((rc.WIDTH, rc.DEPTH), 4)):
        s = rc.start_sketch(*shape, 1)
        want, counts, flags = count_vs_model(engine, s, desc, addrs, buf, limit)
        assert all(counts[i] == 0 and flags[i] == 0 for i in skipped) and 0 in flags and 1 in flags
        keep = [i for i in range(len(desc)) if i not in skipped]
        alone = count_vs_model(engine, s, [desc[i] for i in keep], [addrs[i] for i in keep], buf, limit)
        assert alone[0] == want and alone[1] == [counts[i] for i in keep]
        count_vs_model(engine, s, desc, addrs, buf, limit, counts=False)
    # a batch with no counted message at all: zeros, and the sketch stays byte for byte
    s = rc.start_sketch(3, 2, 2)
    none = [desc[i] for i in skipped]
    want, counts, flags = count_vs_model(engine, s, none, [addrs[0]] * len(none), buf)
    assert want == s and counts == flags == [0] * len(none)


def test_saturation(engine):
    """buckets at 0xFFFFFFF0, then 40 messages of one address: the count stops at 0xFFFFFFFF and stays"""
    n = 40
    for shape in ((1, 1), (3, 2), (rc.WIDTH, rc.DEPTH)):
        s = rc.start_sketch(*shape, 3)
        s["buckets"] = [[0xFFFFFFF0] * shape[0] for _ in range(shape[1])]
        _, desc, addrs, buf = rc.size_case(n, shape, "one")
        want, counts, flags = count_vs_model(engine, s, desc, addrs, buf, limit=M32 - 1)
        assert counts == [min(0xFFFFFFF0 + k, M32) for k in range(1, n + 1)] and flags == [0] * 14 + [1] * 26
        assert sorted({b for row in want["buckets"] for b in row}) == ([M32] if shape == (1, 1) else [0xFFFFFFF0, M32])
        want2, counts2, flags2 = count_vs_model(engine, want, desc[:3], addrs[:3], buf, limit=M32)
        assert counts2 == [M32] * 3 and flags2 == [0] * 3 and want2 == want


# -------------------------------------------------------------------- turn
def _turn(engine, T, now, new_seeds, period, reset=None):
    reset = _fill((2,), torch.int32) if reset is None else reset
    ratelimit.turn_dev(engine, T, _clock(now), _seed_rows(new_seeds), reset[:1], period)
    torch.cuda.synchronize()
    got = _u32(reset)
    assert got[1] == GUARD
    return got[0]


def test_turn_against_the_model(engine):
    """no reset leaves every byte alone and the seeds as they were; a reset wipes and reseeds; period = 0 resets
    whenever the clock moved"""
    rng = np.random.default_rng(21)
    P = rc.PERIOD_NS
    for shape in ((1, 1), (3, 2), (257, 3), (rc.WIDTH, rc.DEPTH), (300, 8)):
        s = rc.start_sketch(*shape, 9)
        s["last_reset_ns"] = last = 7 * SEC
        new = rc.seeds_for(shape[1], rng)
        for now, period in ((last, P), (last, 0), (last - 1, P), (0, 0), (last + P, P), (last + P + 1, P),
                            (last + 1, 0), (rc.M64, P)):
            T = put_sketch(engine, s)
            want, w_reset = rc.turn_loop(s, now, period, new)
            assert _turn(engine, T, now, new, period) == w_reset, (shape, now, period)
            check_sketch(T, want)
            assert (want == s) == (not w_reset) and (not w_reset or want["seeds"] == new != s["seeds"])
    # a sketch that starts empty at 0: the first turn past the period resets it, the next at that clock does not
    T, s = ratelimit.RateTables(engine, 3, 2), rc.new_sketch(3, 2)
    for now, w_reset in ((P, 0), (P + 1, 1), (P + 1, 0), (2 * P + 1, 0), (2 * P + 2, 1)):
        new = rc.seeds_for(2, rng)
        s, flag = rc.turn_loop(s, now, P, new)
        assert flag == w_reset and _turn(engine, T, now, new, P) == w_reset
        check_sketch(T, s)


# -------------------------------------------------------------- fail closed
def test_short_workspace_enqueues_nothing(engine):
    n, shape = 65, (257, 3)
    s, desc, addrs, buf = rc.size_case(n, shape, "three")
    T, c = put_sketch(engine, s), Counted(desc, addrs, buf)
    need = ratelimit.workspace_size(engine, n, *shape)
    assert need == ratelimit.workspace_size(engine, n, shape[0], shape[1]) > 0
    ws = _fill((need,))
    with pytest.raises(_lib.RgError, match="rate count"):
        c.run(engine, T, ws=ws[:need - 1])
    assert c.read() == ([GUARD] * n, [FILL] * n)
    assert (ws.cpu().numpy() == FILL).all()
    check_sketch(T, s)
    with pytest.raises(_lib.RgError, match="sketch"):
        ratelimit.rate_workspace(engine, n, 0, 3)
    c.run(engine, T, ws=ws)  # and the same workspace at its full length serves
    assert c.read()[0] == rc.count_loop(s, desc, addrs, buf)[1]


# ------------------------------------------------------- the loop it is for
def _stamp_mac1(msg: bytearray, ck: bytes):
    L = len(msg)
    msg[L - 32:L - 16] = oracle.blake2s(bytes(msg[:L - 32]), ck[:32], 16)


def _cookie_reply(ck: bytes, msg: bytes, addr: bytes, nonce: bytes) -> bytes:
    """Sessions::write_cookie_message from the oracle's primitives (tests/test_gpu_cookie.py)"""
    L = len(msg)
    mac1 = msg[L - 32:L - 16]
    ct, tag = oracle.xaead_seal(ck[32:64], nonce, mac1, oracle.blake2s(addr[:18], ck[64:96], 16))
    return (3).to_bytes(4, "little") + msg[4:8] + nonce + ct + tag


class Responder:
    """eight valid initiations (mac1 valid, mac2 zero), six from one address and two from another, and every array
    of turn -> count -> filter, allocated once so that the same calls can be captured"""

    N, FIRST = 8, (0, 1, 2, 4, 5, 7)  # the first address's messages; 3 and 6 are the second's

    def __init__(self, engine, seed):
        rng = np.random.default_rng(seed)
        n = self.N
        self.engine = engine
        self.ck = rng.integers(0, 256, 96, dtype=np.uint8).tobytes()
        a, b = rc.addr("192.0.2.33", 4000), rc.addr("2001:db8:7:8::9", 4001)
        self.addrs = [a if i in self.FIRST else b for i in range(n)]
        self.msgs, buf = [], bytearray(160 * n)
        for i in range(n):
            msg = bytearray(rng.integers(0, 256, rc.INIT_LEN, dtype=np.uint8).tobytes())
            msg[0:4] = (1).to_bytes(4, "little")
            _stamp_mac1(msg, self.ck)
            msg[-16:] = bytes(16)
            buf[160 * i:160 * i + rc.INIT_LEN] = msg
            self.msgs.append(bytes(msg))
        self.desc = [(160 * i, rc.INIT_LEN, 0) for i in range(n)]
        self.buf = bytes(buf)
        self.nonces = rng.integers(0, 256, (n, 24), dtype=np.uint8)
        self.new_seeds = rc.seeds_for(rc.DEPTH, rng)
        self.d_ck, self.d_nonces = _dev(np.frombuffer(self.ck, np.uint8)), _dev(self.nonces)
        self.d_new = _seed_rows(self.new_seeds)
        self.c = Counted(self.desc, self.addrs, self.buf)
        self.T = ratelimit.RateTables(engine)
        self.ws = ratelimit.rate_workspace(engine, n)
        self.d_now, self.reset = _clock(0), _fill((2,), torch.int32)
        self.replies, self.status = _fill((n + 1, 64)), _fill((n + 1,))

    def clear(self):
        for t in (self.T.buckets, self.T.seeds, self.T.last_reset_ns):
            t.zero_()
        for t in (self.reset, self.replies, self.status, self.c.counts, self.c.flags):
            t.fill_(FILL if t.dtype == torch.uint8 else GUARD - (1 << 32))

    def chain(self, stream=None):
        """rg_rate_turn_dev -> rg_rate_count_batch_dev -> rg_cookie_reply_batch_dev, the flags as `overload`"""
        e, n = self.engine, self.N
        ratelimit.turn_dev(e, self.T, self.d_now, self.d_new, self.reset[:1], stream=stream)
        self.c.run(e, self.T, ws=self.ws, stream=stream)
        e.cookie_reply_dev(self.d_ck, self.c.desc, self.c.addrs, self.c.flags[:n], self.d_nonces, self.c.buf,
                           self.replies[:n], self.status[:n], stream=stream)

    def snapshot(self):
        counts, flags = self.c.read()
        status, reset = _u8(self.status), _u32(self.reset)
        assert status[self.N] == FILL and reset[1] == GUARD
        return (get_sketch(self.T), counts, flags, status[:self.N], reset[0],
                self.replies.cpu().numpy()[:self.N].tobytes(), self.replies.cpu().numpy()[self.N].tobytes())


def test_turn_count_and_filter_captured(engine):
    """turn -> count -> filter captured once and replayed three times, each replay against the same calls run
    uncaptured from the same start and against the model: at the first clock all eight initiations pass; at the same
    clock again the first address's 11th and 12th get a cookie reply, the oracle's; two seconds on the sketch was
    reset and all eight pass"""
    w = Responder(engine, 77)
    n, t0 = w.N, 50 * SEC
    clocks = (t0, t0, t0 + 2 * SEC)

    def run(step):
        out = []
        w.clear()
        for now in clocks:
            w.d_now.copy_(_clock(now))
            w.replies.fill_(FILL)
            step()
            out.append(w.snapshot())
        return out

    want = run(w.chain)
    # the model: the same three turns and counts
    s, empty = rc.new_sketch(), bytes([FILL]) * 64
    late = [i for i in w.FIRST[4:]]  # messages 5 and 6 of the first address
    for k, now in enumerate(clocks):
        s, reset = rc.turn_loop(s, now, rc.PERIOD_NS, w.new_seeds)
        s, counts, flags = rc.count_loop(s, w.desc, w.addrs, w.buf)
        sketch, g_counts, g_flags, status, g_reset, replies, guard = want[k]
        assert reset == g_reset == (0 if k == 1 else 1) and sketch == s and g_counts == counts and g_flags == flags
        assert guard == empty
        over = late if k == 1 else []
        assert flags == [1 if i in over else 0 for i in range(n)]
        assert status == [COOKIE if i in over else OK for i in range(n)]
        for i in range(n):
            row = replies[64 * i:64 * i + 64]
            assert row == (_cookie_reply(w.ck, w.msgs[i], w.addrs[i], w.nonces[i].tobytes()) if i in over else empty), (k, i)
    assert [want[1][1][i] for i in w.FIRST] == [7, 8, 9, 10, 11, 12] and [want[1][1][i] for i in (3, 6)] == [3, 4]
    assert want[2][1] == want[0][1] == [1, 2, 3, 1, 4, 5, 2, 6]

    stream, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    w.clear()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=stream):
        w.chain(stream=stream)
    torch.cuda.synchronize()
    got = run(g.replay)
    for k in range(3):
        for name, a, b in zip(("sketch", "counts_out", "overload_out", "status", "reset_out", "replies", "guard row"),
                              got[k], want[k]):
            assert a == b, (name, k)
