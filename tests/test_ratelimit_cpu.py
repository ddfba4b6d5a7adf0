"""The device-resident handshake rate limiter, the part that needs no GPU: the ABI surface (header, both libraries,
ctypes table, source list), the layout of rg_rate_seed and rg_rate_tables and the constants, the library's hash
against the model's, the key derivation, the sequential model (tests/ratelimit_cases.py) against the reference's own
unit tests, rg_rate_workspace_size, the argument rules -- each answered before the device is touched -- and the turn
model, one case per line of its loop."""
import ctypes
import math
import os
import re
import subprocess
import textwrap

import numpy as np

import ratelimit_cases as rc
from conftest import REPO
from rustyguard_amd import _lib, build, ratelimit

NAMES = ("rg_rate_column", "rg_rate_workspace_size", "rg_rate_count_batch_dev", "rg_rate_turn_dev")
EINVAL, EDEVICE = -1, -2
M32, M64 = rc.M32, rc.M64


def test_header_libraries_and_binding_have_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "rg_aead.h")).read(), flags=re.S)
    build.build()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _lib.SIGNATURES
        for path in (build.LIB, build.TEST_LIB):
            out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
            assert f" T {name}\n" in out, (name, path)
    assert re.search(r"#define\s+RG_ABI_VERSION\s+6\b", text)  # additive: the version stays
    assert _lib.lib().rg_abi_version() == 6
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [3, 3, 13, 7]
    assert "rg_ratelimit.hip" in build.KERNELS and "rg_ratelimit.hip" not in build.HOST
    assert "rg_ratehash.h" in build.HEADERS
    for unit in build.HOST:
        assert "rg_rate_" not in open(os.path.join(build.CSRC, unit)).read(), unit


def test_layout_and_constants_with_gcc(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "rg_aead.h"
        int main(void) {
            printf("%zu %zu %zu %zu\\n", sizeof(rg_rate_seed), _Alignof(rg_rate_seed), offsetof(rg_rate_seed, a),
                   offsetof(rg_rate_seed, b));
            printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(rg_rate_tables), offsetof(rg_rate_tables, buckets),
                   offsetof(rg_rate_tables, seeds), offsetof(rg_rate_tables, last_reset_ns),
                   offsetof(rg_rate_tables, width), offsetof(rg_rate_tables, depth));
            printf("%u %u %u %u %llu\\n", RG_RATE_WIDTH, RG_RATE_DEPTH, RG_RATE_LIMIT, RG_RATE_MAX_DEPTH,
                   RG_RATE_PERIOD_NS);
            return 0;
        }
    """))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                   check=True)
    vals = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert vals[:4] == [16, 8, 0, 8]
    assert vals[4:10] == [32, 0, 8, 16, 24, 28]
    # CountMinSketch::with_params(10.0 / 20_000.0, 0.01): width = ceil(e / epsilon), depth = ceil(ln(1 / delta))
    width, depth = math.ceil(math.e / (10.0 / 20_000.0)), math.ceil(math.log(1 / 0.01))
    assert vals[10:] == [width, depth, 10, 8, 10**9] == [5437, 5, 10, 8, 10**9]
    assert vals[10:] == [rc.WIDTH, rc.DEPTH, rc.LIMIT, rc.MAX_DEPTH, rc.PERIOD_NS]
    assert vals[10:] == [ratelimit.RATE_WIDTH, ratelimit.RATE_DEPTH, ratelimit.RATE_LIMIT, ratelimit.RATE_MAX_DEPTH,
                         ratelimit.RATE_PERIOD_NS]
    S, T = ratelimit.RateSeedStruct, ratelimit.RateTablesStruct
    assert (ctypes.sizeof(S), S.a.offset, S.b.offset) == (16, 0, 8) and ratelimit.SEED_BYTES == 16
    assert [ctypes.sizeof(T)] + [getattr(T, n).offset for n, _ in T._fields_] == vals[4:10]


# ------------------------------------------------------------ key and column
def _addr_with_key(key: int) -> bytes:
    """an rg_src_addr whose key is `key`: IPv4 below 2^32, else an IPv6 address with that /64"""
    if key <= M32:
        return key.to_bytes(4, "big") + bytes(12) + b"\x34\x12" + bytes(6)
    return key.to_bytes(8, "big") + bytes(range(1, 9)) + b"\x34\x12" + bytes(6)


def test_library_column_equals_the_models():
    keys = (0, 1, M32, 1 << 32, M64)
    seeds = ((0, 0), (M64, M64), (0, M64), (M64, 0))
    widths = (1, 2, 3, 5437, M32)
    n = 0
    for key in keys:
        a = _addr_with_key(key)
        assert rc.key_of(a) == key
        for seed in seeds:
            for w in widths:
                got, want = ratelimit.column(seed, a, w), rc.column(key, seed, w)
                assert got == want and 0 <= got < w, (key, seed, w, got, want)
                n += 1
    assert n == 100
    rng = np.random.default_rng(41)
    for _ in range(400):
        key = int(rng.integers(0, 1 << 64, dtype=np.uint64)) >> int(rng.integers(0, 64))
        seed = tuple(int(x) for x in rng.integers(0, 1 << 64, 2, dtype=np.uint64))
        w = max(1, int(rng.integers(0, 1 << 32, dtype=np.uint64)) >> int(rng.integers(0, 32)))
        a = _addr_with_key(key)
        assert ratelimit.column(seed, a, w) == rc.column(rc.key_of(a), seed, w) < w
    # the columns spread: 2000 keys over the default width under one seed hit well over a thousand buckets
    cols = {rc.column(k, (7, 9), rc.WIDTH) for k in range(2000)}
    assert len(cols) > 1500 and max(cols) < rc.WIDTH
    # and the hash is written out: fold of small numbers has no high half
    assert rc.fold(3, 5) == 15 and rc.fold(1 << 63, 4) == 2 and rc.fold(M64, M64) == 1 ^ (M64 - 1)


def test_key_derivation():
    seed = (0x0123456789ABCDEF, 0xFEDCBA9876543210)
    col = lambda a: ratelimit.column(seed, a, M32)  # noqa: E731
    # IPv4: the port and the pad bytes are not part of the key
    v4 = [rc.addr("192.0.2.7", p, pad) for p, pad in ((0, bytes(6)), (51820, bytes(6)), (65535, b"\xff" * 6))]
    assert {rc.key_of(a) for a in v4} == {0xC0000207} and len({col(a) for a in v4}) == 1
    # IPv6: a pair that differs only below the /64 has one key, a pair that differs in ip[7] has two
    a, b = rc.addr("2001:db8:1:2:3:4:5:6", 9), rc.addr("2001:db8:1:2:ffff:ffff:ffff:ffff", 10)
    c = rc.addr("2001:db8:1:3:3:4:5:6", 9)
    assert a[:8] == b[:8] and a[8:16] != b[8:16] and a[:7] == c[:7] and a[7] != c[7]
    assert rc.key_of(a) == rc.key_of(b) == 0x20010DB800010002 and rc.key_of(c) == 0x20010DB800010003
    assert col(a) == col(b) != col(c)
    # ip[4..16] == 0 is keyed as IPv4, whatever the family was; one nonzero byte anywhere behind it makes it a /64
    short = rc.addr("c000:207::", 1)
    assert short[:4] == v4[0][:4] and rc.key_of(short) == 0xC0000207 and col(short) == col(v4[0])
    for k in range(4, 16):
        other = bytearray(v4[0])
        other[k] = 1
        assert rc.key_of(bytes(other)) == int.from_bytes(other[:8], "big") != 0xC0000207, k
        assert col(bytes(other)) == rc.column(rc.key_of(bytes(other)), seed, M32), k
    assert rc.key_of(rc.addr("0.0.0.0")) == 0 == rc.key_of(rc.addr("::"))
    assert ratelimit.column(seed, rc.addr("::"), 1) == 0 and _lib.lib().rg_rate_column(None, None, 5) == 0


# ------------------------------------------- the model and the reference's tests
def test_model_against_the_reference_unit_tests():
    """rate_limiter.rs:206-217: five counts of one key return 1..5 on a 3 x 3 sketch and a reset returns to 1;
    estimate >= actual on the default sketch; and saturation"""
    rng = np.random.default_rng(3)
    s = rc.new_sketch(3, 3, rc.seeds_for(3, rng))
    assert [rc.count_one(s, 1234) for _ in range(5)] == [1, 2, 3, 4, 5]
    s, reset = rc.turn_loop(s, 10, 0, rc.seeds_for(3, rng))
    assert reset == 1 and rc.count_one(s, 1234) == 1
    s = rc.new_sketch(seeds=rc.seeds_for(rc.DEPTH, rng))
    keys = [rc.key_of(a) for a in rc.addresses("distinct", 1000, rng)]
    times = [int(x) for x in rng.integers(1, 10, 1000)]
    assert len(set(keys)) == 1000
    order = [k for k, t in zip(keys, times) for _ in range(t)]
    rng.shuffle(order)
    seen, last = {}, {}
    for k in order:
        seen[k] = seen.get(k, 0) + 1
        last[k] = rc.count_one(s, k)
        assert last[k] >= seen[k]
    assert all(last[k] >= t for k, t in zip(keys, times)) and sum(last[k] == t for k, t in zip(keys, times)) > 900
    s = rc.new_sketch(2, 2, [(1, 2), (3, 4)])
    s["buckets"] = [[M32 - 1, M32 - 1], [M32 - 1, M32 - 1]]
    assert [rc.count_one(s, 5) for _ in range(3)] == [M32, M32, M32]
    assert sorted(s["buckets"][0]) == sorted(s["buckets"][1]) == [M32 - 1, M32]


def test_model_count_loop_uncounted_messages_and_limit():
    rng = np.random.default_rng(8)
    desc, addrs, buf, skipped = rc.uncounted_case(rng)
    s0 = rc.start_sketch(3, 2, 1)
    s1, counts, flags = rc.count_loop(s0, desc, addrs, buf, 12)
    assert len(skipped) == 9 and all(counts[i] == 0 and flags[i] == 0 for i in skipped)
    assert [rc.counted(d, buf) for d in desc].count(False) == 9
    keep = [i for i in range(len(desc)) if i not in skipped]
    s2, counts2, flags2 = rc.count_loop(s0, [desc[i] for i in keep], [addrs[i] for i in keep], buf, 12)
    assert s2 == s1 and counts2 == [counts[i] for i in keep] and flags2 == [flags[i] for i in keep]
    assert 0 in flags2 and 1 in flags2 and all(f == (c > 12) for f, c in zip(flags, counts))
    assert sum(map(sum, s1["buckets"])) - sum(map(sum, s0["buckets"])) == 2 * len(keep)


# ---------------------------------------------------------------- workspace
def test_workspace_size_is_monotone_and_refuses_absurd_sizes():
    size = _lib.lib().rg_rate_workspace_size
    sizes = [0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 4099, 65536, 1 << 20, (1 << 29) - 1]
    widths = [1, 2, 3, 256, 257, 5437, 65536, 65537, 1 << 24, (1 << 24) + 1, (1 << 29) - 1]
    for d in range(1, 9):
        for w in widths:
            col = [size(n, w, d) for n in sizes]
            assert all(x <= y for x, y in zip(col, col[1:])) and col[0] >= 256, (w, d, col)
            assert all(c % 256 == 0 for c in col)
        for n in sizes:
            row = [size(n, w, d) for w in widths]
            assert all(x <= y for x, y in zip(row, row[1:])), (n, d, row)
    for n in sizes:
        for w in widths:
            col = [size(n, w, d) for d in range(1, 9)]
            assert all(x <= y for x, y in zip(col, col[1:])), (n, w, col)
    # out of range: the shape, n, n * depth, width * depth
    assert size(5, 0, 5) == 0 and size(5, 5437, 0) == 0 and size(5, 5437, 9) == 0
    assert size(1 << 32, 3, 1) == 0 and size((1 << 64) - 1, 3, 1) == 0 and size(M32, 3, 1) > 0
    assert size((1 << 31), 3, 2) == 0 and size((1 << 31) - 1, 3, 2) > 0 and size(M32 // 5 + 1, 5437, 5) == 0
    assert size(1, M32, 1) > 0 and size(1, M32, 2) == 0 and size(1, 1 << 31, 2) == 0 and size(1, (1 << 31) - 1, 2) > 0
    # three words an item (bucket word, count, estimate), two orders at the default size, one for 256 buckets or
    # fewer, none for a single bucket
    assert size(4099, 5437, 5) >= 4099 * 5 * 4 * 5 and size(4099, 1, 1) < size(4099, 256, 1) < size(4099, 257, 1)


# ------------------------------------------------------------------ refusals
class Args:
    """A set of arguments every rule accepts, as plain addresses that nothing may dereference: the context is a block
    whose device ordinal no machine has, so a call that got past its argument rules ends in RG_EDEVICE at
    hipSetDevice, with nothing enqueued, and every refusal below is the work of the one thing changed."""

    N, WIDTH, DEPTH = 9, 257, 3

    def __init__(self):
        self.ctx = ctypes.create_string_buffer(1 << 16)
        ctypes.memmove(self.ctx, (ctypes.c_int * 1)(0x3FFFFFF0), 4)  # rg_ctx.device
        self.need = int(_lib.lib().rg_rate_workspace_size(self.N, self.WIDTH, self.DEPTH))
        self.t = ratelimit.RateTablesStruct(buckets=0x10000, seeds=0x20000, last_reset_ns=0x30000, width=self.WIDTH,
                                            depth=self.DEPTH)
        self.desc, self.addrs, self.buf, self.counts, self.flags, self.ws = 0x40000, 0x50000, 0x60000, 0x70000, 0x80000, 0x90000
        self.now, self.new_seeds, self.reset = 0xA0000, 0xB0000, 0xC0000

    def count(self, ctx="ctx", tables="t", desc=None, addrs=None, n=None, buf=None, counts=None, flags=None, ws=None,
              wl=None, **fields):
        d = lambda v, x: x if v is None else (None if v == 0 else v)  # noqa: E731
        return _lib.lib().rg_rate_count_batch_dev(
            self._ctx(ctx), self._tables(tables, fields), d(desc, self.desc), d(addrs, self.addrs),
            self.N if n is None else n, d(buf, self.buf), 4096, 10, d(counts, self.counts), d(flags, self.flags),
            d(ws, self.ws), self.need if wl is None else wl, None)

    def turn(self, ctx="ctx", tables="t", now=None, new_seeds=None, reset=None, period=10**9, **fields):
        d = lambda v, x: x if v is None else (None if v == 0 else v)  # noqa: E731
        return _lib.lib().rg_rate_turn_dev(self._ctx(ctx), self._tables(tables, fields), d(now, self.now), period,
                                           d(new_seeds, self.new_seeds), d(reset, self.reset), None)

    def _ctx(self, ctx):
        return ctypes.cast(self.ctx, ctypes.c_void_p) if ctx == "ctx" else None

    def _tables(self, tables, fields):
        if tables is None:
            return None
        t = ratelimit.RateTablesStruct.from_buffer_copy(self.t)
        for k, v in fields.items():
            setattr(t, k, v)
        return ctypes.byref(t)


TABLE_RULES = (dict(tables=None), dict(buckets=0), dict(seeds=0), dict(last_reset_ns=0),  # a null required pointer
               dict(seeds=0x20001), dict(seeds=0x20008),                                   # seeds: 16 bytes
               dict(last_reset_ns=0x30001), dict(last_reset_ns=0x30004),                   # last_reset_ns: 8
               dict(buckets=0x10001), dict(buckets=0x10002),                               # words: 4
               dict(depth=0), dict(depth=9), dict(depth=M32), dict(width=0),               # the shape
               dict(width=M32, depth=2), dict(width=1 << 31, depth=2))                     # width * depth above 2^32 - 1


def _refused(call, name, bad):
    assert call(**bad) == EINVAL, (name, bad)
    assert name in _lib.lib().rg_last_error(), (name, bad, _lib.lib().rg_last_error())


def test_every_argument_rule_is_answered_before_the_device_is_touched():
    a = Args()
    # the arguments as they stand pass every rule: the calls get as far as selecting the device
    assert a.count() == EDEVICE and a.turn() == EDEVICE
    assert a.count(wl=a.need + 1) == EDEVICE and a.turn(period=0) == EDEVICE and a.turn(period=M64) == EDEVICE
    assert a.count(depth=8, wl=1 << 30) == EDEVICE and a.count(width=1, depth=1) == EDEVICE
    # the optional array, and a size of zero
    assert a.count(counts=0) == EDEVICE and a.count(n=0) == 0 and a.count(n=0, tables=None, ws=0) == 0
    # a null context, whatever else
    assert a.count(ctx=None) == EINVAL and a.turn(ctx=None) == EINVAL and a.count(ctx=None, n=0) == EINVAL
    for bad in TABLE_RULES:
        _refused(a.count, b"rate count", bad)
        _refused(a.turn, b"rate turn", bad)
    for bad in (dict(desc=0), dict(addrs=0), dict(buf=0), dict(flags=0), dict(ws=0),  # a null required pointer
                dict(n=1 << 32), dict(n=(1 << 64) - 1),                                # a count above 2^32 - 1
                dict(n=M32 // 3 + 1, wl=1 << 62), dict(n=M32, wl=1 << 62),             # ... n * depth
                dict(addrs=a.addrs + 1), dict(addrs=a.addrs + 4),                      # rg_src_addr rows: 8 bytes
                dict(counts=a.counts + 1), dict(counts=a.counts + 2),                  # words: 4
                dict(ws=a.ws + 1), dict(ws=a.ws + 8),                                  # the workspace: 16
                dict(wl=a.need - 1), dict(wl=0), dict(n=4099)):                        # a short workspace
        _refused(a.count, b"rate count", bad)
    assert a.count(n=M32 // 3, wl=1 << 62) == EDEVICE  # n * depth == 2^32 - 1 is in range
    for bad in (dict(now=0), dict(new_seeds=0), dict(reset=0),
                dict(now=a.now + 1), dict(now=a.now + 4),
                dict(new_seeds=a.new_seeds + 1), dict(new_seeds=a.new_seeds + 8),
                dict(reset=a.reset + 1), dict(reset=a.reset + 2)):
        _refused(a.turn, b"rate turn", bad)


# ----------------------------------------------------------------- the turn
def test_model_turn_one_case_per_line():
    rng = np.random.default_rng(12)
    old, new = rc.seeds_for(2, rng), rc.seeds_for(2, rng)
    s = rc.new_sketch(3, 2, old)
    s["buckets"], s["last_reset_ns"] = [[1, 2, 3], [4, 5, M32]], 1000
    P = rc.PERIOD_NS
    wiped = {"buckets": [[0] * 3] * 2, "seeds": new}
    for now, period, reset in ((1000, P, 0),          # now == last
                               (1000, 0, 0),          # ... even with no period
                               (999, P, 0),           # now < last
                               (0, 0, 0),
                               (1000 + P, P, 0),      # now - last == period
                               (1000 + P + 1, P, 1),  # now - last == period + 1
                               (1001, 0, 1),          # period = 0: whenever the clock moved
                               (M64, M64 - 1000, 0), (M64, M64 - 1001, 1)):  # the far end of the clock
        got, flag = rc.turn_loop(s, now, period, new)
        assert flag == reset, (now, period)
        assert got == ({**wiped, "last_reset_ns": now} if reset else s), (now, period)
    # a sketch that starts at 0 resets on its first turn, and not again at the same clock
    s0 = rc.new_sketch(3, 2, old)
    s1, flag = rc.turn_loop(s0, 7, P, new)
    assert flag == 0 and s1 == s0
    s1, flag = rc.turn_loop(s0, P + 1, P, new)
    assert flag == 1 and s1["last_reset_ns"] == P + 1 and rc.turn_loop(s1, P + 1, P, old) == (s1, 0)


def test_cases_cover_what_they_claim():
    """the size cases' inputs: at n >= 2047 the model puts messages on both sides of the limit for every shape and
    address list; three addresses' messages lie on both sides of a wave edge and of a tile edge of the item space;
    (257, 3) needs a second radix pass and (1, 1) none"""
    assert [w * d for w, d in rc.SHAPES] == [1, 6, 771, 27185]
    for n in (2047, 2049, 4099):
        for shape in rc.SHAPES:
            for kind in rc.KINDS:
                s, desc, addrs, buf = rc.size_case(n, shape, kind)
                assert all(rc.counted(d, buf) for d in desc)
                assert all(1 <= b <= 16 for row in s["buckets"] for b in row)
                after, counts, flags = rc.count_loop(s, desc, addrs, buf)
                assert 0 < sum(flags) < n, (n, shape, kind, sum(flags))
                keys = [rc.key_of(a) for a in addrs]
                assert len(set(keys)) == {"one": 1, "three": 3, "distinct": n}[kind]
                if kind == "three":
                    d = shape[1]
                    for edge in (64, rc.TILE):  # an item edge inside the batch: message edge // d and its neighbours
                        m = edge // d
                        assert m < n or (n, d, edge) == (2047, 1, rc.TILE)  # 2047 items: one tile
                        assert set(keys[m:m + 3]) <= set(keys[m - 3:m])
    desc, addrs, buf, skipped = rc.uncounted_case(np.random.default_rng(1))
    assert all(addrs[i] == addrs[0] for i in skipped) and all(rc.counted(desc[i - 1], buf) for i in skipped)
    assert all(rc.counted(desc[i + 1], buf) and addrs[i + 1] == addrs[0] for i in skipped)
