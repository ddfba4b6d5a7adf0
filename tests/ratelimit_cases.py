"""The device-resident handshake rate limiter's model and cases, shared by test_ratelimit_cpu.py and
test_gpu_ratelimit.py.

`count_loop` and `turn_loop` are the sequential loops of include/rg_aead.h ("device-resident handshake rate
limiter") over plain Python lists, `key_of` and `column` the key and the column as the header writes them out; they
are the only source of expected values.  A sketch is a dict: buckets (depth lists of width ints), seeds (depth pairs
(a, b)) and last_reset_ns."""
import ipaddress

import numpy as np

M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
KEY_SKIP = 0xFFFFFFFF
WIDTH, DEPTH, LIMIT, MAX_DEPTH = 5437, 5, 10, 8
PERIOD_NS = 10**9
TILE = 2048
INIT_LEN, RESP_LEN = 148, 92
K1, K2 = 0x9E3779B97F4A7C15, 0xD6E8FEB86659FD93


# ------------------------------------------------------------ key and column
def addr(ip: str, port: int = 0, pad: bytes = bytes(6)) -> bytes:
    """one rg_src_addr row: the address's octets at the front of 16 bytes, the port little-endian, 6 pad bytes"""
    return ipaddress.ip_address(ip).packed.ljust(16, b"\0") + port.to_bytes(2, "little") + pad


def key_of(a: bytes) -> int:
    """lib.rs:509-512 over rg_src_addr: ip[4..16] all zero is IPv4, keyed by the big-endian u32 of ip[0..4]; every
    other address by its /64, the big-endian u64 of ip[0..8]"""
    if a[4:16] == bytes(12):
        return int.from_bytes(a[0:4], "big")
    return int.from_bytes(a[0:8], "big")


def fold(x: int, y: int) -> int:
    p = x * y
    return (p & M64) ^ (p >> 64)


def column(key: int, seed, width: int) -> int:
    h = fold(fold(key ^ seed[0], K1) ^ seed[1], K2)
    return ((h >> 32) * width) >> 32


# ---------------------------------------------------------------- the loops
def new_sketch(width=WIDTH, depth=DEPTH, seeds=None):
    return {"buckets": [[0] * width for _ in range(depth)], "seeds": list(seeds or [(0, 0)] * depth), "last_reset_ns": 0}


def copy_sketch(s):
    return {"buckets": [list(r) for r in s["buckets"]], "seeds": list(s["seeds"]), "last_reset_ns": s["last_reset_ns"]}


def counted(d, buf: bytes) -> bool:
    """the filter would go on to read this message's MACs; d = (offset, len, key_idx)"""
    off, ln, key_idx = d
    if off % 16 or off > len(buf) or ln > len(buf) - off or ln not in (INIT_LEN, RESP_LEN) or key_idx == KEY_SKIP:
        return False
    return int.from_bytes(buf[off:off + 4], "little") == (1 if ln == INIT_LEN else 2)


def count_one(s, key: int) -> int:
    """CountMinSketch::count with saturating buckets: bump the key's bucket in every row, return the minimum"""
    width, est = len(s["buckets"][0]), M32
    for row, seed in zip(s["buckets"], s["seeds"]):
        c = column(key, seed, width)
        row[c] = min(row[c] + 1, M32)
        est = min(est, row[c])
    return est


def count_loop(s, desc, addrs, buf: bytes, limit=LIMIT):
    """-> (the sketch after, counts_out, overload_out)"""
    s = copy_sketch(s)
    counts, flags = [], []
    for d, a in zip(desc, addrs):
        est = count_one(s, key_of(a)) if counted(d, buf) else 0
        counts.append(est)
        flags.append(1 if est > limit else 0)
    return s, counts, flags


def turn_loop(s, now: int, period: int, new_seeds):
    """-> (the sketch after, reset_out)"""
    s = copy_sketch(s)
    last = s["last_reset_ns"]
    if now > last and now - last > period:
        s["buckets"] = [[0] * len(r) for r in s["buckets"]]
        s["seeds"] = list(new_seeds)
        s["last_reset_ns"] = now
        return s, 1
    return s, 0


# -------------------------------------------------------------------- cases
# (width, depth): one bucket for everything, heavy collisions, a bucket range that needs a second radix pass (771
# buckets), the default
SHAPES = ((1, 1), (3, 2), (257, 3), (WIDTH, DEPTH))
SIZES = (1, 63, 64, 65, 2047, 2049, 4099)
KINDS = ("one", "three", "distinct")
# Two frames every descriptor of the size cases points at (buf is never written, so frames may be shared): an
# initiation at 0 and a response at 160, in a buffer of 320 bytes.
FRAMES_LEN = 320


def frames(rng) -> bytes:
    b = bytearray(rng.integers(0, 256, FRAMES_LEN, dtype=np.uint8).tobytes())
    b[0:4], b[160:164] = (1).to_bytes(4, "little"), (2).to_bytes(4, "little")
    return bytes(b)


def descs(n):
    """initiations and responses in turn, all counted; key_idx is anything but RG_KEY_SKIP"""
    return [((0, INIT_LEN, i) if i % 2 == 0 else (160, RESP_LEN, 7)) for i in range(n)]


def seeds_for(depth, rng):
    return [(int(a), int(b)) for a, b in rng.integers(0, 1 << 64, (depth, 2), dtype=np.uint64)]


def start_sketch(width, depth, seed):
    """random seeds, random nonzero buckets (1..16, so that estimates start on both sides of the default limit)"""
    rng = np.random.default_rng(seed)
    s = new_sketch(width, depth, seeds_for(depth, rng))
    s["buckets"] = [[int(x) for x in rng.integers(1, 17, width)] for _ in range(depth)]
    s["last_reset_ns"] = 5
    return s


def addresses(kind, n, rng):
    """one: one IPv4 address under changing ports.  three: an IPv4 and two IPv6 addresses in turn, so that one
    address's messages lie on both sides of every wave and tile edge, the IPv6 ones with changing low halves.
    distinct: n different keys, IPv4 and IPv6 /64s in turn."""
    out = []
    for i in range(n):
        port = int(rng.integers(0, 65536))
        if kind == "one":
            a = addr("198.51.100.9", port)
        elif kind == "three":
            low = ":".join(f"{int(x):x}" for x in rng.integers(0, 65536, 4))
            a = (addr("203.0.113.77", port), addr(f"2001:db8:0:5:{low}", port), addr(f"2001:db8:0:6:{low}", port))[i % 3]
        else:
            a = addr(f"10.{i >> 16 & 255}.{i >> 8 & 255}.{i & 255}", port) if i % 2 else \
                addr(f"2001:db8:{i >> 16:x}:{i & 0xFFFF:x}::{port:x}", port)
        out.append(a)
    return out


def size_case(n, shape, kind):
    """-> (start sketch, desc, addrs, buf) of one size case; the start depends on the shape alone.  (Its seed is one
    under which every case of n >= 2047 has messages on both sides of the default limit: a small sketch can start
    with every bucket of an address above it.  test_ratelimit_cpu.py checks that on the model.)"""
    width, depth = shape
    rng = np.random.default_rng([n, width, depth, KINDS.index(kind)])
    return start_sketch(width, depth, 3 + 4 * width + depth), descs(n), addresses(kind, n, rng), frames(rng)


def uncounted_case(rng):
    """-> (desc, addrs, buf, the indices of the uncounted messages): counted messages of two addresses, and between
    those of the first each way a message is not counted, from that address"""
    buf = frames(rng)
    a, b = addr("192.0.2.1", 1), addr("2001:db8::1", 2)
    ok_i, ok_r = (0, INIT_LEN, 0), (160, RESP_LEN, 0)
    skips = [(8, INIT_LEN, 0),            # unaligned
             (176, INIT_LEN, 0),          # runs 4 bytes past buf_len
             (FRAMES_LEN, RESP_LEN, 0),   # starts at buf_len
             (FRAMES_LEN + 16, 0, 0),     # starts past it
             (0, 147, 0),                 # no handshake length
             (0, RESP_LEN, 0),            # type word 1 under a response's length
             (160, INIT_LEN, 0),          # type word 2 under an initiation's
             (0, INIT_LEN, KEY_SKIP),     # RG_KEY_SKIP
             (160, RESP_LEN, KEY_SKIP)]
    desc, addrs, skipped = [ok_i, ok_r], [a, b], []
    for k, d in enumerate(skips):
        skipped.append(len(desc))
        desc += [d, ok_r if k % 2 else ok_i, ok_i]
        addrs += [a, a, b]
    return desc, addrs, buf, skipped
