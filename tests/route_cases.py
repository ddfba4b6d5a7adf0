"""Cases shared by the cryptokey-routing tests (test_route_cpu.py, test_gpu_route.py).

The yardstick is `brute`: longest-prefix match by trying every prefix, written here in Python and sharing
nothing with csrc/rg_route.h.  `route_model` and `check_model` restate the per-packet rules of include/rg_aead.h
("device-resident cryptokey routing") over plain Python integers; they are the only source of expected values.

A table case is (name, rows): rows a list of (address as a 32-bit integer -- host bits below the prefix length
may be set --, prefix length, peer)."""
import numpy as np

OK, ERR, INVALID, REJECTED, UNALIGNED, NOT_DATA, PENDING, COOKIE, KEYEXCHANGE, UNROUTABLE = range(10)
SKIP = 0xFFFFFFFF
NONE = 0xFFFFFFFF
DESC_DTYPE = np.dtype([("offset", np.uint64), ("len", np.uint32), ("key_idx", np.uint32)])

PREFIX_LENGTHS = (0, 1, 15, 16, 17, 23, 24, 25, 31, 32)  # both sides of each stride boundary
INNER_LENGTHS = (0, 19, 20, 21, 31, 32, 33, 1499, 1500)
BATCH_SIZES = (1, 63, 64, 65, 257)  # 257: one packet past a workgroup


def ip(a, b, c, d):
    return a << 24 | b << 16 | c << 8 | d


def mask(plen):
    return (0xFFFFFFFF << (32 - plen)) & 0xFFFFFFFF if plen else 0


def brute(rows, addrs):
    """Longest-prefix match of every address (uint32 array) against every row, in array order: a later row wins
    over an earlier one of the same length.  -> uint32 array, NONE where nothing matches."""
    addrs = np.asarray(addrs, np.uint32)
    best_len = np.full(len(addrs), -1, np.int64)
    best = np.full(len(addrs), NONE, np.uint32)
    for net, plen, peer in rows:
        m = np.uint32(mask(plen))
        hit = ((addrs & m) == (np.uint32(net) & m)) & (plen >= best_len)
        best_len[hit] = plen
        best[hit] = peer
    return best


def probes(rows):
    """For every prefix its first address, its last, the one just before and the one just after (mod 2^32)."""
    out = []
    for net, plen, _ in rows:
        first = net & mask(plen)
        last = first | (~mask(plen) & 0xFFFFFFFF)
        out += [first, last, (first - 1) & 0xFFFFFFFF, (last + 1) & 0xFFFFFFFF]
    out += [0, 0xFFFFFFFF, ip(127, 0, 0, 1)]
    return np.array(sorted(set(out)), np.uint32)


def _strides():
    """One prefix of every length of PREFIX_LENGTHS in a region of its own (above a /1), host bits set."""
    rows = [(0, 0, 0), (ip(128, 0, 0, 0), 1, 1)]
    for k, plen in enumerate(PREFIX_LENGTHS[2:]):
        rows.append((ip(130 + 4 * k, 77, 201, 0xA5), plen, 2 + k))  # host bits below plen are set: masked
    return rows


def _nested():
    """Prefixes inside prefixes across both stride boundaries, siblings, and a prefix given twice."""
    return [
        (ip(10, 0, 0, 0), 8, 1), (ip(10, 0, 0, 0), 15, 6), (ip(10, 1, 0, 0), 16, 2), (ip(10, 1, 128, 0), 17, 8),
        (ip(10, 1, 2, 0), 23, 7), (ip(10, 1, 2, 0), 24, 3), (ip(10, 1, 3, 0), 24, 13),  # siblings under the /23
        (ip(10, 1, 2, 0), 25, 10), (ip(10, 1, 2, 128), 25, 4),  # siblings under the /24
        (ip(10, 1, 2, 200), 32, 5), (ip(10, 1, 2, 201), 32, 15), (ip(10, 1, 2, 254), 31, 9),
        (ip(10, 1, 2, 77), 24, 11),  # the /24 again with host bits set and another peer: the last row wins
        (ip(10, 1, 2, 200), 32, 12),  # the /32 again
        (ip(10, 1, 2, 128), 25, 14),  # the /25 again
        (ip(10, 200, 0, 9), 32, 16),  # a /32 straight under the /8: two new blocks for one address
        (ip(192, 168, 0, 0), 16, 17), (ip(192, 168, 255, 255), 32, 18), (ip(192, 169, 0, 0), 32, 19),
    ]


def _random(nrows, seed, npeers):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(nrows):
        plen = int(rng.choice(PREFIX_LENGTHS[2:] + (8, 12, 20, 28)))
        # a few /16 regions, so that prefixes nest and share blocks
        net = ip(int(rng.choice((10, 10, 172, 192))), int(rng.integers(0, 4)), int(rng.integers(0, 256)),
                 int(rng.integers(0, 256)))
        rows.append((net, plen, int(rng.integers(0, npeers))))
    rows += rows[:5]  # given twice ...
    rows += [(net, plen, (peer + 1) % npeers) for net, plen, peer in rows[5:10]]  # ... and with another peer
    return rows


def table_cases():
    return [
        ("empty", []),
        ("default_only", [(ip(1, 2, 3, 4), 0, 7)]),
        ("strides", _strides()),
        ("nested", _nested()),
        ("default_and_nested", [(0, 0, 20)] + _nested()),
        ("max_peer", [(ip(9, 9, 9, 9), 32, 0x7FFFFFFF), (ip(9, 9, 0, 0), 16, 0), (ip(0, 0, 0, 0), 32, 3),
                      (ip(255, 255, 255, 255), 32, 4), (ip(255, 255, 255, 254), 31, 5)]),
        ("random_256", _random(246, 7, 40)),
    ]


def prefix_rows(rows):
    """rows -> rg_route_prefix records (12 bytes: addr[4] in network order, prefix_len, peer)."""
    dt = np.dtype([("addr", np.uint8, 4), ("prefix_len", np.uint32), ("peer", np.uint32)])
    out = np.zeros(len(rows), dt)
    for i, (net, plen, peer) in enumerate(rows):
        out[i] = (np.frombuffer(int(net).to_bytes(4, "big"), np.uint8), plen, peer)
    return out


def expected_words(rows):
    """The table's exact size from the rows alone: the root, one block per /16 network that holds a prefix longer
    than 16, one per /24 network that holds a prefix longer than 24."""
    mid = {(net & mask(plen)) >> 16 for net, plen, _ in rows if plen > 16}
    low = {(net & mask(plen)) >> 8 for net, plen, _ in rows if plen > 24}
    return 65536 + 256 * (len(mid) + len(low))


# ------------------------------------------------------------------ packets
def ipv4(L, src, dst, rng, total=None, ihl=5, version=4):
    """An inner packet of L bytes: random bytes under an IPv4 header's fixed fields (as far as L reaches)."""
    pkt = rng.integers(1, 256, L, dtype=np.uint8)  # no zero byte: zeroed padding shows
    hdr = bytes([version << 4 | ihl, 0]) + int(L if total is None else total).to_bytes(2, "big")
    hdr += bytes(rng.integers(0, 256, 8, dtype=np.uint8)) + int(src).to_bytes(4, "big") + int(dst).to_bytes(4, "big")
    k = min(L, 20)
    pkt[:k] = np.frombuffer(hdr[:k], np.uint8)
    return pkt


def acceptable(pkt):
    """The IPv4 acceptance rule -> total_length, or 0."""
    L = len(pkt)
    if L < 20:
        return 0
    version, hdr = int(pkt[0]) >> 4, (int(pkt[0]) & 15) * 4
    total = int(pkt[2]) << 8 | int(pkt[3])
    return total if version == 4 and 20 <= hdr <= total <= L else 0


def roundup16(x):
    return (x + 15) // 16 * 16


def route_model(rows, peer_slot, desc, buf):
    """rg_route_batch_dev over plain integers -> (peers, slots, desc_out, status, buf')."""
    n, out = len(desc), buf.copy()
    peers, slots = np.full(n, NONE, np.uint32), np.full(n, SKIP, np.uint32)
    desc_out, status = desc.copy(), np.zeros(n, np.uint8)
    desc_out["key_idx"] = SKIP
    for i in range(n):
        off, L = int(desc["offset"][i]), int(desc["len"][i])
        if off % 16:
            status[i] = UNALIGNED
            continue
        if off + 16 + roundup16(L) + 16 > len(buf):
            status[i] = INVALID
            continue
        pkt = buf[off + 16:off + 16 + L]
        if not acceptable(pkt):
            status[i] = INVALID
            continue
        peer = int(brute(rows, [int.from_bytes(bytes(pkt[16:20]), "big")])[0])
        if peer == NONE or peer >= len(peer_slot):
            status[i] = UNROUTABLE
            continue
        peers[i] = peer
        if int(peer_slot[peer]) == SKIP:
            status[i] = REJECTED
            continue
        out[off + 16 + L:off + 16 + roundup16(L)] = 0
        slots[i] = peer_slot[peer]
        desc_out[i] = (off, roundup16(L), peer_slot[peer])
    return peers, slots, desc_out, status, out


def check_model(rows, slot_peer, desc, key_idx, buf, status):
    """rg_route_check_batch_dev over plain integers -> (status', inner_len)."""
    st, inner = np.array(status, np.uint8).copy(), np.zeros(len(desc), np.uint32)
    for i in range(len(desc)):
        if st[i] != OK:
            continue
        off, W = int(desc["offset"][i]), int(desc["len"][i])
        if W == 32:
            continue
        pkt = buf[off + 16:off + W - 16]
        total = acceptable(pkt) if W >= 32 else 0
        if not total:
            st[i] = INVALID
            continue
        peer = int(brute(rows, [int.from_bytes(bytes(pkt[12:16]), "big")])[0])
        k = int(key_idx[i])
        if peer == NONE or k >= len(slot_peer) or int(slot_peer[k]) != peer:
            st[i] = UNROUTABLE
            continue
        inner[i] = total
    return st, inner


# The routing scenario of the packet tests: the "nested" table; peers 0 .. NPEERS - 1, of which peer 9 has no
# session and peers >= NPEERS do not exist (peer 16 and above: the table names them, peer_slot does not).
NPEERS = 16
NKEYS = 5
ROWS = _nested()
NO_SESSION = 9


def peer_slots():
    """peer -> key row: peers share the NKEYS rows round robin, peer NO_SESSION has none."""
    slot = (np.arange(NPEERS) % NKEYS).astype(np.uint32)
    slot[NO_SESSION] = SKIP
    return slot


# destinations by what the scenario does with them
DST_OK = (ip(10, 1, 2, 5), ip(10, 1, 2, 129), ip(10, 1, 2, 200), ip(10, 1, 3, 9), ip(10, 9, 9, 9), ip(10, 1, 200, 1))
DST_NO_SESSION = (ip(10, 1, 2, 254), ip(10, 1, 2, 255))  # peer 9
DST_NONE = (ip(11, 0, 0, 1), ip(9, 255, 255, 255))  # no prefix
DST_BEYOND = (ip(10, 200, 0, 9), ip(192, 168, 1, 1))  # peers 16 and 17: >= NPEERS


def send_batch(n, seed):
    """n inner packets in frames with headroom: every inner length of INNER_LENGTHS, and every verdict class once
    n >= 63.  -> (desc with the unpadded lengths, buf, kinds) -- kinds is what each packet was made to be."""
    rng = np.random.default_rng(seed)
    kinds_cycle = ["ok"] * 9 + ["short", "ok", "version", "ok", "ihl", "ok", "total_long", "ok", "total_short", "ok",
                                "unaligned", "ok", "outside", "none", "ok", "beyond", "no_session", "ok"]
    desc = np.zeros(n, DESC_DTYPE)
    kinds, pkts, off = [], [], 0
    for i in range(n):
        kind = kinds_cycle[i % len(kinds_cycle)]
        L = INNER_LENGTHS[2:][i % 7] if i < 63 else int(rng.choice((20, 21, 40, 47, 48, 576, 1280, 1499, 1500)))
        dst = DST_OK[i % len(DST_OK)]
        kw = {}
        if kind == "short":
            L = (0, 19)[(i // len(kinds_cycle)) % 2]
        elif kind == "version":
            kw = {"version": 6}
        elif kind == "ihl":
            kw = {"ihl": 4}
        elif kind == "total_long":
            kw = {"total": L + 1}
        elif kind == "total_short":
            kw = {"total": 23, "ihl": 6}
        elif kind == "none":
            dst = DST_NONE[i % 2]
        elif kind == "beyond":
            dst = DST_BEYOND[i % 2]
        elif kind == "no_session":
            dst = DST_NO_SESSION[i % 2]
        elif kind == "ok" and L >= 60 and i % 3 == 0:
            kw = {"ihl": 15, "total": 60 + (L - 60) // 2}  # options; a total_length short of L
        pkts.append(ipv4(L, ip(10, 1, 2, 1), dst, rng, **kw))
        desc[i] = (off + (8 if kind == "unaligned" else 0), L, 0xABCD)  # key_idx is ignored
        off += 16 + roundup16(L) + 16 + 16
        kinds.append(kind)
    buf = rng.integers(1, 256, off + 64, dtype=np.uint8)
    for d, p in zip(desc, pkts):
        o = int(d["offset"]) + 16
        buf[o:o + len(p)] = p
    for i, kind in enumerate(kinds):
        if kind == "outside":  # the padded frame ends one chunk past the buffer
            desc["offset"][i] = (len(buf) - (16 + roundup16(int(desc["len"][i])) + 16) + 16) // 16 * 16
    return desc, buf, kinds


def recv_inner(n, seed):
    """Inner packets for the receive test, already padded as a sender pads them: (session, padded packet, kind).
    Session s is peer SRC_PEER[s]; 'own' sources belong to it, 'other' to another peer, 'none' to nobody."""
    rng = np.random.default_rng(seed)
    out = []
    cycle = ["own", "own", "other", "own", "none", "keepalive", "own", "not_ip", "own", "short_total", "own"]
    for i in range(n):
        kind = cycle[i % len(cycle)]
        s = i % len(SRC_PEER)
        peer = SRC_PEER[s]
        L = (20, 21, 31, 32, 33, 1499, 1500, 47)[i % 8]
        if kind == "keepalive":
            out.append((s, np.zeros(0, np.uint8), kind))
            continue
        src = {"own": SRC_OF[peer], "other": SRC_OF[SRC_PEER[(s + 1) % len(SRC_PEER)]], "none": ip(11, 0, 0, 1)}.get(
            kind, SRC_OF[peer])
        total = None
        if kind == "short_total":
            total = 19
        elif i % 4 == 0:
            total = max(20, L - 3)
        pkt = ipv4(L, src, ip(10, 1, 2, 1), rng, total=total, version=6 if kind == "not_ip" else 4)
        out.append((s, np.concatenate([pkt, np.zeros(roundup16(L) - L, np.uint8)]), kind))
    return out


SRC_PEER = (1, 2, 10)  # session (key row) -> peer, for the receive tests
SRC_OF = {1: ip(10, 77, 0, 1), 2: ip(10, 1, 5, 5), 10: ip(10, 1, 2, 99)}  # an address of each peer's own
