"""The in-order model of the inbound demultiplexer (include/rg_aead.h, "device-resident inbound demultiplexer") and the
builders of the mixed batches the CPU and GPU tests share.  demux_loop and verdict_loop are the header's loops written
out, one datagram at a time; demux_model and verdict_model compute the same arrays with numpy for the large batches
(tests/test_demux_cpu.py holds the two against each other)."""
import numpy as np

OK, DECRYPT_ERR, INVALID, REJECTED, UNALIGNED, NOT_DATA, PENDING, COOKIE, FULL = 0, 1, 2, 3, 4, 5, 6, 7, 10
SKIP = 0xFFFFFFFF
DESC, ADDR = 16, 24  # rg_pkt_desc, rg_src_addr
INIT_LEN, RESP_LEN, COOKIE_LEN = 148, 92, 64
TILE = 2048  # kGroupTile

DESC_DTYPE = np.dtype([("offset", "<u8"), ("len", "<u4"), ("key_idx", "<u4")])
INERT = np.array([(0, 0, SKIP)], DESC_DTYPE)[0]
LISTS = ("hs", "ck", "data")


def list_of(cls: int):
    return {1: "hs", 2: "hs", 3: "ck", 4: "data"}.get(cls)


def classify(d, buf) -> tuple[int, int]:
    """one datagram -> (class 1-4 and PENDING, or 0 and its verdict): the header's rules in the header's order"""
    off, ln, key = int(d["offset"]), int(d["len"]), int(d["key_idx"])
    if key == SKIP:
        return 0, REJECTED
    if off % 16:
        return 0, UNALIGNED
    if ln < 4 or off + ln > len(buf):  # Python integers: 64 bits and more, no wrap
        return 0, INVALID
    t = int.from_bytes(bytes(buf[off:off + 4]), "little")
    want = {1: INIT_LEN, 2: RESP_LEN, 3: COOKIE_LEN}
    if t in want:
        return (t, PENDING) if ln == want[t] else (0, INVALID)
    return (4, PENDING) if t == 4 else (0, INVALID)


def empty_lists(caps):
    """every list all inert"""
    out = {}
    for name, cap in zip(LISTS, caps):
        out[name + "_desc"] = np.full(cap, INERT, DESC_DTYPE)
    for name in ("init_desc", "resp_desc"):
        out[name] = np.full(caps[0], INERT, DESC_DTYPE)
    out["hs_addrs"] = np.zeros((caps[0], ADDR), np.uint8)
    out["data_addrs"] = np.zeros((caps[2], ADDR), np.uint8)
    return out


def demux_loop(desc, addrs, buf, caps):
    """the header's loop -> dict(status, cls, pos, counts, hs_desc, hs_addrs, init_desc, resp_desc, ck_desc, data_desc,
    data_addrs); caps = (cap_hs, cap_ck, cap_data)"""
    n = len(desc)
    cap = dict(zip(LISTS, caps))
    rank, seen = dict.fromkeys(LISTS, 0), dict.fromkeys(LISTS, 0)
    out = empty_lists(caps)
    status, cls, pos = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.full(n, SKIP, np.uint32)
    for i in range(n):
        c, st = classify(desc[i], buf)
        L = list_of(c)
        if L is not None:
            seen[L] += 1
            k = rank[L]
            cls[i] = c
            if k < cap[L]:
                rank[L] += 1
                row = (int(desc[i]["offset"]), int(desc[i]["len"]), 0)
                out[L + "_desc"][k] = row
                if L == "hs":
                    out["init_desc" if c == 1 else "resp_desc"][k] = row
                if L != "ck":
                    out[L + "_addrs"][k, :18] = addrs[i, :18]
                pos[i] = k
            else:
                st = FULL
        status[i] = st
    out.update(status=status, cls=cls, pos=pos,
               counts=np.array([rank[L] for L in LISTS] + [seen[L] for L in LISTS], np.uint32))
    return out


def demux_model(desc, addrs, buf, caps):
    """demux_loop with numpy"""
    n, buf_len = len(desc), len(buf)
    off, ln, key = desc["offset"], desc["len"], desc["key_idx"]
    skip = key == SKIP
    unal = ~skip & ((off & np.uint64(15)) != 0)
    room = np.where(off <= buf_len, np.uint64(buf_len) - np.minimum(off, np.uint64(buf_len)), np.uint64(0))
    inb = ~skip & ~unal & (ln >= 4) & (off <= buf_len) & (ln.astype(np.uint64) <= room)
    at = off[inb].astype(np.int64)
    t = np.zeros(n, np.uint32)
    padded = np.concatenate([np.asarray(buf, np.uint8), np.zeros(4, np.uint8)]).astype(np.uint32)
    t[inb] = padded[at] | (padded[at + 1] << 8) | (padded[at + 2] << 16) | (padded[at + 3] << 24)
    cls = np.zeros(n, np.uint8)
    cls[inb & (t == 1) & (ln == INIT_LEN)] = 1
    cls[inb & (t == 2) & (ln == RESP_LEN)] = 2
    cls[inb & (t == 3) & (ln == COOKIE_LEN)] = 3
    cls[inb & (t == 4)] = 4
    status = np.full(n, INVALID, np.uint8)
    status[skip], status[unal] = REJECTED, UNALIGNED
    pos = np.full(n, SKIP, np.uint32)
    out = empty_lists(caps)
    counts = np.zeros(6, np.uint32)
    for j, (L, mask) in enumerate((("hs", (cls == 1) | (cls == 2)), ("ck", cls == 3), ("data", cls == 4))):
        idx = np.nonzero(mask)[0]
        r = min(len(idx), caps[j])
        counts[j], counts[3 + j] = r, len(idx)
        listed = idx[:r]
        status[listed], status[idx[r:]] = PENDING, FULL
        pos[listed] = np.arange(r, dtype=np.uint32)
        rows = desc[listed].copy()
        rows["key_idx"] = 0
        out[L + "_desc"][:r] = rows
        if L == "hs":
            for name, c in (("init_desc", 1), ("resp_desc", 2)):
                own = cls[listed] == c
                out[name][:r][own] = rows[own]
        if L != "ck":
            out[L + "_addrs"][:r, :18] = addrs[listed, :18]
    out.update(status=status, cls=cls, pos=pos, counts=counts)
    return out


def verdict_loop(status, cls, pos, caps, chains):
    """the header's way back -> status; chains = dict(filter, init, finish, cookie, data), each a status array over
    its list or None"""
    out = np.array(status, np.uint8, copy=True)
    for i in range(len(out)):
        if out[i] != PENDING:
            continue
        c, k = int(cls[i]), int(pos[i])
        st = PENDING
        if c in (1, 2) and k < caps[0] and chains.get("filter") is not None:
            st = int(chains["filter"][k])
            if st == OK:
                own = chains.get("init" if c == 1 else "finish")
                st = int(own[k]) if own is not None else PENDING
        elif c == 3 and k < caps[1] and chains.get("cookie") is not None:
            st = int(chains["cookie"][k])
        elif c == 4 and k < caps[2] and chains.get("data") is not None:
            st = int(chains["data"][k])
        out[i] = st
    return out


def verdict_model(status, cls, pos, caps, chains):
    """verdict_loop with numpy"""
    out = np.array(status, np.uint8, copy=True)
    cls, pos = np.asarray(cls), np.asarray(pos, np.uint32)
    todo = out == PENDING

    def take(mask, arr, cap):
        m = todo & mask & (pos < cap)
        return m, np.asarray(arr, np.uint8)[pos[m]]

    if chains.get("filter") is not None:
        for c, name in ((1, "init"), (2, "finish")):
            m, f = take(cls == c, chains["filter"], caps[0])
            own = chains.get(name)
            o = np.asarray(own, np.uint8)[pos[m]] if own is not None else np.full(len(f), PENDING, np.uint8)
            out[m] = np.where(f != OK, f, o)
    for c, name, cap in ((3, "cookie", caps[1]), (4, "data", caps[2])):
        if chains.get(name) is not None:
            m, v = take(cls == c, chains[name], cap)
            out[m] = v
    return out


# ------------------------------------------------------------------ the cases
# One small buf serves every batch: the demux never writes it, so descriptors may all point at a few type words.
BUF_LEN = 1024
SLOTS = {1: 0, 2: 160, 3: 256, 4: 320, 0: 336, 5: 352, 0x01000000: 368, 0xFFFFFFFF: 384}  # type word -> offset
LEN_OF = {1: INIT_LEN, 2: RESP_LEN, 3: COOKIE_LEN, 4: 96}


def make_buf(seed=0):
    buf = np.random.default_rng([seed, 99]).integers(0, 256, BUF_LEN, dtype=np.uint8)
    for t, off in SLOTS.items():
        buf[off:off + 4] = np.frombuffer(np.uint32(t).tobytes(), np.uint8)
    return buf


def good(t, key=0):
    """a descriptor the demux lists: type t at its slot, with t's length"""
    return (SLOTS[t], LEN_OF[t], key)


# one datagram per branch of the loop: (descriptor, class, status before capacities)
BRANCHES = [
    ((SLOTS[1], INIT_LEN, SKIP), 0, REJECTED),             # an empty slot, even where everything else is right
    ((SLOTS[4] + 8, 96, 0), 0, UNALIGNED),
    ((SLOTS[4] + 1, 96, SKIP), 0, REJECTED),               # SKIP is answered before alignment
    ((SLOTS[4], 3, 0), 0, INVALID),                        # len == 3
    ((SLOTS[4], 0, 0), 0, INVALID),
    ((BUF_LEN - 16, 32, 0), 0, INVALID),                   # past the end of buf
    ((BUF_LEN, 4, 0), 0, INVALID),                         # starts at the end
    ((BUF_LEN + 16, 4, 0), 0, INVALID),                    # starts past the end
    (((1 << 64) - 16, 32, 0), 0, INVALID),                 # offset + len wraps 64 bits
    (((1 << 64) - 16, 0xFFFFFFFF, 0), 0, INVALID),
    ((SLOTS[1] + 8, 3, 0), 0, UNALIGNED),                  # alignment is answered before the length
    (good(1), 1, PENDING),
    ((SLOTS[1], RESP_LEN, 0), 0, INVALID),                 # type 1 with length 92
    ((SLOTS[1], INIT_LEN + 16, 0), 0, INVALID),
    (good(2, key=7), 2, PENDING),                          # any key_idx but SKIP; the row is written with 0
    ((SLOTS[2], INIT_LEN, 0), 0, INVALID),                 # type 2 with length 148
    (good(3), 3, PENDING),
    ((SLOTS[3], COOKIE_LEN + 16, 0), 0, INVALID),
    ((SLOTS[3], INIT_LEN, 0), 0, INVALID),
    (good(4), 4, PENDING),
    ((SLOTS[4], 4, 0), 4, PENDING),                        # a type-4 datagram of any length is listed
    ((SLOTS[4], 33, 1), 4, PENDING),
    ((BUF_LEN - 16, 16, 0), 0, INVALID),                   # the last 16 bytes of buf: in bounds, a random type word
    ((SLOTS[0], 64, 0), 0, INVALID),                       # type 0
    ((SLOTS[5], 64, 0), 0, INVALID),                       # type 5
    ((SLOTS[0x01000000], INIT_LEN, 0), 0, INVALID),        # a non-zero reserved byte: the type word is not 1
    ((SLOTS[0xFFFFFFFF], 64, 0), 0, INVALID),
]


def branch_table():
    """-> (desc, addrs, buf, classes, statuses) of BRANCHES"""
    buf = make_buf()
    buf[BUF_LEN - 16:BUF_LEN - 12] = (9, 9, 9, 9)
    desc = np.array([b[0] for b in BRANCHES], DESC_DTYPE)
    return desc, rand_addrs(len(desc), 5), buf, [b[1] for b in BRANCHES], [b[2] for b in BRANCHES]


def rand_addrs(n, seed=0):
    """the pad bytes too: no list may carry them over"""
    return np.random.default_rng([n, seed, 3]).integers(0, 256, (n, ADDR), dtype=np.uint8)


JUNK = [(SLOTS[4], 96, SKIP), (SLOTS[4] + 4, 96, 0), (SLOTS[4], 3, 0), (BUF_LEN - 16, 64, 0), ((1 << 64) - 16, 32, 0),
        (SLOTS[1], RESP_LEN, 0), (SLOTS[2], INIT_LEN, 0), (SLOTS[3], 80, 0), (SLOTS[0], 64, 0), (SLOTS[5], 64, 0),
        (SLOTS[0x01000000], INIT_LEN, 0)]
MIXES = ("random", "all_init", "all_resp", "all_cookie", "all_data", "alternate", "last_tile", "junk")


def mixed_desc(n, mix="random", seed=0):
    """n descriptors into make_buf(): classes per `mix`.  random: every class and every kind of junk, any key_idx;
    all_*: one class; alternate: 1, 2, 3, 4, junk in strict turn; last_tile: data with cookies only in the last tile
    of TILE datagrams; junk: nothing listed"""
    rng = np.random.default_rng([n, MIXES.index(mix), seed])
    kinds = np.array([good(1), good(2), good(3), good(4)] + JUNK, DESC_DTYPE)
    i = np.arange(n)
    if mix == "random":
        pick = rng.integers(0, len(kinds), n)
    elif mix.startswith("all_"):
        pick = np.full(n, ("init", "resp", "cookie", "data").index(mix[4:]))
    elif mix == "alternate":
        pick = np.where(i % 5 < 4, i % 5, 4 + (i // 5) % len(JUNK))
    elif mix == "last_tile":
        pick = np.where((i >= (n - 1) // TILE * TILE) & (i % 3 == 0), 2, 3)
    else:
        pick = 4 + rng.integers(0, len(JUNK), n)
    desc = kinds[pick].copy()
    if mix == "random":  # any key_idx but SKIP reads the same
        live = desc["key_idx"] != SKIP
        desc["key_idx"][live] = rng.integers(0, SKIP, int(live.sum()), dtype=np.uint32)
    return desc
