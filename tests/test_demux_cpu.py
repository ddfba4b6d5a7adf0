"""The model of the inbound demultiplexer (tests/demux_cases.py) on its own, without a GPU: the rule order of the
header's loop on a hand-written table with one datagram per branch, the oracle's message-type rule, the invariants of
the lists, the way back, and the numpy form of both loops against the loops themselves."""
import numpy as np
import pytest

import demux_cases as dc
from oracle import oracle

CAPS = [(8, 8, 8), (0, 0, 0), (1, 0, 2), (3, 1, 0), (1000, 1000, 1000)]


def same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


def test_rule_order_on_the_branch_table():
    desc, addrs, buf, classes, statuses = dc.branch_table()
    n = len(desc)
    for i in range(n):
        assert dc.classify(desc[i], buf) == (classes[i], statuses[i]), (i, desc[i])
    out = dc.demux_loop(desc, addrs, buf, (n, n, n))
    assert list(out["cls"]) == classes and list(out["status"]) == statuses
    # the table holds every verdict the demux can give but RG_PKT_FULL, and every class
    assert set(statuses) == {dc.REJECTED, dc.UNALIGNED, dc.INVALID, dc.PENDING} and set(classes) == {0, 1, 2, 3, 4}
    hs = [i for i, c in enumerate(classes) if c in (1, 2)]
    assert list(out["counts"]) == [len(hs), classes.count(3), classes.count(4)] * 2
    # a listed row: the datagram's offset and len, key_idx 0, and its address with the pad zeroed
    for k, i in enumerate(hs):
        assert out["hs_desc"][k] == np.array((desc[i]["offset"], desc[i]["len"], 0), dc.DESC_DTYPE)
        assert bytes(out["hs_addrs"][k]) == bytes(addrs[i, :18]) + bytes(6) and out["pos"][i] == k
    assert (out["hs_desc"][len(hs):] == dc.INERT).all() and not out["hs_addrs"][len(hs):].any()
    assert bytes(dc.INERT.tobytes()) == bytes(12) + b"\xff" * 4
    same(out, dc.demux_model(desc, addrs, buf, (n, n, n)))


def test_type_rule_agrees_with_the_oracle():
    """tests/test_oracle_golden.py::test_message_type_dispatch pins the oracle's rule: the little-endian type word
    selects 1, 2, 3 (NOT_DATA) or 4; every other value is InvalidMessage.  The same words through the model, each in
    a frame of the length its type asks for."""
    types = [0, 1, 2, 3, 4, 5, 0xFF, 0x104, 0x01000000, 0xFFFFFFFF]
    buf = np.zeros(160 * len(types), np.uint8)
    desc = np.zeros(len(types), dc.DESC_DTYPE)
    for k, t in enumerate(types):
        buf[160 * k:160 * k + 4] = np.frombuffer(np.uint32(t).tobytes(), np.uint8)
        desc[k] = (160 * k, dc.LEN_OF.get(t, 48), 0)
    st, _ = oracle.open_batch(np.zeros((1, 32), np.uint8), desc.astype(oracle.DESC_DTYPE), buf.copy())
    out = dc.demux_loop(desc, dc.rand_addrs(len(types)), buf, (16, 16, 16))
    for k, t in enumerate(types):
        if st[k] == oracle.NOT_DATA:
            assert out["cls"][k] == t and t in (1, 2, 3) and out["status"][k] == dc.PENDING
        elif t == 4:
            assert out["cls"][k] == 4 and st[k] == oracle.DECRYPT_ERR  # data: on to the open, whose verdict it is
        else:
            assert st[k] == oracle.INVALID and out["cls"][k] == 0 and out["status"][k] == dc.INVALID, t
    assert [int(c) for c in out["cls"]] == [0, 1, 2, 3, 4, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("mix", dc.MIXES)
def test_list_invariants_and_the_numpy_form(mix):
    buf = dc.make_buf()
    for n in (1, 7, 300):
        desc, addrs = dc.mixed_desc(n, mix), dc.rand_addrs(n)
        for caps in CAPS:
            out = dc.demux_loop(desc, addrs, buf, caps)
            same(out, dc.demux_model(desc, addrs, buf, caps), (mix, n, caps))
            rank, seen = out["counts"][:3], out["counts"][3:]
            assert (seen >= rank).all() and list(rank) == [min(int(s), c) for s, c in zip(seen, caps)]
            where = {}
            for j, L in enumerate(dc.LISTS):
                idx = [i for i in range(n) if dc.list_of(int(out["cls"][i])) == L and out["status"][i] == dc.PENDING]
                assert len(idx) == rank[j] and [int(out["pos"][i]) for i in idx] == list(range(rank[j]))  # ascending in i
                full = [i for i in range(n) if dc.list_of(int(out["cls"][i])) == L and out["status"][i] == dc.FULL]
                assert len(full) == seen[j] - rank[j] and (not full or not idx or min(full) > max(idx))
                where[L] = set(idx)
                rows = out[L + "_desc"]
                assert (rows[rank[j]:] == dc.INERT).all() and (rows[:rank[j]]["key_idx"] == 0).all()
            assert not (where["hs"] & where["ck"]) and not (where["hs"] & where["data"]) and not (where["ck"] & where["data"])
            # init_desc and resp_desc partition hs_desc
            hs, ini, rsp = out["hs_desc"], out["init_desc"], out["resp_desc"]
            for k in range(caps[0]):
                live = [r for r in (ini[k], rsp[k]) if r != dc.INERT]
                assert len(live) == (1 if k < rank[0] else 0) and all(r == hs[k] for r in live)
                if k < rank[0]:
                    assert (ini[k] != dc.INERT) == (hs[k]["len"] == dc.INIT_LEN)


def test_verdict_leaves_pending_for_a_null_chain_and_a_bad_pos():
    buf = dc.make_buf()
    n = 200
    desc, addrs = dc.mixed_desc(n, "random", seed=3), dc.rand_addrs(n)
    caps = (30, 5, 40)
    out = dc.demux_loop(desc, addrs, buf, caps)
    rng = np.random.default_rng(11)
    chains = {k: rng.choice(np.array([dc.OK, dc.REJECTED, dc.INVALID, dc.COOKIE, dc.DECRYPT_ERR], np.uint8), c)
              for k, c in (("filter", caps[0]), ("init", caps[0]), ("finish", caps[0]), ("cookie", caps[1]), ("data", caps[2]))}
    chains["filter"][::2] = dc.OK
    status, cls, pos = out["status"], out["cls"], out["pos"]
    final = dc.verdict_loop(status, cls, pos, caps, chains)
    assert np.array_equal(final, dc.verdict_model(status, cls, pos, caps, chains))
    assert not (final == dc.PENDING).any() and np.array_equal(final[status != dc.PENDING], status[status != dc.PENDING])
    for i in np.nonzero(status == dc.PENDING)[0]:
        c, k = int(cls[i]), int(pos[i])
        if c in (1, 2):
            f = chains["filter"][k]
            assert final[i] == (f if f != dc.OK else chains["init" if c == 1 else "finish"][k])
        else:
            assert final[i] == chains["cookie" if c == 3 else "data"][k]
    # a chain that did not run: its datagrams stay pending, the others' verdicts are the same
    for gone in chains:
        part = {k: (None if k == gone else v) for k, v in chains.items()}
        got = dc.verdict_loop(status, cls, pos, caps, part)
        assert np.array_equal(got, dc.verdict_model(status, cls, pos, caps, part))
        own = {"filter": (1, 2), "init": (1,), "finish": (2,), "cookie": (3,), "data": (4,)}[gone]
        for i in range(n):
            mine = status[i] == dc.PENDING and cls[i] in own
            if gone in ("init", "finish"):
                mine = mine and chains["filter"][pos[i]] == dc.OK
            assert got[i] == (dc.PENDING if mine else final[i]), (gone, i)
    # a pos out of range or a cls outside 1-4 is never used as an index
    bad_pos, bad_cls = pos.copy(), cls.copy()
    pend = np.nonzero(status == dc.PENDING)[0]
    for i in pend[:10]:
        bad_pos[i] = caps[dc.LISTS.index(dc.list_of(int(cls[i])))] + (0 if i % 2 else 1 << 20)
    for i in pend[10:14]:
        bad_cls[i] = (0, 5, 255, 17)[i % 4]
    got = dc.verdict_loop(status, bad_cls, bad_pos, caps, chains)
    assert np.array_equal(got, dc.verdict_model(status, bad_cls, bad_pos, caps, chains))
    assert (got[pend[:14]] == dc.PENDING).all() and np.array_equal(got[pend[14:]], final[pend[14:]])
