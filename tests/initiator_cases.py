"""The Python model of the Noise IKpsk2 initiator path and the case builders of its tests.

initiate restates encrypt_handshake_init (rustyguard-crypto/src/lib.rs:287-344) and consume_response restates
decrypt_handshake_resp + HandshakeState::split(true) (lib.rs:435-465, prim.rs:299-313) behind the session lookup
of handle_handshake_resp (rustyguard-core/src/handshake.rs:140-230), both with the statuses and rows of
include/rg_aead.h; commit is the reference's in-order loop over a batch.  The primitives and the responder are
those of tests/handshake_cases.py.
"""
from __future__ import annotations

import numpy as np

import handshake_cases as hc
from handshake_cases import (DECRYPT_ERR, INVALID, KEY_SKIP, KEYEXCHANGE, OK, PEER_NONE, REJECTED,  # noqa: F401
                             UNALIGNED)

ZERO_PENDING = bytes(96) + PEER_NONE.to_bytes(4, "little") + bytes(28)  # empty, failed or consumed
ZERO_MSG = bytes(160)


def pending_row(chain: bytes, hash_: bytes, esk: bytes, peer: int, sender: int) -> bytes:
    """rg_hs_pending: chain, hash, esk, peer, sender, pad[24]."""
    row = chain + hash_ + esk + peer.to_bytes(4, "little") + sender.to_bytes(4, "little") + bytes(24)
    assert len(row) == 128
    return row


def initiate(sk_i: bytes, peers: list, peer_idx: int, esk: bytes, ts: bytes, sender: int, cookie: bytes | None = None):
    """encrypt_handshake_init for one ungated row: (status, the 160-byte message row, the pending row).
    peers: (public key, preshared key, mac1 key) rows."""
    if peer_idx >= len(peers):
        return INVALID, ZERO_MSG, ZERO_PENDING
    pk_r = peers[peer_idx][0]
    if hc.x25519(esk, pk_r) == bytes(32) or hc.x25519(sk_i, pk_r) == bytes(32):  # es, ss
        return KEYEXCHANGE, ZERO_MSG, ZERO_PENDING
    msg, hs = hc.make_initiation(sk_i, pk_r, esk, ts, sender)
    msg = msg[:116] + hc.mac(peers[peer_idx][2], msg[:116]) + bytes(16)  # mac1 under the row's own mac1 key
    if cookie is not None:
        msg = msg[:132] + hc.mac(cookie, msg[:132])
    assert len(msg) == 148
    return OK, msg + bytes(12), pending_row(hs.chain, hs.hash, esk, peer_idx, sender)


ZERO_OUT = (bytes(64), PEER_NONE, 0)  # a failure's key row, pend_idx_out and remote_out


def consume_response(msg: bytes, table: dict, pending: list, sk_i: bytes, peers: list, *, aligned: bool = True,
                     in_buf: bool = True, length: int = 92, gated: bool = False, key_skip: bool = False):
    """One message by the finish call's table, against the pending rows as they stand: (status, send key ||
    receive key, pending row, remote id).  table: receiver id -> pending row, as the device table maps it.
    Does not touch `pending`: a failing message leaves its row alone, and consuming is commit's."""
    if not aligned:
        return (UNALIGNED, *ZERO_OUT)
    if not in_buf or length != 92:
        return (INVALID, *ZERO_OUT)
    if gated or key_skip:
        return (REJECTED, *ZERO_OUT)
    if msg[0:4] != (2).to_bytes(4, "little"):
        return (INVALID, *ZERO_OUT)
    row = table.get(int.from_bytes(msg[8:12], "little"))
    if row is None:
        return (REJECTED, *ZERO_OUT)
    if row >= len(pending):
        return (INVALID, *ZERO_OUT)
    p = pending[row]
    peer = int.from_bytes(p[96:100], "little")
    if peer == PEER_NONE:
        return (REJECTED, *ZERO_OUT)
    if peer >= len(peers):
        return (INVALID, *ZERO_OUT)
    esk = p[64:96]
    if hc.x25519(esk, msg[12:44]) == bytes(32) or hc.x25519(sk_i, msg[12:44]) == bytes(32):  # ee, se
        return (KEYEXCHANGE, *ZERO_OUT)
    fin = hc.finish_initiator(msg, hc.HS(p[0:32], p[32:64]), sk_i, esk, peers[peer][1])
    if fin is None:
        return (DECRYPT_ERR, *ZERO_OUT)
    return OK, fin[0] + fin[1], row, int.from_bytes(msg[4:8], "little")


def commit(msgs: list, flags: list, table: dict, pending: list, sk_i: bytes, peers: list):
    """The batch in array order, by the header's table: every message is judged against the pending rows as
    they stand before the batch (so its own failure -- a bad tag, a zero secret -- is reported even behind a
    message that finished its row); the first message that finishes a pending row consumes it (zeros, peer =
    RG_PEER_NONE) and a later valid one for the same row is rejected; a message that fails leaves its row alone.
    flags: consume_response's keyword arguments per message.
    Returns (statuses, key rows, pending rows out, remote ids, the pending rows afterwards)."""
    after = list(pending)
    out = []
    for msg, kw in zip(msgs, flags):
        res = consume_response(msg, table, pending, sk_i, peers, **kw)
        if res[0] == OK:
            if after[res[2]] == ZERO_PENDING:  # a lower-indexed message of this batch finished the row
                res = (REJECTED, *ZERO_OUT)
            else:
                after[res[2]] = ZERO_PENDING
        out.append(res)
    return ([r[0] for r in out], [r[1] for r in out], [r[2] for r in out], [r[3] for r in out], after)


def commit_by_min(msgs: list, flags: list, table: dict, pending: list, sk_i: bytes, peers: list):
    """The same result the way the device computes it: every message judged against the pending rows as they
    stand before the batch, then the lowest index per row wins and the other claimants are rejected."""
    res = [consume_response(m, table, pending, sk_i, peers, **kw) for m, kw in zip(msgs, flags)]
    st = np.array([r[0] for r in res])
    rows = np.array([r[2] for r in res], np.int64)
    claim = np.full(len(pending), len(msgs), np.int64)
    ok = np.flatnonzero(st == OK)
    np.minimum.at(claim, rows[ok], ok)
    after = list(pending)
    for i in ok:
        if claim[rows[i]] == i:
            after[rows[i]] = ZERO_PENDING
        else:
            res[i] = (REJECTED, *ZERO_OUT)
    return ([r[0] for r in res], [r[1] for r in res], [r[2] for r in res], [r[3] for r in res], after)


# -------------------------------------------------------------- case builders
INITIATE_KINDS = ["valid", "valid_cookie", "gated", "bad_peer", "low_order_peer"]
FINISH_KINDS = ["valid", "tag_flipped", "eph_zero", "eph_one", "type1", "len148", "offset8", "past_buf", "gated",
                "key_skip", "unknown_receiver", "consumed_row", "bad_peer_row"]


class Initiator:
    """An initiator with npeers responders it knows (one more peer row, the last, holds a public key of small
    order) and a pool of neph ephemeral keys, all drawn from one seeded generator."""

    def __init__(self, seed: int, npeers: int = 5, neph: int = 40):
        rng = np.random.default_rng(seed)
        rb = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
        self.rng, self.rb = rng, rb
        self.sk_i = rb(32)
        self.pk_i = hc.pubkey(self.sk_i)
        self.sk_r = [rb(32) for _ in range(npeers)]
        self.peers = [(hc.pubkey(sk), rb(32), hc.mac1_key(hc.pubkey(sk))) for sk in self.sk_r]
        self.esk = [rb(32) for _ in range(neph)]
        self.own = np.frombuffer(self.sk_i + self.pk_i, np.uint8).copy()
        self.npeers = npeers

    def peers_with_low_order(self, i: int = 0) -> list:
        """The peer rows plus one whose public key is the i-th small-order point of hc.EDGE_POINTS."""
        pk = hc.EDGE_POINTS[i % 4][1]
        return self.peers + [(pk, bytes(32), hc.mac1_key(pk))]


def initiate_batch(ini: Initiator, kinds: list):
    """The inputs of one rg_handshake_initiate_batch_dev call and the model's rows.  Returns a dict of arrays:
    peers (rows incl. the low-order one), peer_idx, gate, esk, ts, sids, cookies, has_cookie, and want_status,
    want_msgs [n, 160], want_pending [n, 128] (None entries for gated rows: untouched)."""
    n = len(kinds)
    rng = ini.rng
    peers = ini.peers_with_low_order(int(rng.integers(0, 4)))
    low = len(peers) - 1
    peer_idx = np.zeros(n, np.uint32)
    gate = np.zeros(n, np.uint8)
    esk = np.zeros((n, 32), np.uint8)
    ts = np.zeros((n, 12), np.uint8)
    sids = rng.permutation(1 << 20)[:n].astype(np.uint32) + 0x5000_0000  # unique: they key the pending table
    cookies = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    has_cookie = np.zeros(n, np.uint8)
    want = []
    for i, k in enumerate(kinds):
        esk[i] = np.frombuffer(ini.esk[i % len(ini.esk)], np.uint8)
        ts[i] = np.frombuffer(hc.tai64n(1_700_000_000 + i, 1000 * i), np.uint8)
        peer_idx[i] = i % ini.npeers
        if k == "valid_cookie":
            has_cookie[i] = 1 + i % 3
        elif k == "gated":
            gate[i] = [REJECTED, 7, INVALID, 6][i % 4]
        elif k == "bad_peer":
            peer_idx[i] = [len(peers), len(peers) + 7, PEER_NONE][i % 3]
        elif k == "low_order_peer":
            peer_idx[i] = low
        want.append(None if k == "gated" else
                    initiate(ini.sk_i, peers, int(peer_idx[i]), esk[i].tobytes(), ts[i].tobytes(), int(sids[i]),
                             cookies[i].tobytes() if has_cookie[i] else None))
    return dict(peers=hc.peer_rows(peers), peer_list=peers, peer_idx=peer_idx, gate=gate, esk=esk, ts=ts, sids=sids,
                cookies=cookies, has_cookie=has_cookie, want=want)


def respond(ini: Initiator, msg: bytes, peer: int, esk_r: bytes, session_id: int) -> bytes:
    """The 92-byte response of responder `peer` to a 148-byte initiation, by the responder model."""
    st, row = hc.consume_initiation(msg, ini.sk_r[peer], [ini.pk_i])
    assert st == OK
    st, resp, _ = hc.build_response(row, [(ini.pk_i, ini.peers[peer][1], hc.mac1_key(ini.pk_i))], esk_r, session_id, None)
    assert st == OK
    return resp


class FinishWorld:
    """npending pending rows of one initiator (two of them already consumed, one with peer = npeers) and one
    valid response per live row, from which finish_batch deals its messages."""

    def __init__(self, seed: int, npending: int = 40):
        self.ini = ini = Initiator(seed, neph=npending)
        rng = ini.rng
        self.sids = rng.permutation(1 << 20)[:npending].astype(np.uint32) + 0x6000_0000
        self.pending, self.responses = [], []
        for r in range(npending):
            peer = r % ini.npeers
            st, msg, row = initiate(ini.sk_i, ini.peers, peer, ini.esk[r], hc.tai64n(1_800_000_000, r), int(self.sids[r]))
            assert st == OK
            self.pending.append(row)
            self.responses.append(respond(ini, msg[:148], peer, ini.rb(32), 0x7000_0000 + r))
        self.table = {int(s): r for r, s in enumerate(self.sids)}
        # rows a response may not finish: two consumed earlier, one whose peer row does not exist
        self.consumed = [npending - 1, npending - 2]
        self.bad_peer = npending - 3
        for r in self.consumed:
            self.pending[r] = ZERO_PENDING
        p = bytearray(self.pending[self.bad_peer])
        p[96:100] = ini.npeers.to_bytes(4, "little")
        self.pending[self.bad_peer] = bytes(p)
        self.live = list(range(npending - 3))


def finish_batch(w: FinishWorld, plan: list, desc_dtype):
    """The frames of one rg_handshake_finish_batch_dev call.  plan: (kind, pending row) per message (the row is
    ignored by kinds that name their own).  Frames lie 96 bytes apart with 0 / 16 / 32-byte gaps (`past_buf`
    descriptors point across the end of the buffer).  Returns (desc, gate, buf, msgs, flags)."""
    rng = w.ini.rng
    n = len(plan)
    gaps = rng.integers(0, 3, n) * 16
    off, pos = [], 0
    for i in range(n):
        off.append(pos)
        pos += 96 + int(gaps[i])
    buf = rng.integers(0, 256, pos, dtype=np.uint8)
    desc = np.zeros(n, desc_dtype)
    gate = np.zeros(n, np.uint8)
    msgs, flags = [], []
    for i, (kind, row) in enumerate(plan):
        if kind == "consumed_row":
            row = w.consumed[i % 2]
        elif kind == "bad_peer_row":
            row = w.bad_peer
        m = bytearray(w.responses[row])
        kw = {}
        o, ln, key = off[i], 92, int(rng.integers(0, 1000))
        if kind == "tag_flipped":
            m[44 + int(rng.integers(0, 16))] ^= 1 << int(rng.integers(0, 8))
        elif kind == "eph_zero":
            m[12:44] = hc.le(0)
        elif kind == "eph_one":
            m[12:44] = hc.le(1)
        elif kind == "type1":
            m[0:4] = (1).to_bytes(4, "little")
        elif kind == "len148":
            ln, kw = 148, dict(length=148)
        elif kind == "offset8":
            o, kw = o + 8, dict(aligned=False)
        elif kind == "past_buf":
            o, kw = (pos - 91 + 15) // 16 * 16, dict(in_buf=False)  # the last boundary from which 92 bytes overrun
        elif kind == "gated":
            gate[i], kw = [REJECTED, 7, INVALID, 6][i % 4], dict(gated=True)
        elif kind == "key_skip":
            key, kw = KEY_SKIP, dict(key_skip=True)
        elif kind == "unknown_receiver":
            m[8:12] = (0x0BAD_0000 + i).to_bytes(4, "little")
        buf[off[i]:off[i] + 92] = np.frombuffer(bytes(m), np.uint8)
        desc[i] = (o, ln, key)
        msgs.append(bytes(m))
        flags.append(kw)
    return desc, gate, buf, msgs, flags
