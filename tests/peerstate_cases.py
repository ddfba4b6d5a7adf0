"""The Python model of the device-resident peer handshake state (rg_hs_peer_state and the four rg_peer_*_batch_dev
calls) and the case builders of its tests.

The three fields are those the reference keeps in Peer (rustyguard-core/src/lib.rs:170-180).  ts_loop is the
timestamp-replay check of handle_handshake_init (handshake.rs:88-91) as the reference runs it, one row after the
other; ts_by_max is the same result the way the device computes it, as a prefix maximum per peer.  consume_loop is
handle_cookie / decrypt_cookie (handshake.rs:233-257) in order, so the last valid message of a peer wins;
record_loop is `peer.last_sent_mac1 = mac1` in order.  BLAKE2s and XChaCha20-Poly1305 are the CPU oracle's.
A state row is 64 bytes: latest_ts[12], has_cookie u32, cookie[16], last_sent_mac1[16], pad[16].
"""
from __future__ import annotations

import numpy as np

from oracle import oracle

OK, DECRYPT_ERR, INVALID, REJECTED, UNALIGNED = 0, 1, 2, 3, 4
PEER_NONE = 0xFFFFFFFF
KEY_SKIP = 0xFFFFFFFF
ROW = 64
ZERO_RESULT = bytes(108) + PEER_NONE.to_bytes(4, "little") + bytes(16)  # a turned-down row: zeros, peer = RG_PEER_NONE


def cookie_key(pk: bytes) -> bytes:
    """cookie_key(public key) = BLAKE2s-256("cookie--" || pk) (rustyguard-crypto/src/lib.rs:75-77)."""
    return oracle.blake2s(b"cookie--" + pk)


def state_row(latest_ts: bytes = bytes(12), cookie: bytes | None = None, mac1: bytes = bytes(16),
              pad: bytes = bytes(16)) -> bytes:
    row = latest_ts + (1 if cookie is not None else 0).to_bytes(4, "little") + (cookie or bytes(16)) + mac1 + pad
    assert len(row) == ROW
    return row


def result_row(ts: bytes, peer: int, fill: int = 0x11) -> bytes:
    """an rg_hs_init_result whose secret fields hold `fill`: chain, hash, ephemeral, timestamp, peer, sender, pad"""
    row = bytes([fill]) * 96 + ts + (peer & 0xFFFFFFFF).to_bytes(4, "little") + bytes([fill]) * 4 + bytes(12)
    assert len(row) == 128
    return row


def _ts(row: bytes) -> bytes:
    return row[96:108]


def _peer(row: bytes) -> int:
    return int.from_bytes(row[108:112], "little")


# --------------------------------------------------------------- timestamps
def ts_loop(state: list, results: list, status: list, npeers: int | None = None):
    """The reference's loop, literally, over the rows in array order.  Returns (state, results, status,
    peers_out) afterwards; the inputs are not touched."""
    npeers = len(state) if npeers is None else npeers
    state, results, status = list(state), list(results), list(status)
    peers_out = [PEER_NONE] * len(results)
    for i, row in enumerate(results):
        if status[i] != OK:
            continue
        p = _peer(row)
        if p >= npeers:
            status[i], results[i] = INVALID, ZERO_RESULT
            continue
        if _ts(row) < state[p][:12]:  # bytes compare as big-endian numbers
            status[i], results[i] = REJECTED, ZERO_RESULT
        else:
            state[p] = _ts(row) + state[p][12:]
            peers_out[i] = p
    return state, results, status, peers_out


def ts_by_max(state: list, results: list, status: list, npeers: int | None = None):
    """The same result as a prefix maximum: row i is accepted iff its timestamp >= max(latest at the start, the
    timestamps of the eligible rows ahead of it with the same peer); latest ends as the maximum of them all."""
    npeers = len(state) if npeers is None else npeers
    state_out, res_out, st_out = list(state), list(results), list(status)
    peers_out = [PEER_NONE] * len(results)
    val = lambda b: int.from_bytes(b, "big")  # noqa: E731
    elig = [i for i in range(len(results)) if status[i] == OK and _peer(results[i]) < npeers]
    for i in range(len(results)):
        if status[i] == OK and _peer(results[i]) >= npeers:
            st_out[i], res_out[i] = INVALID, ZERO_RESULT
    for p in sorted({_peer(results[i]) for i in elig}):
        rows = [i for i in elig if _peer(results[i]) == p]  # stable: array order
        start = val(state[p][:12])
        prefix = 0  # the identity: exclusive prefix maximum of the group
        for i in rows:
            if val(_ts(results[i])) < max(start, prefix):
                st_out[i], res_out[i] = REJECTED, ZERO_RESULT
            else:
                peers_out[i] = p
            prefix = max(prefix, val(_ts(results[i])))
        state_out[p] = max(start, prefix).to_bytes(12, "big") + state[p][12:]
    return state_out, res_out, st_out, peers_out


def random_ts_batch(rng, n: int, npeers: int, nts: int = 6, bad: float = 0.1, out_of_range: int = 3):
    """n result rows over npeers peers with few distinct timestamps (so ties are common), about `bad` of them
    with a status that is not OK and `out_of_range` OK rows whose peer is >= npeers.  Returns (results, status)."""
    pool = [bytes(rng.integers(0, 256, 12, dtype=np.uint8)) for _ in range(nts)]
    pool += [pool[0][:11] + bytes([pool[0][11] ^ 1]), bytes([pool[0][0] ^ 0x80]) + pool[0][1:]]
    results, status = [], []
    far = set(rng.choice(n, min(out_of_range, n), replace=False).tolist()) if out_of_range else set()
    for i in range(n):
        p = int(rng.integers(0, npeers))
        st = OK
        if i in far:
            p = [npeers, npeers + 5, PEER_NONE][i % 3]
        elif rng.random() < bad:
            st = [DECRYPT_ERR, INVALID, REJECTED, UNALIGNED, 8][int(rng.integers(0, 5))]
        if st == OK:
            results.append(result_row(pool[int(rng.integers(0, len(pool)))], p, fill=1 + i % 250))
        else:
            results.append(ZERO_RESULT)  # as the init call leaves a failure
        status.append(st)
    return results, status


def _t(hexs: str) -> bytes:
    b = bytes.fromhex(hexs)
    assert len(b) == 12
    return b


T_MID = _t("400000006553f100" "0000c350")
# Hand-made edge batches: (name, latest_ts of peer 0 at the start, the timestamps of peer 0's rows in order, the
# verdicts the reference's rule gives them).  Bytes compare big-endian: byte 0 is the most significant.
EDGE_TS = [
    ("equal_to_latest_passes", T_MID, [T_MID, T_MID], [OK, OK]),
    ("byte0_only", T_MID, [bytes([0x3F]) + T_MID[1:], bytes([0x41]) + T_MID[1:], T_MID], [REJECTED, OK, REJECTED]),
    ("byte11_only", T_MID, [T_MID[:11] + b"\x4f", T_MID[:11] + b"\x51", T_MID], [REJECTED, OK, REJECTED]),
    # 00 01 00 00 against 01 00 00 00 inside one 32-bit word: little-endian words would order them the other way
    ("le_word_flip_word0", _t("00010000" "00000000" "00000000"),
     [_t("01000000" "00000000" "00000000"), _t("00010000" "00000000" "00000000")], [OK, REJECTED]),
    ("le_word_flip_word1", _t("40000000" "00010000" "00000000"),
     [_t("40000000" "00000100" "00000000"), _t("40000000" "01000000" "00000000"),
      _t("40000000" "00010000" "00000000")], [REJECTED, OK, REJECTED]),
    ("le_word_flip_word2", _t("40000000" "00000000" "00010000"),
     [_t("40000000" "00000000" "01000000"), _t("40000000" "00000000" "00010000")], [OK, REJECTED]),
    ("fresh_peer_takes_zero", bytes(12), [bytes(12), bytes(11) + b"\x01", bytes(12)], [OK, OK, REJECTED]),
    ("all_ff", b"\xff" * 12, [b"\xff" * 12, b"\xff" * 11 + b"\xfe"], [OK, REJECTED]),
    ("five_then_three", bytes(12), [bytes(11) + b"\x05", bytes(11) + b"\x03", bytes(11) + b"\x05"],
     [OK, REJECTED, OK]),
]


def edge_ts_case(name: str):
    """(state, results, status, the verdicts) of one EDGE_TS batch: peer 0's rows interleaved with rows of peer 1
    (which starts from a cookie and a mac1 that must stay) and a row that is not OK."""
    _, latest, tss, verdicts = next(e for e in EDGE_TS if e[0] == name)
    state = [state_row(latest, mac1=bytes(range(16))), state_row(T_MID, cookie=bytes(range(16, 32)))]
    results, status, want = [], [], []
    for k, (ts, v) in enumerate(zip(tss, verdicts)):
        results += [result_row(ts, 0, 0x20 + k), result_row(T_MID, 1, 0x40 + k)]
        status += [OK, OK]
        want += [v, OK]
    results.insert(1, ZERO_RESULT)
    status.insert(1, DECRYPT_ERR)
    want.insert(1, DECRYPT_ERR)
    return state, results, status, want


# ------------------------------------------------------------------- cookies
def cookie_message(receiver: int, nonce: bytes, key: bytes, mac1: bytes, cookie: bytes) -> bytes:
    """CookieMessage: le32(3) || receiver || nonce[24] || XChaCha20-Poly1305(key, nonce, aad = mac1, cookie)."""
    ct, tag = oracle.xaead_seal(key, nonce, mac1, cookie)
    msg = (3).to_bytes(4, "little") + receiver.to_bytes(4, "little") + nonce + ct + tag
    assert len(msg) == 64
    return msg


def consume_one(msg: bytes, state: list, keys: list, table: dict, *, aligned=True, in_buf=True, length=64,
                gated=False, key_skip=False):
    """One message by the consume call's table against the state as it stood before the call: (status, cookie,
    peer or None)."""
    zero = bytes(16)
    if not aligned:
        return UNALIGNED, zero, None
    if not in_buf or length != 64:
        return INVALID, zero, None
    if gated or key_skip:
        return REJECTED, zero, None
    if msg[0:4] != (3).to_bytes(4, "little"):
        return INVALID, zero, None
    p = table.get(int.from_bytes(msg[4:8], "little"))
    if p is None:
        return REJECTED, zero, None
    if p >= len(state):
        return INVALID, zero, None
    pt = oracle.xaead_open(keys[p], msg[8:32], state[p][32:48], msg[32:48], msg[48:64])
    if pt is None:
        return DECRYPT_ERR, zero, None
    return OK, bytes(pt), p


def consume_loop(state: list, keys: list, table: dict, msgs: list, flags: list):
    """handle_cookie over the batch in array order: every message that opens is OK and overwrites the peer's
    cookie, so the last valid one stays.  last_sent_mac1 does not change within the call.  Returns (state,
    statuses, cookies_out)."""
    after = list(state)
    st, out = [], []
    for msg, kw in zip(msgs, flags):
        s, ck, p = consume_one(msg, state, keys, table, **kw)
        if s == OK:
            after[p] = after[p][:12] + (1).to_bytes(4, "little") + ck + after[p][32:]
        st.append(s)
        out.append(ck)
    return after, st, out


def gather(state: list, peer_idx: list):
    """(cookies, has_cookie) as the initiate and response calls take them."""
    cookies, has = [], []
    for p in peer_idx:
        h = p < len(state) and int.from_bytes(state[p][12:16], "little") != 0
        cookies.append(state[p][16:32] if h else bytes(16))
        has.append(1 if h else 0)
    return cookies, has


def record_loop(state: list, peer_idx: list, status: list, messages: list, mac1_offset: int):
    """peer.last_sent_mac1 = the message's mac1 field, in array order over the rows that were sent."""
    after = list(state)
    for p, s, m in zip(peer_idx, status, messages):
        if s == OK and p < len(state):
            after[p] = after[p][:32] + m[mac1_offset:mac1_offset + 16] + after[p][48:]
    return after


def rows_array(rows: list, width: int) -> np.ndarray:
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), width).copy()
