"""The in-order model of the five peer-endpoint calls (include/rg_aead.h, "device-resident peer endpoints") and the
generators of the cases the CPU and GPU tests share.  The model is the header's loop, written out: the last eligible
item of a peer in array order leaves its address in the peer's row, every other row keeps its bytes."""
import numpy as np

OK, DECRYPT_ERR, REJECTED, PENDING = 0, 1, 3, 6
SKIP = NONE = 0xFFFFFFFF
ROW, ADDR = 32, 24  # rg_endpoint, rg_src_addr
WAVE = 64

SIZES = (1, 63, 64, 65, 257, 2049, 5000)
NPEERS = (1, 3, 300, 70001)
KINDS = ("constant", "round_robin", "blocks", "blocks_off17", "random")


def addr(ip: str, port: int, pad: bytes = bytes(6)) -> bytes:
    """one rg_src_addr"""
    import ipaddress

    return ipaddress.ip_address(ip).packed.ljust(16, b"\0") + port.to_bytes(2, "little") + pad


def some_row(a: bytes) -> bytes:
    """the rg_endpoint row a note leaves for the address a: ip, port_le, set = 1, zero"""
    return bytes(a[:18]) + b"\x01\x00" + bytes(12)


def is_some(row) -> bool:
    return bytes(row[18:20]) != b"\0\0"


# ------------------------------------------------------------------ the model
def recv_peers(slot_peer, key_idx):
    """peer_of for rg_endpoint_note_recv_batch_dev (and the finish wrapper, with pend_peers and pend_idx_out)"""
    nkeys = len(slot_peer)
    return [int(slot_peer[k]) if k < nkeys else NONE for k in (int(x) for x in key_idx)]


def note_loop(table, peer_of, status, src):
    """-> the table after the call; table uint8 [npeers][32], src uint8 [n][24]"""
    out = np.array(table, np.uint8, copy=True)
    npeers = len(out)
    for i, (p, s) in enumerate(zip(peer_of, status)):
        if s == OK and p < npeers:
            out[p] = np.frombuffer(some_row(bytes(src[i])), np.uint8)
    return out


def gather_loop(table, peer_of, idx, none):
    """-> (idx_out, dst uint8 [n][24]) of the two gathers; peer_of as above, NONE for an index out of range"""
    npeers = len(table)
    idx_out, dst = [], np.zeros((len(idx), ADDR), np.uint8)
    for i, (p, x) in enumerate(zip(peer_of, idx)):
        if p < npeers and is_some(table[p]):
            idx_out.append(int(x))
            dst[i, :18] = table[p][:18]
        else:
            idx_out.append(none)
    return idx_out, dst


def gate_loop(table, slot_peer, slots):
    return gather_loop(table, recv_peers(slot_peer, slots), slots, SKIP)


def peers_loop(table, peer_idx):
    return gather_loop(table, [int(p) for p in peer_idx], peer_idx, NONE)


# ------------------------------------------------------------------ the cases
def start_table(npeers, rng):
    """every third peer configured, with the `zero` field planted non-zero: a row no note writes keeps these bytes"""
    t = np.zeros((npeers, ROW), np.uint8)
    seeded = np.arange(0, npeers, 3)
    t[seeded, :18] = rng.integers(0, 256, (len(seeded), 18), dtype=np.uint8)
    t[seeded, 18] = 1
    t[seeded, 20:] = 0xEE
    return t


def note_case(n, npeers, kind, seed=0):
    """One receive batch over a session table: -> dict(slot_peer, key_idx, status, src, table, quiet_peer).
    Rows 0..G-1 are live sessions of distinct peers spread over the table (peer npeers - 1 among them); behind them
    one row of a peer only ineligible items name (when npeers allows), a free row and two rows whose peer is out of
    range.  A few items name those rows or a row past the table, whatever `kind` says, and the second wave (or the
    only one of a small batch with seed 1) holds no eligible lane."""
    rng = np.random.default_rng([n, npeers, KINDS.index(kind), seed])
    G = min(npeers, 300) if npeers < 3 else min(npeers - 1, 300)
    peers = [int(x) for x in np.unique(np.linspace(0, npeers - 1, G + (npeers >= 3)).astype(np.int64))]
    quiet_peer = peers.pop(len(peers) // 2) if npeers >= 3 else None
    G = len(peers)
    slot_peer = peers + ([quiet_peer] if quiet_peer is not None else []) + [NONE, npeers, min(npeers + 5, NONE - 1)]
    nkeys = len(slot_peer)
    quiet_row, free_row, bad_row = (G if quiet_peer is not None else None), nkeys - 3, nkeys - 2
    i = np.arange(n)
    pick = {"constant": np.zeros(n, np.int64), "round_robin": i % 3, "blocks": i // WAVE,
            "blocks_off17": (i + 17) // WAVE, "random": rng.integers(0, G, n)}[kind]
    key_idx = (pick % G).astype(np.uint32)
    status = rng.choice(np.array([OK, OK, OK, REJECTED, DECRYPT_ERR, PENDING], np.uint8), n)
    if n >= 2 * WAVE:
        status[WAVE:2 * WAVE][status[WAVE:2 * WAVE] == OK] = REJECTED
    elif seed == 1:
        status[status == OK] = DECRYPT_ERR
    elif n == 1:
        status[0] = OK
    # the special rows, at places spread over the batch (a batch of one wave or more)
    spots = [int(x) for x in rng.permutation(n)[:12]] if n >= WAVE - 1 else []
    specials = [(free_row, OK), (bad_row, OK), (bad_row + 1, OK), (nkeys, OK), (SKIP, OK), (nkeys + 7, REJECTED)]
    if quiet_row is not None:
        specials += [(quiet_row, REJECTED), (quiet_row, DECRYPT_ERR), (quiet_row, PENDING)]
    for at, (k, s) in zip(spots, specials):
        key_idx[at], status[at] = k, s
    src = rng.integers(0, 256, (n, ADDR), dtype=np.uint8)  # the pad bytes too: no note may carry them over
    return dict(slot_peer=slot_peer, key_idx=[int(k) for k in key_idx], status=[int(s) for s in status], src=src,
                table=start_table(npeers, rng), quiet_peer=quiet_peer)


def gather_case(n, npeers, seed=0):
    """-> dict(table, slot_peer, slots, peer_idx): unset peers, SKIP / NONE inputs, indices out of range"""
    rng = np.random.default_rng([n, npeers, 77, seed])
    table = start_table(npeers, rng)
    nkeys = min(npeers, 200) + 3
    slot_peer = [int(p) for p in rng.integers(0, npeers, nkeys - 3)] + [NONE, npeers, NONE - 1]
    slots = [int(x) for x in rng.integers(0, nkeys, n)]
    peer_idx = [int(x) for x in rng.integers(0, npeers, n)]
    for at, v in zip(rng.permutation(n)[:min(n, 6)], (SKIP, nkeys, nkeys + 1, SKIP - 1, 1 << 31, nkeys - 3)):
        slots[int(at)] = v
    for at, v in zip(rng.permutation(n)[:min(n, 5)], (NONE, npeers, npeers + 1, NONE - 1, 1 << 31)):
        peer_idx[int(at)] = max(v, npeers) if v != NONE else NONE
    return dict(table=table, slot_peer=slot_peer, slots=slots, peer_idx=peer_idx)
