"""Cryptokey routing over librg_aead (include/rg_aead.h, "device-resident cryptokey routing"): the AllowedIPs
table built from (cidr, peer) pairs, the host lookup, and the three device calls.  As the rest of this package
it serves the tests and the benchmark; every call goes through the HIP library.

Reference -> this module
  peer_net.insert(cidr, peer) / lookup      (rustyguard-tun/src/lib.rs) -> build_table / lookup
  handle_intern up to send_message          (:214-243)                 -> route_batch_dev, send_batch_dev_routed
  handle_extern's source check              (:174-202)                 -> route_check_batch_dev
"""
from __future__ import annotations

import ipaddress

import numpy as np

from . import _lib
from ._lib import check, lib
from .aead import _nbytes, _ndesc, _stream_handle, _vp

PKT_UNROUTABLE = 9
PREFIX_DTYPE = np.dtype([("addr", np.uint8, 4), ("prefix_len", np.uint32), ("peer", np.uint32)])
ROOT_WORDS = 65536


def prefixes(pairs) -> np.ndarray:
    """(cidr, peer) pairs -> rg_route_prefix rows.  A cidr is "a.b.c.d/len" (host bits may be set: the table
    masks them) or an (address bytes, len) tuple."""
    pairs = list(pairs)
    rows = np.zeros(len(pairs), PREFIX_DTYPE)
    for i, (cidr, peer) in enumerate(pairs):
        if isinstance(cidr, str):
            addr, _, plen = cidr.partition("/")
            cidr = (ipaddress.IPv4Address(addr).packed, int(plen) if plen else 32)
        rows[i] = (np.frombuffer(bytes(cidr[0]), np.uint8), cidr[1], peer)
    return rows


def table_words(rows: np.ndarray) -> int:
    return int(lib().rg_route_table_words(_vp(rows) if len(rows) else None, len(rows)))


def build_table(pairs, cap_words: int | None = None) -> np.ndarray:
    """The route table (uint32 words, host memory) of (cidr, peer) pairs or of rg_route_prefix rows."""
    rows = pairs if isinstance(pairs, np.ndarray) and pairs.dtype == PREFIX_DTYPE else prefixes(pairs)
    rows = np.ascontiguousarray(rows)
    if cap_words is None:
        cap_words = table_words(rows)
        if cap_words == 0:
            raise _lib.RgError("route table: an invalid prefix row (prefix_len > 32 or peer > 0x7FFFFFFF)")
    table = np.zeros(cap_words, np.uint32)
    check(lib().rg_route_table_build(_vp(rows) if len(rows) else None, len(rows), _vp(table), cap_words),
          "rg_route_table_build")
    return table


def lookup(table: np.ndarray, addr) -> int:
    """Host lookup: the peer of an address ("a.b.c.d" or 4 bytes), PEER_NONE (0xFFFFFFFF) if none."""
    a = np.frombuffer(ipaddress.IPv4Address(addr).packed if isinstance(addr, str) else bytes(addr), np.uint8)
    assert a.size == 4
    return int(lib().rg_route_lookup(_vp(table), table.size, _vp(a)))


def route_workspace(engine, n: int, nkeys: int, device=None):
    """The scratch tensor (uint8, on the engine's device) send_batch_dev_routed needs (rg_route_workspace_size)."""
    import torch

    size = int(engine.library.rg_route_workspace_size(n, nkeys))
    if size == 0:
        raise _lib.RgError(f"no workspace can hold a batch of {n} packets")
    return torch.empty(size, dtype=torch.uint8, device=device if device is not None else f"cuda:{engine.device}")


def route_batch_dev(engine, table, peer_slot, desc, buf, slots_out, desc_out, status, peers_out=None, stream=None):
    """rg_route_batch_dev: destination lookup, peer -> key row and the zero padding of a batch of inner packets.
    table: the uint32 route table on the device; peer_slot uint32 one per peer; desc rg_pkt_desc rows with the
    unpadded inner lengths; slots_out uint32 / desc_out rg_pkt_desc / status uint8 / peers_out uint32 (optional)
    one per packet."""
    n = _ndesc(desc)
    assert _nbytes(slots_out) >= 4 * n and _nbytes(desc_out) >= 16 * n and _nbytes(status) >= n
    assert peers_out is None or _nbytes(peers_out) >= 4 * n
    engine._check(engine.library.rg_route_batch_dev(engine.handle, _vp(table), _nbytes(table) // 4, _vp(peer_slot),
                                                    _nbytes(peer_slot) // 4, _vp(desc), n, _vp(buf), _nbytes(buf),
                                                    _vp(peers_out), _vp(slots_out), _vp(desc_out), _vp(status),
                                                    _stream_handle(stream)), "rg_route_batch_dev")


def route_check_batch_dev(engine, table, slot_peer, desc, key_idx, buf, status, inner_len_out=None, stream=None):
    """rg_route_check_batch_dev: the source check behind recv_batch_dev_resident.  slot_peer uint32 one per key
    row; desc the frames' descriptors; key_idx what the receive reported; status updated in place; inner_len_out
    (uint32, optional) the inner packets' total_length."""
    n = _ndesc(desc)
    assert _nbytes(key_idx) >= 4 * n and _nbytes(status) >= n
    assert inner_len_out is None or _nbytes(inner_len_out) >= 4 * n
    engine._check(engine.library.rg_route_check_batch_dev(engine.handle, _vp(table), _nbytes(table) // 4,
                                                          _vp(slot_peer), _nbytes(slot_peer) // 4, _vp(desc),
                                                          _vp(key_idx), n, _vp(buf), _nbytes(buf), _vp(status),
                                                          _vp(inner_len_out), _stream_handle(stream)),
                  "rg_route_check_batch_dev")


def send_batch_dev_routed(engine, keys, receivers, state, table, peer_slot, desc, buf, status, peers_out=None,
                          counters_out=None, rekey_out=None, now_ns=None, workspace=None, stream=None):
    """rg_send_batch_dev_routed: route, reserve counters, seal, all on `stream` with no host step.  Returns the
    workspace used (its first 16 n bytes are the route's working descriptors)."""
    n = _ndesc(desc)
    nkeys = _nbytes(keys) // 32
    assert _nbytes(state) >= 24 * nkeys and _nbytes(receivers) >= 4 * nkeys and _nbytes(status) >= n
    assert peers_out is None or _nbytes(peers_out) >= 4 * n
    assert (counters_out is None or _nbytes(counters_out) >= 8 * n) and (rekey_out is None or _nbytes(rekey_out) >= n)
    assert now_ns is None or _nbytes(now_ns) >= 8
    if workspace is None:
        workspace = route_workspace(engine, n, nkeys)
    engine._check(engine.library.rg_send_batch_dev_routed(engine.handle, _vp(keys), _vp(receivers), nkeys, _vp(state),
                                                          _vp(table), _nbytes(table) // 4, _vp(peer_slot),
                                                          _nbytes(peer_slot) // 4, _vp(desc), n, _vp(now_ns), _vp(buf),
                                                          _nbytes(buf), _vp(peers_out), _vp(status),
                                                          _vp(counters_out), _vp(rekey_out), _vp(workspace),
                                                          _nbytes(workspace), _stream_handle(stream)),
                  "rg_send_batch_dev_routed")
    return workspace
