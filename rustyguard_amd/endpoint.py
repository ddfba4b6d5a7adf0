"""The device-resident peer endpoints over librg_aead (include/rg_aead.h, "device-resident peer endpoints"): one
rg_endpoint row per peer with the claim words the note calls need, the three calls that move a row behind a receive
or a finished handshake, and the two that turn a send's slots or a list of peers into destination addresses.  As the
rest of this package it serves the tests and the benchmark; every call goes through the HIP library.

Reference -> this module
  decrypt_packet's endpoint move        (rustyguard-core/src/lib.rs:659-671)    -> note_recv_batch_dev
  handle_handshake_resp's endpoint move (rustyguard-core/src/handshake.rs:205)  -> note_finish_batch_dev
  send_message's early return           (rustyguard-core/src/lib.rs:550-553)    -> gate_batch_dev
  the keepalive and rekey destinations  (rustyguard-core/src/time.rs:67, :135)  -> gate_batch_dev, peers_batch_dev
  PeerState::new(p.endpoint)                                                    -> seed
"""
from __future__ import annotations

import ctypes

from .aead import _nbytes, _stream_handle, _vp, encode_src_addr

ENDPOINT_BYTES = 32  # rg_endpoint
ADDR_BYTES = 24  # rg_src_addr


class EndpointStruct(ctypes.Structure):
    """rg_endpoint"""
    _fields_ = [("ip", ctypes.c_uint8 * 16), ("port_le", ctypes.c_uint16), ("set", ctypes.c_uint16),
                ("zero", ctypes.c_uint8 * 12)]


def row_bytes(ip: str, port: int) -> bytes:
    """one rg_endpoint row that is Some(ip:port)"""
    return encode_src_addr(ip, port)[:18] + (1).to_bytes(2, "little") + bytes(12)


class EndpointTable:
    """npeers rg_endpoint rows (uint8 [npeers][32], all None) and the claim words of the note calls (int32 [npeers],
    zeroed once here and left zeroed by every call) on the engine's device."""

    def __init__(self, engine, npeers: int, device=None):
        import torch

        dev = device if device is not None else f"cuda:{engine.device}"
        self.engine, self.npeers = engine, npeers
        self.endpoints = torch.zeros((npeers, ENDPOINT_BYTES), dtype=torch.uint8, device=dev)
        self.claim = torch.zeros(npeers, dtype=torch.int32, device=dev)

    def seed(self, peer: int, ip: str, port: int):
        """the configured endpoint of a peer (PeerState::new(p.endpoint)), stored before the first call"""
        import numpy as np
        import torch

        row = np.frombuffer(row_bytes(ip, port), np.uint8).copy()
        self.endpoints[peer] = torch.from_numpy(row).to(self.endpoints.device)

    def rows(self):
        """the rows as host bytes, one per peer (waits for the device)"""
        return [r.tobytes() for r in self.endpoints.cpu().numpy()]

    # ------------------------------------------------------------------ notes
    def note_recv_batch_dev(self, slot_peer, key_idx, status, src, stream=None):
        """rg_endpoint_note_recv_batch_dev: behind the resident receive and in front of the route check, with its
        key_idx_out (uint32) and status (uint8); src uint8 [n][24], one rg_src_addr per packet."""
        n = _nbytes(status)
        assert _nbytes(key_idx) >= 4 * n and _nbytes(src) >= ADDR_BYTES * n
        e = self.engine
        e._check(e.library.rg_endpoint_note_recv_batch_dev(
            e.handle, _vp(self.endpoints), self.npeers, _vp(slot_peer), _nbytes(slot_peer) // 4, _vp(key_idx),
            _vp(status), _vp(src), n, _vp(self.claim), _stream_handle(stream)), "rg_endpoint_note_recv_batch_dev")

    def note_peers_batch_dev(self, peer_idx, status, src, stream=None):
        """rg_endpoint_note_peers_batch_dev: the same with the peer of item i named by peer_idx (uint32)."""
        n = _nbytes(status)
        assert _nbytes(peer_idx) >= 4 * n and _nbytes(src) >= ADDR_BYTES * n
        e = self.engine
        e._check(e.library.rg_endpoint_note_peers_batch_dev(
            e.handle, _vp(self.endpoints), self.npeers, _vp(peer_idx), _vp(status), _vp(src), n, _vp(self.claim),
            _stream_handle(stream)), "rg_endpoint_note_peers_batch_dev")

    def note_finish_batch_dev(self, pend_idx_out, pend_peers, status, src, stream=None):
        """rg_endpoint_note_finish_batch_dev: behind handshake_finish_dev, with its pend_idx_out and status;
        pend_peers uint32 [npending] names the peer of each pending row."""
        n = _nbytes(status)
        assert _nbytes(pend_idx_out) >= 4 * n and _nbytes(src) >= ADDR_BYTES * n
        e = self.engine
        e._check(e.library.rg_endpoint_note_finish_batch_dev(
            e.handle, _vp(self.endpoints), self.npeers, _vp(pend_idx_out), _vp(pend_peers), _nbytes(pend_peers) // 4,
            _vp(status), _vp(src), n, _vp(self.claim), _stream_handle(stream)), "rg_endpoint_note_finish_batch_dev")

    # ---------------------------------------------------------------- gathers
    def gate_batch_dev(self, slot_peer, slots, slots_out, dst_out, stream=None):
        """rg_endpoint_gate_batch_dev: in front of a resident send; slots / slots_out uint32 [n] (may be one
        tensor), dst_out uint8 [n][24]."""
        n = _nbytes(slots) // 4
        assert _nbytes(slots_out) >= 4 * n and _nbytes(dst_out) >= ADDR_BYTES * n
        e = self.engine
        e._check(e.library.rg_endpoint_gate_batch_dev(
            e.handle, _vp(self.endpoints), self.npeers, _vp(slot_peer), _nbytes(slot_peer) // 4, _vp(slots), n,
            _vp(slots_out), _vp(dst_out), _stream_handle(stream)), "rg_endpoint_gate_batch_dev")

    def peers_batch_dev(self, peer_idx, peers_out, dst_out, stream=None):
        """rg_endpoint_peers_batch_dev: the same by peer, RG_PEER_NONE for a peer without an endpoint."""
        n = _nbytes(peer_idx) // 4
        assert _nbytes(peers_out) >= 4 * n and _nbytes(dst_out) >= ADDR_BYTES * n
        e = self.engine
        e._check(e.library.rg_endpoint_peers_batch_dev(
            e.handle, _vp(self.endpoints), self.npeers, _vp(peer_idx), n, _vp(peers_out), _vp(dst_out),
            _stream_handle(stream)), "rg_endpoint_peers_batch_dev")
