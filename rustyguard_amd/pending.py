"""The device-resident pending handshakes over librg_aead (include/rg_aead.h, "device-resident pending
handshakes"): the initiator's table of handshakes in flight, one row a peer, allocated together, the call that puts
the initiator chain's pending rows into it, and the turn that retries, expires and merges the requests for new
handshakes into the one list the chain takes.  As the rest of this package it serves the tests and the benchmark;
every call goes through the HIP library.

Reference -> this module
  the tail of new_handshake                (rustyguard-core/src/handshake.rs:266-297) -> install_dev
  the InitAttempt and ExpireHandshake arms (rustyguard-core/src/time.rs:49-83, 99-113) -> turn_dev
"""
from __future__ import annotations

import ctypes

from . import _lib
from .aead import _nbytes, _stream_handle, _vp
from .session import rx_capacity

PENDING_BYTES = 128  # rg_hs_pending
TIMER_BYTES = 16  # rg_pending_timer
PEER_WORD, SENDER_WORD = 24, 25  # of a pending row's 32 words
REKEY_TIMEOUT_NS = 5 * 10**9
REKEY_ATTEMPT_TIME_NS = 90 * 10**9
PEER_NONE = 0xFFFFFFFF


class PendingTimerStruct(ctypes.Structure):
    """rg_pending_timer"""
    _fields_ = [("started_ns", ctypes.c_uint64), ("sent_ns", ctypes.c_uint64)]


class PendingTablesStruct(ctypes.Structure):
    """rg_pending_tables"""
    _fields_ = [(name, ctypes.c_void_p) for name in ("pending", "timers", "hs_ids", "pend_table")] + \
               [(name, ctypes.c_uint32) for name in ("npeers", "pend_cap")]


ARRAYS = tuple(name for name, _ in PendingTablesStruct._fields_[:4])


class PendingTables:
    """An empty table for npeers peers on the engine's device: pending uint8 [npeers][128] zeroed with peer =
    RG_PEER_NONE, timers uint8 [npeers][16] and hs_ids int32 [npeers] zero, pend_table int32 [pend_cap][2] all ones;
    peers is the constant 0..npeers-1 that rg_session_install_finish_batch_dev takes as pend_peers."""

    def __init__(self, engine, npeers: int, pend_cap: int | None = None, device=None):
        import torch

        dev = device if device is not None else f"cuda:{engine.device}"
        self.npeers = npeers
        self.pend_cap = rx_capacity(npeers) if pend_cap is None else pend_cap
        self.pending = torch.zeros((npeers, PENDING_BYTES), dtype=torch.uint8, device=dev)
        self.pending[:, 4 * PEER_WORD:4 * PEER_WORD + 4] = 0xFF
        self.timers = torch.zeros((npeers, TIMER_BYTES), dtype=torch.uint8, device=dev)
        self.hs_ids = torch.zeros(npeers, dtype=torch.int32, device=dev)
        self.pend_table = torch.full((self.pend_cap, 2), -1, dtype=torch.int32, device=dev)
        self.peers = torch.arange(npeers, dtype=torch.int32, device=dev)

    def struct(self) -> PendingTablesStruct:
        t = PendingTablesStruct()
        for name in ARRAYS:
            setattr(t, name, getattr(self, name).data_ptr())
        t.npeers, t.pend_cap = self.npeers, self.pend_cap
        return t


def _tables(tables):
    return ctypes.byref(tables if isinstance(tables, PendingTablesStruct) else tables.struct())


def workspace_size(engine, n: int, m: int, npeers: int) -> int:
    """rg_pending_workspace_size: bytes of scratch for an install of n rows (m = 0) or a turn with m requests
    (n = 0); 0 when a size is too large"""
    return int(engine.library.rg_pending_workspace_size(n, m, npeers))


def pending_workspace(engine, n: int, m: int, npeers: int, device=None):
    """That scratch as a tensor (uint8, on the engine's device)."""
    import torch

    size = workspace_size(engine, n, m, npeers)
    if size == 0:
        raise _lib.RgError(f"no workspace can hold {n} rows, {m} requests and {npeers} peers")
    return torch.empty(size, dtype=torch.uint8, device=device if device is not None else f"cuda:{engine.device}")


def index_dev(engine, tables, stream=None):
    """rg_pending_index_dev: pend_table rebuilt from the live rows."""
    engine._check(engine.library.rg_pending_index_dev(engine.handle, _tables(tables), _stream_handle(stream)),
                  "rg_pending_index_dev")


def install_dev(engine, tables, batch, gate, now_ns, status, installed_out, workspace=None, stream=None):
    """rg_pending_install_batch_dev: behind handshake_initiate_dev, with its pending rows (batch, uint8 [n][128],
    wiped by the call) and status (as gate, uint8 or None); now_ns a device tensor holding one uint64, status uint8
    [n], installed_out uint32 [n].  Returns the workspace used."""
    n = _nbytes(status)
    assert _nbytes(batch) >= PENDING_BYTES * n and _nbytes(installed_out) >= 4 * n and (gate is None or _nbytes(gate) >= n)
    if workspace is None:
        workspace = pending_workspace(engine, n, 0, tables.npeers)
    engine._check(engine.library.rg_pending_install_batch_dev(
        engine.handle, _tables(tables), _vp(batch), _vp(gate), n, _vp(now_ns), _vp(status), _vp(installed_out),
        _vp(workspace), _nbytes(workspace), _stream_handle(stream)), "rg_pending_install_batch_dev")
    return workspace


def turn_dev(engine, tables, now_ns, init_peers_out, init_gate_out, counts_out, start_peers=None, start_status=None,
             start_match: int = 0, expired_out=None, workspace=None, stream=None):
    """rg_pending_turn_dev: init_peers_out uint32 [npeers], init_gate_out uint8 [npeers], counts_out uint32 [2],
    expired_out uint8 [npeers] or None; start_peers uint32 [m] with start_status uint8 [m] or None: the requests,
    those whose status equals start_match (all without start_status).  Returns the workspace used."""
    m = 0 if start_peers is None else _nbytes(start_peers) // 4
    assert _nbytes(init_peers_out) >= 4 * tables.npeers and _nbytes(init_gate_out) >= tables.npeers
    assert _nbytes(counts_out) >= 8 and (expired_out is None or _nbytes(expired_out) >= tables.npeers)
    assert start_status is None or _nbytes(start_status) >= m
    if workspace is None:
        workspace = pending_workspace(engine, 0, m, tables.npeers)
    engine._check(engine.library.rg_pending_turn_dev(
        engine.handle, _tables(tables), _vp(now_ns), _vp(start_peers), _vp(start_status), start_match, m,
        _vp(init_peers_out), _vp(init_gate_out), _vp(expired_out), _vp(counts_out), _vp(workspace),
        _nbytes(workspace), _stream_handle(stream)), "rg_pending_turn_dev")
    return workspace
