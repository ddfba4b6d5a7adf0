"""The device-resident session table over librg_aead (include/rg_aead.h, "device-resident session table"): the
arrays the resident send, receive and route calls take, allocated together, and the calls that install finished
handshakes into them and expire sessions out of them on the device.  As the rest of this package it serves the
tests and the benchmark; every call goes through the HIP library.

Reference -> this module
  the tail of handle_handshake_init    (rustyguard-core/src/handshake.rs:110-133) -> install_resp_batch_dev
  the tail of handle_handshake_resp    (:201-227)                                 -> install_finish_batch_dev
  the ExpireTransport timer            (rustyguard-core/src/time.rs:84-98)        -> expire_batch_dev
"""
from __future__ import annotations

import ctypes

from . import _lib
from .aead import _nbytes, _stream_handle, _vp

PKT_FULL = 10
WINDOW_BYTES = 264  # rg_antireplay
STATE_BYTES = 24  # rg_send_state


class TablesStruct(ctypes.Structure):
    """rg_session_tables"""
    _fields_ = [(name, ctypes.c_void_p) for name in ("send_keys", "recv_keys", "receivers", "local_ids", "slot_peer",
                                                     "windows", "send_state", "rx_table", "peer_slot")] + \
               [(name, ctypes.c_uint32) for name in ("nkeys", "rx_cap", "npeers")]


ARRAYS = tuple(name for name, _ in TablesStruct._fields_[:9])


def rx_capacity(nkeys: int) -> int:
    """the smallest rx_cap the calls take for nkeys rows"""
    cap = 2
    while cap < 2 * nkeys:
        cap <<= 1
    return cap


class SessionTables:
    """An empty table of nkeys rows for npeers peers on the engine's device: one uint8 / int32 tensor per array of
    rg_session_tables (the word arrays are int32 tensors holding the uint32 bits), rx_table of rx_cap (receiver,
    key_idx) rows."""

    def __init__(self, engine, nkeys: int, npeers: int, rx_cap: int | None = None, device=None):
        import torch

        dev = device if device is not None else f"cuda:{engine.device}"
        self.nkeys, self.npeers = nkeys, npeers
        self.rx_cap = rx_capacity(nkeys) if rx_cap is None else rx_cap
        z8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
        ff = lambda *shape: torch.full(shape, -1, dtype=torch.int32, device=dev)  # noqa: E731
        self.send_keys, self.recv_keys = z8(nkeys, 32), z8(nkeys, 32)
        self.receivers = torch.zeros(nkeys, dtype=torch.int32, device=dev)
        self.local_ids = torch.zeros(nkeys, dtype=torch.int32, device=dev)
        self.slot_peer = ff(nkeys)
        self.windows, self.send_state = z8(nkeys, WINDOW_BYTES), z8(nkeys, STATE_BYTES)
        self.rx_table = ff(self.rx_cap, 2)
        self.peer_slot = ff(npeers)

    def struct(self) -> TablesStruct:
        t = TablesStruct()
        for name in ARRAYS:
            setattr(t, name, getattr(self, name).data_ptr())
        t.nkeys, t.rx_cap, t.npeers = self.nkeys, self.rx_cap, self.npeers
        return t


def _tables(tables):
    return ctypes.byref(tables if isinstance(tables, TablesStruct) else tables.struct())


def session_workspace(engine, n: int, nkeys: int, npeers: int, device=None):
    """The scratch tensor (uint8, on the engine's device) the session calls need (rg_session_workspace_size)."""
    import torch

    size = int(engine.library.rg_session_workspace_size(n, nkeys, npeers))
    if size == 0:
        raise _lib.RgError(f"no workspace can hold a batch of {n} handshakes")
    return torch.empty(size, dtype=torch.uint8, device=device if device is not None else f"cuda:{engine.device}")


def _workspace(engine, tables, n, workspace):
    return session_workspace(engine, n, tables.nkeys, tables.npeers) if workspace is None else workspace


def install_batch_dev(engine, tables, gate, local_ids, remote_ids, peers, transport_keys, status, rows_out, now_ns=None,
                      workspace=None, stream=None):
    """rg_session_install_batch_dev: one handshake per row of status (uint8); gate uint8 or None, local_ids /
    remote_ids / peers / rows_out uint32, transport_keys [n][64] (zeroed by the call), now_ns a device tensor
    holding one uint64 or None.  Returns the workspace used."""
    n = _nbytes(status)
    assert _nbytes(transport_keys) >= 64 * n and _nbytes(rows_out) >= 4 * n
    assert all(_nbytes(t) >= 4 * n for t in (local_ids, remote_ids, peers)) and (gate is None or _nbytes(gate) >= n)
    workspace = _workspace(engine, tables, n, workspace)
    engine._check(engine.library.rg_session_install_batch_dev(
        engine.handle, _tables(tables), _vp(gate), _vp(local_ids), _vp(remote_ids), _vp(peers), _vp(transport_keys), n,
        _vp(now_ns), _vp(status), _vp(rows_out), _vp(workspace), _nbytes(workspace), _stream_handle(stream)),
        "rg_session_install_batch_dev")
    return workspace


def install_resp_batch_dev(engine, tables, gate, session_ids, results, transport_keys, status, rows_out, now_ns=None,
                           workspace=None, stream=None):
    """rg_session_install_resp_batch_dev: behind handshake_resp_dev, with its session_ids, results, transport_keys
    and status (as gate)."""
    n = _nbytes(status)
    assert _nbytes(transport_keys) >= 64 * n and _nbytes(rows_out) >= 4 * n and _nbytes(results) >= 128 * n
    assert _nbytes(session_ids) >= 4 * n and (gate is None or _nbytes(gate) >= n)
    workspace = _workspace(engine, tables, n, workspace)
    engine._check(engine.library.rg_session_install_resp_batch_dev(
        engine.handle, _tables(tables), _vp(gate), _vp(session_ids), _vp(results), _vp(transport_keys), n, _vp(now_ns),
        _vp(status), _vp(rows_out), _vp(workspace), _nbytes(workspace), _stream_handle(stream)),
        "rg_session_install_resp_batch_dev")
    return workspace


def install_finish_batch_dev(engine, tables, gate, pend_idx_out, remote_out, pend_session_ids, pend_peers,
                             transport_keys, status, rows_out, now_ns=None, workspace=None, stream=None):
    """rg_session_install_finish_batch_dev: behind handshake_finish_dev, with its pend_idx_out, remote_out,
    transport_keys and status (as gate) and the session_ids / peer_idx arrays the initiate call was given."""
    n = _nbytes(status)
    npending = _nbytes(pend_session_ids) // 4
    assert _nbytes(transport_keys) >= 64 * n and _nbytes(rows_out) >= 4 * n and _nbytes(pend_peers) >= 4 * npending
    assert _nbytes(pend_idx_out) >= 4 * n and _nbytes(remote_out) >= 4 * n and (gate is None or _nbytes(gate) >= n)
    workspace = _workspace(engine, tables, n, workspace)
    engine._check(engine.library.rg_session_install_finish_batch_dev(
        engine.handle, _tables(tables), _vp(gate), _vp(pend_idx_out), _vp(remote_out), _vp(pend_session_ids),
        _vp(pend_peers), npending, _vp(transport_keys), n, _vp(now_ns), _vp(status), _vp(rows_out), _vp(workspace),
        _nbytes(workspace), _stream_handle(stream)), "rg_session_install_finish_batch_dev")
    return workspace


def expire_batch_dev(engine, tables, now_ns=None, rows=None, expired_out=None, workspace=None, stream=None):
    """rg_session_expire_batch_dev: rows past REJECT_AFTER_TIME at *now_ns (None: no time rule) and the rows named
    in `rows` (uint32, None: none) leave the table; expired_out (uint8, one per row, optional)."""
    m = 0 if rows is None else _nbytes(rows) // 4
    assert expired_out is None or _nbytes(expired_out) >= tables.nkeys
    workspace = _workspace(engine, tables, 0, workspace)
    engine._check(engine.library.rg_session_expire_batch_dev(
        engine.handle, _tables(tables), _vp(now_ns), _vp(rows), m, _vp(expired_out), _vp(workspace),
        _nbytes(workspace), _stream_handle(stream)), "rg_session_expire_batch_dev")
    return workspace


def index_dev(engine, tables, stream=None):
    """rg_session_index_dev: rx_table rebuilt from local_ids / slot_peer."""
    engine._check(engine.library.rg_session_index_dev(engine.handle, _tables(tables), _stream_handle(stream)),
                  "rg_session_index_dev")
