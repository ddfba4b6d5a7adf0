"""The device-resident session timers over librg_aead (include/rg_aead.h, "device-resident session timers"): one
rg_session_timer row beside every row of a session.SessionTables, the three calls that keep the rows behind an
install, a send and a receive, and the turn that lists the keepalives and rekeys that are due.  As the rest of this
package it serves the tests and the benchmark; every call goes through the HIP library.

Reference -> this module
  handle_handshake_resp's RekeyAttempt push  (rustyguard-core/src/handshake.rs:218-222) -> arm_batch_dev
  send_message past REKEY_AFTER_MESSAGES     (rustyguard-core/src/lib.rs:564-570)       -> note_send_batch_dev
  decrypt_packet's keepalive flag            (:664-669)                                 -> note_recv_batch_dev
  tick_timers                                (rustyguard-core/src/time.rs:42-140)       -> turn_dev
"""
from __future__ import annotations

import ctypes

from . import _lib
from .aead import _nbytes, _stream_handle, _vp
from .session import _tables

TIMER_BYTES = 16  # rg_session_timer
KEEPALIVE_PENDING = 1
KEEPALIVE_TIMEOUT_NS = 10 * 10**9
REKEY_AFTER_TIME_NS = 120 * 10**9
REJECT_AFTER_TIME_NS = 180 * 10**9


class TimerStruct(ctypes.Structure):
    """rg_session_timer"""
    _fields_ = [("rekey_at_ns", ctypes.c_uint64), ("flags", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


def timer_rows(engine, nkeys: int, device=None):
    """nkeys zeroed rg_session_timer rows (uint8 [nkeys][16]) on the engine's device: nothing armed"""
    import torch

    return torch.zeros((nkeys, TIMER_BYTES), dtype=torch.uint8,
                       device=device if device is not None else f"cuda:{engine.device}")


def timer_workspace(engine, nkeys: int, npeers: int, device=None):
    """The scratch tensor (uint8, on the engine's device) the turn needs (rg_timer_workspace_size)."""
    import torch

    size = int(engine.library.rg_timer_workspace_size(nkeys, npeers))
    if size == 0:
        raise _lib.RgError(f"no workspace can hold a turn over {nkeys} rows and {npeers} peers")
    return torch.empty(size, dtype=torch.uint8, device=device if device is not None else f"cuda:{engine.device}")


def _nkeys(timers):
    return _nbytes(timers) // TIMER_BYTES


def arm_batch_dev(engine, timers, rows, gate, now_ns, rekey_after_ns: int, stream=None):
    """rg_timer_arm_batch_dev: behind an install, with its rows_out (uint32) and status (as gate, uint8 or None);
    rekey_after_ns REKEY_AFTER_TIME_NS for sessions we initiated, 0 for sessions we responded to."""
    n = _nbytes(rows) // 4
    assert gate is None or _nbytes(gate) >= n
    engine._check(engine.library.rg_timer_arm_batch_dev(
        engine.handle, _vp(timers), _nkeys(timers), _vp(rows), _vp(gate), n, _vp(now_ns), rekey_after_ns,
        _stream_handle(stream)), "rg_timer_arm_batch_dev")


def note_send_batch_dev(engine, timers, slots, status, rekey_out, now_ns, stream=None):
    """rg_timer_note_send_batch_dev: behind a resident or routed send, with its slots, status and rekey_out."""
    n = _nbytes(status)
    assert _nbytes(slots) >= 4 * n and _nbytes(rekey_out) >= n
    engine._check(engine.library.rg_timer_note_send_batch_dev(
        engine.handle, _vp(timers), _nkeys(timers), _vp(slots), _vp(status), _vp(rekey_out), n, _vp(now_ns),
        _stream_handle(stream)), "rg_timer_note_send_batch_dev")


def note_recv_batch_dev(engine, timers, send_state, key_idx, status, now_ns, stream=None):
    """rg_timer_note_recv_batch_dev: behind the resident receive, with its key_idx_out and status."""
    n = _nbytes(status)
    assert _nbytes(key_idx) >= 4 * n and _nbytes(send_state) >= 24 * _nkeys(timers)
    engine._check(engine.library.rg_timer_note_recv_batch_dev(
        engine.handle, _vp(timers), _vp(send_state), _nkeys(timers), _vp(key_idx), _vp(status), n, _vp(now_ns),
        _stream_handle(stream)), "rg_timer_note_recv_batch_dev")


def turn_dev(engine, tables, timers, now_ns, ka_slots_out, rekey_peers_out, rekey_gate_out, counts_out, workspace=None,
             stream=None):
    """rg_timer_turn_dev: ka_slots_out / rekey_peers_out uint32 [npeers], rekey_gate_out uint8 [npeers],
    counts_out uint32 [2].  Returns the workspace used."""
    assert _nkeys(timers) >= tables.nkeys and _nbytes(counts_out) >= 8
    assert all(_nbytes(t) >= 4 * tables.npeers for t in (ka_slots_out, rekey_peers_out))
    assert _nbytes(rekey_gate_out) >= tables.npeers
    if workspace is None:
        workspace = timer_workspace(engine, tables.nkeys, tables.npeers)
    engine._check(engine.library.rg_timer_turn_dev(
        engine.handle, _tables(tables), _vp(timers), _vp(now_ns), _vp(ka_slots_out), _vp(rekey_peers_out),
        _vp(rekey_gate_out), _vp(counts_out), _vp(workspace), _nbytes(workspace), _stream_handle(stream)),
        "rg_timer_turn_dev")
    return workspace
