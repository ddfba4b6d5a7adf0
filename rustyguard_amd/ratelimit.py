"""The device-resident handshake rate limiter over librg_aead (include/rg_aead.h, "device-resident handshake rate
limiter"): the responder's count-min sketch over source addresses, allocated together, the call that counts a batch
of handshake messages and hands the under-load filter its overload flags, and the turn that wipes and reseeds the
sketch once its period has passed.  As the rest of this package it serves the tests and the benchmark; every call
goes through the HIP library.

Reference -> this module
  DynamicState::overloaded, count_min_sketch.count (rustyguard-core/src/lib.rs:508-514) -> count_dev
  the rate-limiter reset of Sessions::turn         (rustyguard-core/src/lib.rs:406-408) -> turn_dev
"""
from __future__ import annotations

import ctypes

from . import _lib
from .aead import _nbytes, _stream_handle, _vp

RATE_WIDTH = 5437
RATE_DEPTH = 5
RATE_LIMIT = 10
RATE_MAX_DEPTH = 8
RATE_PERIOD_NS = 10**9
SEED_BYTES = 16  # rg_rate_seed
ADDR_BYTES = 24  # rg_src_addr


class RateSeedStruct(ctypes.Structure):
    """rg_rate_seed"""
    _fields_ = [("a", ctypes.c_uint64), ("b", ctypes.c_uint64)]


class RateTablesStruct(ctypes.Structure):
    """rg_rate_tables"""
    _fields_ = [(name, ctypes.c_void_p) for name in ("buckets", "seeds", "last_reset_ns")] + \
               [(name, ctypes.c_uint32) for name in ("width", "depth")]


ARRAYS = tuple(name for name, _ in RateTablesStruct._fields_[:3])


class RateTables:
    """An empty sketch on the engine's device: buckets int32 [depth][width] zero, seeds uint8 [depth][16] (zero until
    the caller stores its CSPRNG's output or a turn resets), last_reset_ns int64 [1] zero."""

    def __init__(self, engine, width: int = RATE_WIDTH, depth: int = RATE_DEPTH, device=None):
        import torch

        dev = device if device is not None else f"cuda:{engine.device}"
        self.width, self.depth = width, depth
        self.buckets = torch.zeros((depth, width), dtype=torch.int32, device=dev)
        self.seeds = torch.zeros((depth, SEED_BYTES), dtype=torch.uint8, device=dev)
        self.last_reset_ns = torch.zeros(1, dtype=torch.int64, device=dev)

    def struct(self) -> RateTablesStruct:
        t = RateTablesStruct()
        for name in ARRAYS:
            setattr(t, name, getattr(self, name).data_ptr())
        t.width, t.depth = self.width, self.depth
        return t


def _tables(tables):
    return ctypes.byref(tables if isinstance(tables, RateTablesStruct) else tables.struct())


def column(seed, addr: bytes, width: int, library=None) -> int:
    """rg_rate_column: the column of the rg_src_addr `addr` (24 bytes) under seed = (a, b) in a row of `width`
    buckets, computed by the library on the host."""
    assert len(addr) == ADDR_BYTES
    s = RateSeedStruct(*seed)
    buf = ctypes.create_string_buffer(bytes(addr), ADDR_BYTES)
    return int((library or _lib.lib()).rg_rate_column(ctypes.byref(s), buf, width))


def workspace_size(engine, n: int, width: int = RATE_WIDTH, depth: int = RATE_DEPTH) -> int:
    """rg_rate_workspace_size: bytes of scratch for a count of n messages; 0 when a size is out of range"""
    return int(engine.library.rg_rate_workspace_size(n, width, depth))


def rate_workspace(engine, n: int, width: int = RATE_WIDTH, depth: int = RATE_DEPTH, device=None):
    """That scratch as a tensor (uint8, on the engine's device)."""
    import torch

    size = workspace_size(engine, n, width, depth)
    if size == 0:
        raise _lib.RgError(f"no workspace can hold {n} messages on a {depth} x {width} sketch")
    return torch.empty(size, dtype=torch.uint8, device=device if device is not None else f"cuda:{engine.device}")


def count_dev(engine, tables, desc, addrs, buf, overload_out, counts_out=None, limit: int = RATE_LIMIT, workspace=None,
              stream=None):
    """rg_rate_count_batch_dev: desc uint8 [n][16], addrs uint8 [n][24] and buf as cookie_reply_dev takes them;
    overload_out uint8 [n] (the filter's `overload`), counts_out uint32 [n] or None.  Returns the workspace used."""
    n = _nbytes(overload_out)
    assert _nbytes(desc) >= 16 * n and _nbytes(addrs) >= ADDR_BYTES * n
    assert counts_out is None or _nbytes(counts_out) >= 4 * n
    if workspace is None:
        workspace = rate_workspace(engine, n, tables.width, tables.depth)
    engine._check(engine.library.rg_rate_count_batch_dev(
        engine.handle, _tables(tables), _vp(desc), _vp(addrs), n, _vp(buf), _nbytes(buf), limit, _vp(counts_out),
        _vp(overload_out), _vp(workspace), _nbytes(workspace), _stream_handle(stream)), "rg_rate_count_batch_dev")
    return workspace


def turn_dev(engine, tables, now_ns, new_seeds, reset_out, period_ns: int = RATE_PERIOD_NS, stream=None):
    """rg_rate_turn_dev: now_ns a device tensor holding one uint64, new_seeds uint8 [depth][16] (the caller's CSPRNG
    output, consumed only on a reset), reset_out uint32 [1]."""
    assert _nbytes(new_seeds) >= SEED_BYTES * tables.depth and _nbytes(reset_out) >= 4
    engine._check(engine.library.rg_rate_turn_dev(
        engine.handle, _tables(tables), _vp(now_ns), period_ns, _vp(new_seeds), _vp(reset_out),
        _stream_handle(stream)), "rg_rate_turn_dev")
