"""The device-resident inbound demultiplexer over librg_aead (include/rg_aead.h, "device-resident inbound
demultiplexer"): the lists one mixed batch of datagrams is split into, the split, and the call that carries the
chains' verdicts back to the datagrams' own order.  As the rest of this package it serves the tests and the benchmark;
every call goes through the HIP library.

Reference -> this module
  recv_message's `match msg_type`  (rustyguard-core/src/lib.rs:605-630)  -> Demux.batch_dev
  recv_message's return value      (rustyguard-core/src/lib.rs:605-630)  -> Demux.verdict_batch_dev
"""
from __future__ import annotations

import ctypes

from . import _lib
from .aead import _nbytes, _ndesc, _stream_handle, _vp

DESC_BYTES = 16  # rg_pkt_desc
ADDR_BYTES = 24  # rg_src_addr
KEY_SKIP = 0xFFFFFFFF
INERT_DESC = bytes(12) + b"\xff" * 4  # {offset 0, len 0, RG_KEY_SKIP}


class ListsStruct(ctypes.Structure):
    """rg_demux_lists"""
    _fields_ = [("hs_desc", ctypes.c_void_p), ("hs_addrs", ctypes.c_void_p), ("init_desc", ctypes.c_void_p),
                ("resp_desc", ctypes.c_void_p), ("ck_desc", ctypes.c_void_p), ("data_desc", ctypes.c_void_p),
                ("data_addrs", ctypes.c_void_p), ("cap_hs", ctypes.c_uint32), ("cap_ck", ctypes.c_uint32),
                ("cap_data", ctypes.c_uint32)]


class Demux:
    """The three lists of rg_demux_batch_dev with capacities (cap_hs, cap_ck, cap_data) and the per-datagram outputs
    for batches of up to n datagrams, on the engine's device: hs_desc / init_desc / resp_desc uint8 [cap_hs][16],
    hs_addrs uint8 [cap_hs][24], ck_desc uint8 [cap_ck][16], data_desc uint8 [cap_data][16], data_addrs uint8
    [cap_data][24]; status / cls uint8 [n], pos int32 [n], counts int32 [6] (rank of hs, ck, data, then seen)."""

    def __init__(self, engine, n: int, cap_hs: int, cap_ck: int, cap_data: int, device=None):
        import torch

        dev = device if device is not None else f"cuda:{engine.device}"
        self.engine, self.n = engine, n
        self.cap_hs, self.cap_ck, self.cap_data = cap_hs, cap_ck, cap_data
        z = lambda rows, width: torch.zeros((rows, width), dtype=torch.uint8, device=dev)  # noqa: E731
        self.hs_desc, self.init_desc, self.resp_desc = (z(cap_hs, DESC_BYTES) for _ in range(3))
        self.hs_addrs = z(cap_hs, ADDR_BYTES)
        self.ck_desc = z(cap_ck, DESC_BYTES)
        self.data_desc, self.data_addrs = z(cap_data, DESC_BYTES), z(cap_data, ADDR_BYTES)
        self.status = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.cls = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.pos = torch.zeros(n, dtype=torch.int32, device=dev)
        self.counts = torch.zeros(6, dtype=torch.int32, device=dev)
        self.workspace = workspace(engine, n, dev)

    def lists(self) -> ListsStruct:
        p = lambda t: t.data_ptr() if t.numel() else None  # noqa: E731
        return ListsStruct(p(self.hs_desc), p(self.hs_addrs), p(self.init_desc), p(self.resp_desc), p(self.ck_desc),
                           p(self.data_desc), p(self.data_addrs), self.cap_hs, self.cap_ck, self.cap_data)

    def batch_dev(self, desc, addrs, buf, stream=None):
        """rg_demux_batch_dev: desc uint8 [n][16] and addrs uint8 [n][24], one row per datagram in arrival order."""
        n = _ndesc(desc)
        assert n <= self.n and _nbytes(addrs) >= ADDR_BYTES * n
        e = self.engine
        lists = self.lists()
        e._check(e.library.rg_demux_batch_dev(
            e.handle, _vp(desc), _vp(addrs), n, _vp(buf), _nbytes(buf), ctypes.byref(lists), _vp(self.status),
            _vp(self.cls), _vp(self.pos), _vp(self.counts), _vp(self.workspace), _nbytes(self.workspace),
            _stream_handle(stream)), "rg_demux_batch_dev")
        return n

    def verdict_batch_dev(self, n: int, hs_filter_status=None, init_status=None, finish_status=None,
                          cookie_status=None, data_status=None, stream=None):
        """rg_demux_verdict_batch_dev over the first n datagrams: each chain's status array (uint8, one per row of
        its list) or None for a chain that did not run."""
        for t, cap in ((hs_filter_status, self.cap_hs), (init_status, self.cap_hs), (finish_status, self.cap_hs),
                       (cookie_status, self.cap_ck), (data_status, self.cap_data)):
            assert t is None or _nbytes(t) >= cap
        e = self.engine
        e._check(e.library.rg_demux_verdict_batch_dev(
            e.handle, _vp(self.cls), _vp(self.pos), n, _vp(hs_filter_status), _vp(init_status), _vp(finish_status),
            self.cap_hs, _vp(cookie_status), self.cap_ck, _vp(data_status), self.cap_data, _vp(self.status),
            _stream_handle(stream)), "rg_demux_verdict_batch_dev")


def workspace(engine, n: int, device=None):
    """The scratch tensor (uint8) rg_demux_batch_dev needs for n datagrams (rg_demux_workspace_size)."""
    import torch

    size = int(engine.library.rg_demux_workspace_size(n))
    if size == 0:
        raise _lib.RgError(f"no workspace can hold a batch of {n} datagrams")
    return torch.empty(size, dtype=torch.uint8, device=device if device is not None else f"cuda:{engine.device}")
