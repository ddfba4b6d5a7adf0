"""The flattened kernel (family 3) on a batch whose last group of 1024 packets is short: with 1024 units, packet
2048 of 2049 lies behind the last unit's nominal start, and no wave took it (its status stayed as the caller left
it).  Seal against the oracle, then open back to the plaintext, every status written."""
import numpy as np
import pytest
import torch

from oracle import oracle
from rustyguard_amd.workloads import DESC_DTYPE

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [1025, 2049, 4097, 4099])
def test_short_last_group(engine, n):
    rng = np.random.default_rng(n)
    keys = rng.integers(0, 256, (2, 32), dtype=np.uint8)
    recv = np.array([0xAAAA, 0xBBBB], np.uint32)
    sizes = rng.choice((0, 16, 64), n)
    desc = np.zeros(n, DESC_DTYPE)
    desc["offset"] = np.concatenate([[0], np.cumsum(sizes[:-1] + 32)])
    desc["len"] = sizes
    desc["key_idx"] = rng.integers(0, 2, n)
    buf = rng.integers(0, 256, int(sizes.sum()) + 32 * n, dtype=np.uint8)
    ctr = rng.integers(0, 1 << 62, n).astype(np.uint64)
    want = buf.copy()
    oracle.seal_batch(keys, recv, desc, ctr, want)
    dk, dr = torch.from_numpy(keys).cuda(), torch.from_numpy(recv.view(np.int32)).cuda()
    dd = torch.from_numpy(desc.view(np.uint8).reshape(-1, 16).copy()).cuda()
    dc = torch.from_numpy(ctr.view(np.int64)).cuda()
    db = torch.from_numpy(buf.copy()).cuda()
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    engine.set_staged(3)
    try:
        engine.seal_dev(dk, dr, dd, dc, db, st)
        torch.cuda.synchronize()
        assert engine.last_kernel() == 3
        assert not st.cpu().numpy().any(), np.nonzero(st.cpu().numpy())[0][:10]
        assert np.array_equal(db.cpu().numpy(), want)
        od = desc.copy()
        od["len"] += 32
        st.fill_(0xEE)
        out = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        engine.open_dev(dk, torch.from_numpy(od.view(np.uint8).reshape(-1, 16).copy()).cuda(), db, st, out)
        torch.cuda.synchronize()
        assert not st.cpu().numpy().any() and np.array_equal(out.cpu().numpy().view(np.uint64), ctr)
    finally:
        engine.set_staged(-1)
    got = db.cpu().numpy()
    for i in (0, n - 2, n - 1):  # payloads are plaintext again
        o, p = int(desc["offset"][i]) + 16, int(desc["len"][i])
        assert np.array_equal(got[o:o + p], buf[o:o + p])
