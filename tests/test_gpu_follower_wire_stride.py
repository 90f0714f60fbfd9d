"""qb_dev_ingest_follower past 2^20 messages: a base of 1031 messages laid end
to end K times (the tests/replicate.py idiom), so the grid passes one wave of
workgroups, the run counts' scan has hundreds of blocks and the copies start
anywhere in a tile.  The restatement runs on the base; every 1031-period
slice of every output is compared with it on the device (offsets shifted by k
times the base's bytes / runs)."""
import numpy as np
import pytest
import torch

from etcd_amd.quorum import wire
from tests import follower_wire_pack as P, follower_wire_ref as FW

pytestmark = pytest.mark.gpu
M0 = 1031
K = 1018
TILE, SCAN_BLOCK = 256, 4096


def test_base_laid_end_to_end():
    msgs, grp = P.base_batch(M0)
    buf, off = P.pack(msgs)
    want = FW.ingest(buf, len(buf), off, grp)
    P.assert_mixture(want, M0)
    M, L0, T0 = K * M0, len(buf), int(want["ent_total"])
    assert M > 1 << 20 and M0 % TILE and L0 % 16 and K * T0 > 64 * SCAN_BLOCK and K * L0 < 1 << 32
    dev = P.DEV
    ar = torch.arange(K, dtype=torch.int64, device=dev)[:, None]
    d_buf = P.dev(np.frombuffer(buf, np.uint8)).repeat(K)
    d_off = torch.cat([(P.dev(off)[:M0] + ar * L0).reshape(-1),
                       torch.tensor([K * L0], dtype=torch.int64, device=dev)])
    d_grp = P.dev(np.array(grp, np.uint32)).repeat(K)
    stats = torch.zeros(FW.STATUS_COUNT, dtype=torch.int64, device=dev)
    got = wire.ingest_follower(d_buf, K * L0, d_off, d_grp, P.G, ent_cap=K * T0, stats=stats)
    torch.cuda.synchronize()
    ib, app = got.inbox, got.app
    cols = {"group": ib.group, "flags": ib.flags, "frm": ib.frm, "term": ib.term, "index": ib.index,
            "aux": ib.aux, "commit": app.commit, "status": got.status, "msg_type": got.msg_type,
            "ent_bytes": got.ent_bytes, "ent_n": got.ent_n}
    for name, t in cols.items():
        assert torch.equal(t[:M].view(K, M0), P.dev(want[name]).expand(K, M0)), name
    has = P.dev((want["ent_bytes"] != 0).astype(np.uint64))
    assert torch.equal(got.ent_pos.view(K, M0), P.dev(want["ent_pos"]) + has * ar * L0)
    assert torch.equal(app.ent_off[:M].view(K, M0).to(torch.int64),
                       P.dev(want["ent_off"])[:M0].to(torch.int64) + ar * T0)
    assert int(app.ent_off[M]) == K * T0 == int(got.ent_total[0])
    flat = [x for r in want["runs"] for x in r]
    assert len(flat) == T0
    assert torch.equal(app.ent_term[:K * T0].view(K, T0),
                       P.dev(np.array([t for t, _ in flat], np.uint64)).expand(K, T0))
    assert torch.equal(app.ent_len[:K * T0].view(K, T0),
                       P.dev(np.array([n for _, n in flat], np.uint32)).expand(K, T0))
    assert np.array_equal(stats.cpu().numpy().view(np.uint64), want["stats"] * np.uint64(K))
