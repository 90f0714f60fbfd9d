"""qb_dev_encode_* where every workgroup of the write pass takes a second
trip and where the offsets' scan runs its second level: a base of 1031
messages laid end to end K times (the tests/replicate.py idiom), so the
restatement runs on the base and the expectation is the base's bytes repeated,
the offsets shifted by k times the base's total.  The copies are laid out and
compared on the device."""
import functools

import numpy as np
import pytest
import torch

from etcd_amd.quorum import encode
from tests import encode_pack as P, encode_ref as E

pytestmark = pytest.mark.gpu
M0 = 1031
TILE = 256          # messages per tile of the write pass (qb_encode.hip)
GRID_CAP = 2048     # kStreamBlocks (qb_span_tile.h): the most workgroups a launch has
SCAN_BLOCK = 4096   # lengths per first-level scan block (qb_scan.h kScanPer)
K_TRIPS = 509
K_SCAN = 16274
FILL64 = 0x5A5A5A5A5A5A5A5A


def test_the_sizes_reach_the_second_trip_and_the_second_scan_level():
    assert K_TRIPS * M0 > GRID_CAP * TILE + TILE     # every workgroup strides to a second tile
    assert K_SCAN * M0 > SCAN_BLOCK * SCAN_BLOCK     # the block sums' scan loops (1024 a pass)
    assert K_SCAN * M0 * encode.ENC_MAX_BYTES < 1 << 32
    assert M0 % TILE and M0 % 16                     # copies start anywhere in a tile


@functools.lru_cache(maxsize=None)
def base(sparse):
    """The base's columns and its layout by the restatement; ``sparse``: all
    but every 29th message has type 0 (no bytes)."""
    for seed in range(9, 40):    # the first seed whose total is odd: the copies' spans
        cols = {k: v[:M0].copy() for k, v in P.column_batch(M0 + 1, seed=seed).items()}
        if sparse:               # then start at every residue mod 16
            cols["type"][np.arange(M0) % 29 != 3] = 0
        recs = E.columns(cols, M0)
        want = E.finish(recs)
        if want["nbytes"] % 2:
            break
    assert {st for st, _ in recs} >= ({E.OK, E.NONE} if sparse else {E.OK, E.ENTRIES, E.HOST, E.NONE})
    assert want["nbytes"] % 2
    return cols, want


@pytest.mark.parametrize("K,sparse", ((K_TRIPS, False), (K_SCAN, True)),
                         ids=("second trip", "second scan level"))
def test_columns_laid_end_to_end(K, sparse):
    cols, want = base(sparse)
    M, L0 = K * M0, int(want["nbytes"])
    d = {k: t[:M0].repeat(K) for k, t in P.cols_dev(cols).items()}
    fill = lambda n, dt: torch.full((n * torch.empty(0, dtype=dt).element_size(),), P.FILL,  # noqa: E731
                                    dtype=torch.uint8, device=P.DEV).view(dt)
    out = encode.EncodeOut(fill(K * L0 + 64, torch.uint8)[1:], K * L0, fill(M + 2, torch.int64),
                           fill(M + 1, torch.uint8), fill(M + 1, torch.int32), fill(1, torch.int64),
                           torch.zeros(5, dtype=torch.int64, device=P.DEV))
    encode.encode_columns(d, M=M, out=out)
    torch.cuda.synchronize()
    assert int(out.nbytes[0]) == K * L0
    wb = P.dev(want["bytes"])[:L0]
    assert torch.equal(out.bytes[:K * L0].view(K, L0), wb.expand(K, L0))
    assert bool((out.bytes[K * L0:] == P.FILL).all())
    shift = torch.arange(K, dtype=torch.int64, device=P.DEV)[:, None] * L0
    assert torch.equal(out.msg_off[:M].view(K, M0), P.dev(want["msg_off"])[:M0] + shift)
    assert int(out.msg_off[M]) == K * L0 and int(out.msg_off[M + 1]) == FILL64
    assert torch.equal(out.status[:M].view(K, M0), P.dev(want["status"]).expand(K, M0))
    assert int(out.status[M]) == P.FILL
    at = np.where(want["ent_at"] >= 0, want["ent_at"], 0x5A5A5A5A).astype(np.uint32)
    assert torch.equal(out.ent_at[:M].view(K, M0), P.dev(at).expand(K, M0))
    assert np.array_equal(out.stats.cpu().numpy().view(np.uint64), want["stats"] * np.uint64(K))


def test_slots_laid_end_to_end():
    """The slot front end past the second trip: the group table K times, slot
    offsets shifted by k times the base's slots."""
    G0, off, ids, self_id, term = P.group_table()
    sc = P.slot_columns()
    S0 = int(off[-1])
    K = GRID_CAP * TILE // S0 + 2
    assert K * S0 > GRID_CAP * TILE + TILE
    cols = {"commit": sc["commit"][:S0], "ctx_g": sc["ctx_g"]}
    want = E.finish(E.slots(G0, off, ids, self_id, term, S0, sc["gflags"], 2, E.MSG_HEARTBEAT, cols))
    L0, S = int(want["nbytes"]), K * S0
    off_k = (off[:-1].astype(np.int64)[None, :] + S0 * np.arange(K)[:, None]).reshape(-1)
    off_k = np.concatenate([off_k, [S]]).astype(np.uint32)
    rep = lambda a: P.dev(a).repeat(K)  # noqa: E731
    g = encode.EncodeGroups(P.dev(off_k), rep(ids), rep(self_id), rep(term), S)
    b, moff, st, at, nb = encode.encode_slots(
        g, gflags=rep(sc["gflags"]), gmask=2,
        cols={"commit": rep(cols["commit"]), "ctx_g": rep(cols["ctx_g"])})
    torch.cuda.synchronize()
    assert int(nb[0]) == K * L0
    assert torch.equal(b[:K * L0].view(K, L0), P.dev(want["bytes"])[:L0].expand(K, L0))
    shift = torch.arange(K, dtype=torch.int64, device=P.DEV)[:, None] * L0
    assert torch.equal(moff[:S].view(K, S0), P.dev(want["msg_off"])[:S0] + shift)
    assert torch.equal(st.view(K, S0), P.dev(want["status"]).expand(K, S0))
