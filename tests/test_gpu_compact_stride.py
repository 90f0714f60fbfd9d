"""qb_dev_log_compact where every workgroup takes a second trip: a base of 1031
groups laid end to end K times (tests/replicate.py's per-kind functions), so
the reference runs on the base only and the expectation is a few numpy calls.
The list's order crosses the copies, and the last copy holds groups past the
cap.  At K = 509 (2050 tiles) qb_scan.h's scan is one block of 4096 tile
counts and never takes its second level; K = 1018, the smallest number of
whole copies with more than 4096 tiles, does.  Bit-exact: cmflags, the list
and what lies behind it, the count, every state column and the stats."""
import functools

import numpy as np
import pytest
import torch

from etcd_amd.quorum._dev import to_np
from tests import compact_dev as D, compact_pack as P, compact_ref as R, replicate as X

pytestmark = pytest.mark.gpu
G0 = 1031
TILE = 256          # groups per tile (qb_compact.hip: a thread per group, kBlock threads)
GRID_CAP = 2048     # kStreamBlocks (qb_span_tile.h): the most workgroups a launch has
SCAN_BLOCK = 4096   # tile counts per first-level scan block (qb_scan.h kScanPer)
HELD_BACK = 5       # acting groups past list_cap, all in the last copy
ROWS = ("run_start", "run_term")


def test_the_sizes_reach_the_second_trip_and_the_second_scan_level():
    assert 509 * G0 > GRID_CAP * TILE + TILE          # every workgroup strides to a second tile
    assert (509 * G0 + TILE - 1) // TILE <= SCAN_BLOCK  # ... on one scan block
    assert 1017 * G0 <= SCAN_BLOCK * TILE < 1018 * G0   # the smallest K with a second block


@functools.lru_cache(maxsize=None)
def base_run(mode, hold_back):
    """One copy through the reference, the last ``hold_back`` acting groups
    past the cap."""
    nodes = P.seeded_nodes(G0, 909)
    req = P.seeded_explicit(nodes, 910) if mode == R.CM_EXPLICIT else P.seeded_trigger(nodes, 911)
    before = P.pack_nodes(nodes)
    count = R.log_compact(R.clone(nodes), req, G0, R.new_stats()).count
    stats = R.new_stats()
    res = R.log_compact(nodes, req, count - hold_back, stats)
    assert res.count == count and len(res.records) == count - hold_back and count > G0 // 8
    return {"req": req, "before": before, "after": P.pack_nodes(nodes, base=before),
            "count": count, "flags": np.asarray(res.flags, np.uint16), "stats": stats,
            "list": {k: np.array([r[k] for r in res.records], dt) for k, dt in P.LIST.items()}}


def lay(copies, key):
    out = {}
    for k in P.STATE:
        cols = [c[key][k] for c in copies]
        out[k] = (X.rep_rows(cols, range(len(cols)), G0).reshape(-1) if k in ROWS
                  else X.rep_group(cols, range(len(cols))))
    return out


@pytest.mark.parametrize("mode", (R.CM_EXPLICIT, R.CM_TRIGGER), ids=("explicit", "trigger"))
@pytest.mark.parametrize("K", (509, 1018))
def test_log_compact_over_many_copies(K, mode):
    G = K * G0
    full, last = base_run(mode, 0), base_run(mode, HELD_BACK)
    copies = [full] * (K - 1) + [last]
    count = K * full["count"]
    cap = count - HELD_BACK
    ds = D.DeviceState(lay(copies, "before"))
    req = full["req"]
    tiled = R.Request(req.mode, snapshot_count=req.snapshot_count,
                      catch_up_entries=req.catch_up_entries,
                      **{k: (None if getattr(req, k) is None else np.tile(getattr(req, k), K))
                         for k in ("snap_at", "compact_at", "force", "hold")})
    out = D.poisoned_result(G, cap + 3)
    res = ds.compact(D.device_request(tiled, G), cap, out=out)
    torch.cuda.synchronize()
    assert res.count() == count
    assert np.array_equal(res.flags(), np.concatenate([c["flags"] for c in copies]))
    for k, dt in P.LIST.items():
        want = [c["list"][k] for c in copies]
        if k == "gid":
            want = [w + np.uint32(c * G0) for c, w in enumerate(want)]
        got = to_np(res.cols[k], dt)
        assert np.array_equal(got[:cap], np.concatenate(want)), k
        assert (got[cap:] == D.POISON).all(), k          # nothing behind the cap
    want_stats = {k: sum(c["stats"][k] for c in copies) for k in R.STAT_NAMES}
    assert res.stats_dict() == want_stats
    assert want_stats["deferred"] == HELD_BACK and want_stats["listed"] == cap
    D.assert_state(ds.numpy(), lay(copies, "after"), f"K={K}")
