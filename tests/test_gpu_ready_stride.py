"""qb_dev_ready and qb_dev_advance where every workgroup takes a second trip
and the tile-count scan its second level: a base of 1031 groups laid end to
end K times (tests/replicate.py's per-kind functions), so the reference runs
on 1031 groups and the expectation is a few numpy calls.  Bit-exact: rflags,
the list and what lies behind it, the count, aflags, every state column and
the stats."""
import copy
import functools
import importlib

import numpy as np
import pytest
import torch

from tests import ready_pack as P, ready_ref as R, replicate as X

qy = importlib.import_module("etcd_amd.quorum.ready")

pytestmark = pytest.mark.gpu
DEV = "cuda"
G0 = 1031
TILE = 256          # groups per tile (qb_ready.hip: a thread per group, kBlock threads)
GRID_CAP = 2048     # kStreamBlocks (qb_span_tile.h): the most workgroups a launch has
SCAN_BLOCK = 4096   # tile counts per first-level scan block (qb_scan.h kScanPer)
K = 1018
G = K * G0
HELD_BACK = 7       # ready groups past ready_cap, all in the last copy
ROWS = ("run_start", "run_term")


def test_the_sizes_reach_the_second_trip_and_the_second_scan_level():
    assert G > GRID_CAP * TILE + TILE      # every workgroup strides to a second tile
    assert G > SCAN_BLOCK * TILE           # more tile counts than one scan block holds


def signed(a):
    return a.view({np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32,
                   np.dtype(np.uint16): np.int16, np.dtype(np.uint8): np.uint8}[a.dtype])


@functools.lru_cache(maxsize=None)
def base_run(frac, hold_back):
    """One copy through Ready (accepting, the last ``hold_back`` ready groups
    past the cap) and Advance on the reference."""
    nodes = P.seeded_nodes(G0, frac, 4242)
    before = P.pack_nodes(nodes)
    count = R.ready_call(copy.deepcopy(nodes), False, G0)[2]
    rflags, records, count2, rstats = R.ready_call(nodes, True, count - hold_back)
    assert count2 == count and len(records) == count - hold_back
    after_ready = P.pack_nodes(nodes)
    recs = P.advance_records(nodes, records, np.random.default_rng(9))
    aflags, astats = R.advance_call(nodes, recs)
    return {"before": before, "count": count, "rflags": np.array(rflags, np.uint16),
            "list": {k: v[:len(records)] for k, v in P.pack_records(records, len(records)).items()},
            "rstats": rstats, "after_ready": after_ready, "adv": P.pack_advance(recs),
            "aflags": np.array(aflags, np.uint8), "astats": astats,
            "after_advance": P.pack_nodes(nodes)}


def lay(copies, key):
    """The K copies' state arrays laid end to end."""
    out = {}
    for k in P.DTYPES:
        cols = [c[key][k] for c in copies]
        out[k] = (X.rep_rows(cols, range(len(cols)), G0).reshape(-1) if k in ROWS
                  else X.rep_group(cols, range(len(cols))))
    return out


def shifted(copies, part, col):
    """A record column of every copy end to end; a group column gets its
    copy's offset (a group past the base stays past the whole batch)."""
    out = []
    for c, cp in enumerate(copies):
        a = cp[part][col]
        if col in ("ready_gid", "adv_gid"):
            a64 = a.astype(np.int64)
            a = np.where(a64 < G0, a64 + c * G0, a64 - G0 + G).astype(np.uint32)
        out.append(a)
    return np.concatenate(out)


@pytest.mark.parametrize("layout", ("every copy active", "all idle but the last three"))
def test_ready_and_advance_over_a_million_groups(layout):
    full, last, idle = base_run("all", 0), base_run("all", HELD_BACK), base_run("none", 0)
    assert idle["count"] == 0 and full["count"] > G0 // 2
    if layout == "every copy active":
        copies = [full] * (K - 1) + [last]
    else:
        copies = [idle] * (K - 3) + [full, full, last]
    count = sum(c["count"] for c in copies)
    cap = count - HELD_BACK
    state = qy.ReadyState.from_numpy(lay(copies, "before"), device=DEV)
    fill = lambda n, dt: torch.from_numpy(signed(np.full(max(n, 1), P._FILLS[dt], dt))).to(DEV)  # noqa: E731
    out = qy.ReadyResult(cap + 3, fill(G, np.uint16),
                         {k: fill(cap + 3, dt) for k, dt in P.LIST.items()}, fill(1, np.uint64),
                         torch.zeros(len(R.RSTAT_NAMES), dtype=torch.int64, device=DEV))
    qy.ready(state, accept=True, ready_cap=cap, out=out)
    torch.cuda.synchronize()
    assert out.count() == count
    assert np.array_equal(out.rflags.cpu().numpy().view(np.uint16),
                          np.concatenate([c["rflags"] for c in copies]))
    for k, dt in P.LIST.items():
        got = out.cols[k].cpu().numpy().view(dt)
        assert np.array_equal(got[:cap], shifted(copies, "list", k)), k
        assert (got[cap:] == P._FILLS[dt]).all(), k   # nothing behind the cap
    want_stats = {k: sum(c["rstats"][k] for c in copies) for k in R.RSTAT_NAMES}
    assert out.stats_dict() == want_stats
    assert want_stats["deferred"] == HELD_BACK and want_stats["listed"] == cap
    got = state.numpy()
    for k, w in lay(copies, "after_ready").items():
        assert np.array_equal(got[k], w), ("after ready", k)

    adv = {k: shifted(copies, "adv", k) for k in P.ADV}
    A = len(adv["adv_gid"])
    assert A == cap and (layout != "every copy active" or A > GRID_CAP * TILE + TILE)
    res = qy.AdvanceResult(torch.full((A,), 0xA5, dtype=torch.uint8, device=DEV),
                           torch.zeros(len(R.ASTAT_NAMES), dtype=torch.int64, device=DEV))
    qy.advance(state, qy.AdvanceRecords.from_numpy(adv, device=DEV), out=res)
    torch.cuda.synchronize()
    assert np.array_equal(res.aflags.cpu().numpy(), np.concatenate([c["aflags"] for c in copies]))
    assert res.stats_dict() == {k: sum(c["astats"][k] for c in copies) for k in R.ASTAT_NAMES}
    got = state.numpy()
    for k, w in lay(copies, "after_advance").items():
        assert np.array_equal(got[k], w), ("after advance", k)
