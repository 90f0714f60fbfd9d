"""tests/compact_ref.py against the reference's own tests
(tests/golden/compact_tables.json): each case replayed through the restated
MemoryStorage and, beside it, through the whole call in explicit mode, whose
flags must say what Go returned.  CPU only."""
import json
import os

import numpy as np
import pytest

from tests import compact_pack as P, compact_ref as R

with open(os.path.join(os.path.dirname(__file__), "golden", "compact_tables.json")) as f:
    TABLES = json.load(f)
CASES = [c for group in ("storage", "log", "raft") for c in TABLES[group]]


def expand(runs):
    return [(i, term) for start, term, count in runs for i in range(start, start + count)]


def node_of(case) -> R.Node:
    stable, unstable = expand(case["runs"]), expand(case["unstable"])
    return R.Node(stable + unstable, stable[-1][0] + 1, case["applied"], *case["snap"])


ERR_FLAG = {("snapshot", None): R.SNAPPED, ("compact", None): R.COMPACTED,
            ("snapshot", "ErrSnapOutOfDate"): R.SNAP_OUT_OF_DATE,
            ("compact", "ErrCompacted"): R.ALREADY_COMPACTED,
            ("snapshot", "panic"): R.OUT_OF_BOUND, ("compact", "panic"): R.OUT_OF_BOUND}


def check_want(want, ms: R.MemoryStorage, node: R.Node, snap):
    """``ms``: the storage; ``node``: the whole log (the raftLog's view)."""
    for k, v in want.items():
        if k == "index":
            assert ms.ents[0][0] == v
        elif k == "term":
            assert ms.ents[0][1] == v
        elif k == "len":
            assert len(ms.ents) == v
        elif k == "first":
            assert ms.first_index() == v
        elif k == "snap":
            assert list(snap) == v
        elif k == "left":
            assert len(node.ents) - 1 == v          # allEntries(): without the dummy
        elif k == "last_index":
            assert node.last_index == v
        elif k == "term_at":
            terms = dict(node.ents)
            assert [[i, terms[i]] for i, _ in v] == v
        elif k == "unstable":
            tail = [e for e in node.ents if e[0] >= node.unstable_offset]
            assert [len(tail), tail[0][0]] == v
        else:
            raise AssertionError(f"unknown check {k}")


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_case(case):
    node = node_of(case)                         # through the call
    ms, tail = R._storage_of(node)               # through the bare storage
    for st in case["steps"]:
        op, i, err = st["op"], st["i"], st["err"]
        snap = None
        try:
            if op == "snapshot":
                snap = ms.create_snapshot(i)
            else:
                ms.compact(i)
            got = None
        except R.ErrCompacted:
            got = "ErrCompacted"
        except R.ErrSnapOutOfDate:
            got = "ErrSnapOutOfDate"
        except R.Panic:
            got = "panic"
        assert got == err, (case["name"], st)
        req = R.Request(R.CM_EXPLICIT, snap_at=[i if op == "snapshot" else 0],
                        compact_at=[i if op == "compact" else 0])
        res = R.log_compact([node], req, 1, R.new_stats())
        assert res.flags[0] == ERR_FLAG[(op, err)], (case["name"], st, res.flags)
        assert node.ents == ms.ents + tail
        assert (node.snap_index, node.snap_term) == (ms.snap_index, ms.snap_term)
        check_want(st["want"], ms, node, snap)
        # the table derived from the entries is the packed one, and survives a round trip
        a = P.pack_nodes([node])
        back = P.unpack_nodes(a)[0]
        assert back.ents == node.ents and back.first_index == node.first_index


def test_golden_file_is_the_generators():
    """compact_tables.json is what make_compact_golden.py writes."""
    from tests.golden import make_compact_golden as M
    assert TABLES == json.loads(json.dumps({"storage": M.storage_tables(), "log": M.log_tables(),
                                            "raft": M.raft_tables()}))


def test_trigger_rules():
    """shouldSnapshot's two arms with the wrapped subtraction, the hold, and
    SnapshotCatchUpEntries above and below applied (server.go:1115-1117,
    2042-2051)."""
    ents = [(i, 1 + i // 4) for i in range(0, 21)]
    mk = lambda applied, snapi: R.Node(list(ents), 21, applied, snapi, 1 if snapi else 0)  # noqa: E731
    nodes = [mk(10, 8), mk(10, 8), mk(10, 10), mk(10, 12), mk(10, 0), mk(3, 0), mk(10, 0)]
    req = R.Request(R.CM_TRIGGER, snapshot_count=5, catch_up_entries=4,
                    force=[0, 1, 1, 0, 0, 0, 0], hold=[0, 0, 0, 0, 0, 0, 1])
    st = R.new_stats()
    res = R.log_compact(nodes, req, len(nodes), st)
    assert res.flags == [0,                                   # 10 - 8 <= 5, not forced
                         R.SNAPPED | R.COMPACTED,             # forced
                         0,                                   # forced, but applied == snapi
                         R.SNAP_OUT_OF_DATE,                  # 10 - 12 wraps above the count
                         R.SNAPPED | R.COMPACTED,
                         0,
                         R.SNAPPED | R.HELD]
    assert [n.first_index for n in nodes] == [1, 7, 1, 1, 7, 1, 1]     # compacted at 10 - 4
    assert nodes[1].snap_index == 10 and nodes[1].snap_term == 3
    low = [mk(3, 0)]
    R.log_compact(low, R.Request(R.CM_TRIGGER, snapshot_count=2, catch_up_entries=4), 1, st)
    assert low[0].first_index == 2 and low[0].snap_index == 3         # compacti = 1


def test_stops_change_nothing_and_the_cap_defers():
    ents = [(i, 1 + i // 4) for i in range(0, 21)]
    n = R.Node(list(ents), 15, 10)
    before = R.clone([n])[0]
    req = R.Request(R.CM_EXPLICIT, snap_at=[9], compact_at=[12])        # 12 > applied
    res = R.log_compact([n], req, 1, R.new_stats())
    assert res.flags == [R.PAST_APPLIED] and n == before
    req = R.Request(R.CM_EXPLICIT, snap_at=[9], compact_at=[15])        # 15 > stable_last
    assert R.log_compact([n], req, 1, R.new_stats()).flags == [R.OUT_OF_BOUND] and n == before
    nodes = [R.clone([before])[0] for _ in range(3)]
    st = R.new_stats()
    res = R.log_compact(nodes, R.Request(R.CM_EXPLICIT, snap_at=[9, 0, 9], compact_at=[9, 9, 0]), 2, st)
    assert res.flags == [R.SNAPPED | R.COMPACTED, R.COMPACTED, R.SNAPPED | R.DEFERRED]
    assert res.count == 3 and len(res.records) == 2 and nodes[2] == before
    assert st["listed"] == 2 and st["deferred"] == 1 and st["entries_dropped"] == 18
    assert st["runs_dropped"] == 4 and st["snapped"] == 2
    a = P.pack_nodes(nodes)
    assert list(a["first_index"]) == [10, 10, 1] and list((a["meta"] >> 16) & 0xF) == [4, 4, 6]
    assert np.array_equal(a["run_start"][:4, 0], [9, 12, 16, 20])
