"""qb_dev_log_compact on the device against tests/compact_ref.py, bit for bit:
every state column, cmflags, the list (pre-filled, so a record the call must
not touch shows), list_count and every counter (tests/compact_dev.py does the
comparing).  The reference's own cases, a seeded batch over two tiles in both
modes with every (run count, runs dropped) pair built in, a second call on the
result, one group, an idle call, the cap, and the trigger's rules."""
import numpy as np
import pytest

from tests import compact_dev as D, compact_pack as P, compact_ref as R
from tests.test_compact_ref import CASES, node_of

pytestmark = pytest.mark.gpu
G_FUZZ = 300   # two tiles of 256, the second partial


def test_golden_cases_through_the_wrapper():
    """Every case of compact_tables.json as one group of a batch; call j
    carries each case's step j (a case with fewer steps idles)."""
    run = D.Run([node_of(c) for c in CASES])
    for j in range(max(len(c["steps"]) for c in CASES)):
        s, c = [0] * run.G, [0] * run.G
        for g, case in enumerate(CASES):
            if j < len(case["steps"]):
                st = case["steps"][j]
                (s if st["op"] == "snapshot" else c)[g] = st["i"]
        run.call(R.Request(R.CM_EXPLICIT, snap_at=s, compact_at=c), where=f"golden step {j}")
    # what the reference's tests expect of the storage, on the device's columns
    a = run.ds.numpy()
    for g, case in enumerate(CASES):
        want = case["steps"][-1]["want"]
        if "first" in want:
            assert int(a["first_index"][g]) == want["first"], case["name"]
        if "index" in want and case["steps"][-1]["err"] is None:
            row0 = [int(a[k].reshape(-1)[g]) for k in ("run_start", "run_term")]   # run-major
            assert row0 == [want["index"], want["term"]], case["name"]


def structured_nodes():
    """For every run count n and every k < n two groups whose compaction
    index lies in run k: on its start (behind the dummy entry for k = 0) and
    on its last entry, one before the next start — stable_last for k = n - 1.
    Everything stable and applied."""
    nodes, cs = [], []
    for n in range(1, R.MAX_RUNS + 1):
        ents = [(100 + i, 1 + i // 3) for i in range(3 * n)]
        for k in range(n):
            for c in (max(100 + 3 * k, 101), 100 + 3 * k + 2):
                nodes.append(R.Node(list(ents), 100 + 3 * n, 100 + 3 * n - 1))
                cs.append(c)
    return nodes, cs


def fuzz_batch(seed):
    sn, sc = structured_nodes()
    nodes = sn + P.seeded_nodes(G_FUZZ - len(sn), seed)
    assert len(nodes) == G_FUZZ
    counts = np.bincount([len(R.runs(n.ents)) for n in nodes], minlength=9)
    assert (counts[1:] >= 20).all(), counts          # run counts 1..8, evenly
    return nodes, sc


def cap_below(nodes, req, below):
    """The cap that defers the last ``below`` acting groups (found on a copy)."""
    return R.log_compact(R.clone(nodes), req, len(nodes), R.new_stats()).count - below


def test_fuzz_explicit_then_again():
    nodes, sc = fuzz_batch(11)
    req = P.seeded_explicit(nodes, 12)
    req.compact_at[:len(sc)] = sc
    for g in range(len(sc)):
        req.snap_at[g] = sc[g] - 1 if g % 3 == 0 else 0
    run = D.Run(nodes, meta_rest=np.random.default_rng(3).integers(0, 1 << 32, G_FUZZ, dtype=np.uint64))
    before = [len(R.runs(n.ents)) for n in run.nodes[:len(sc)]]
    run.call(req, cap_below(nodes, req, 3), where="explicit")
    # on the reference alone: every k of every run count, every path, every counter
    dropped = {(b, b - len(R.runs(n.ents))) for b, n in zip(before, run.nodes[:len(sc)])}
    assert dropped == {(n, k) for n in range(1, 9) for k in range(n)}
    st = dict(run.stats)
    assert all(v > 0 for k, v in st.items() if k != "held"), st
    assert st["held"] == 0 and st["deferred"] == 3
    # the same request on the result: what was done is refused as done
    ref = run.call(req, where="explicit again")
    again = {k: run.stats[k] - st[k] for k in st}
    assert again["already_compacted"] > st["already_compacted"], again
    assert again["snap_out_of_date"] > st["snap_out_of_date"], again
    assert again["listed"] == 3 and ref.count == 3      # the three that were deferred


def test_fuzz_trigger_then_again():
    nodes, _ = fuzz_batch(23)
    req = P.seeded_trigger(nodes, 24)
    run = D.Run(nodes)
    run.call(req, cap_below(nodes, req, 2), where="trigger")
    st = dict(run.stats)
    for k in ("snapped", "compacted", "snap_out_of_date", "already_compacted", "held",
              "pending_snapshot", "bad_log", "deferred", "listed", "entries_dropped", "runs_dropped"):
        assert st[k] > 0, (k, st)
    ref = run.call(req, where="trigger again")
    # a group that snapped at applied no longer triggers, held or not: the
    # second call acts on the two deferred groups and on nothing else
    assert ref.count == 2 and run.stats["listed"] == st["listed"] + 2
    assert run.stats["snap_out_of_date"] == 2 * st["snap_out_of_date"]


def test_one_group():
    n = R.Node([(i, 1 + i // 2) for i in range(5, 12)], 12, 9, 5, 3)
    run = D.Run([n])
    ref = run.call(R.Request(R.CM_EXPLICIT, snap_at=[9], compact_at=[8]))
    assert ref.flags == [R.SNAPPED | R.COMPACTED]
    assert ref.records == [{"gid": 0, "flags": 3, "snap_index": 9, "snap_term": 5,
                            "compact_index": 8, "first_before": 6}]
    ref = run.call(R.Request(R.CM_EXPLICIT, snap_at=[9], compact_at=[8]))
    assert ref.flags == [R.SNAP_OUT_OF_DATE | R.ALREADY_COMPACTED]


@pytest.mark.parametrize("req", [
    R.Request(R.CM_EXPLICIT), R.Request(R.CM_EXPLICIT, snap_at=[0] * G_FUZZ),
    R.Request(R.CM_EXPLICIT, compact_at=[0] * G_FUZZ),
    R.Request(R.CM_TRIGGER, snapshot_count=(1 << 64) - 1, catch_up_entries=0),
    R.Request(R.CM_TRIGGER, snapshot_count=(1 << 64) - 1, force=[0] * G_FUZZ, hold=[1] * G_FUZZ)],
    ids=["null-columns", "null-compact", "null-snap", "count-max", "force-zero"])
def test_an_idle_call_changes_no_state_byte(req):
    nodes, _ = fuzz_batch(31)
    run = D.Run(nodes)
    before = {k: v.copy() for k, v in run.ds.numpy().items()}
    ref = run.call(req, where="idle")
    assert not any(ref.flags) and ref.count == 0 and not any(run.stats.values())
    D.assert_state(run.ds.numpy(), before, "idle")


@pytest.mark.parametrize("cap", [0, 1, -1])
def test_the_cap_defers_and_deferred_groups_are_untouched(cap):
    nodes, sc = fuzz_batch(41)
    req = P.seeded_explicit(nodes, 42)
    req.compact_at[:len(sc)] = sc
    probe = R.log_compact(R.clone(nodes), req, len(nodes), R.new_stats())
    acting = np.flatnonzero(np.asarray(probe.flags) & (R.SNAPPED | R.COMPACTED))
    listed = probe.count
    assert acting[0] < 256 <= acting[-2]       # acting groups in both tiles
    cap = listed - 1 if cap < 0 else cap
    run = D.Run(nodes)
    before = run.ds.numpy()
    ref = run.call(req, cap, where=f"cap {cap}")
    deferred = np.flatnonzero(np.asarray(ref.flags) & R.DEFERRED)
    assert len(deferred) == listed - cap and ref.count == listed and len(ref.records) == cap
    after = run.ds.numpy()
    for k in P.STATE:                           # bit-identical to their state before
        b, a = before[k].reshape(-1, run.G), after[k].reshape(-1, run.G)
        assert np.array_equal(b[:, deferred], a[:, deferred]), k


def test_trigger_rules_on_the_device():
    """force, hold, applied < snap_index (the wrapped subtraction), and
    catch_up_entries above and below applied."""
    ents = [(i, 1 + i // 4) for i in range(0, 21)]
    mk = lambda applied, snapi: R.Node(list(ents), 21, applied, snapi, 1 if snapi else 0)  # noqa: E731
    nodes = [mk(10, 8), mk(10, 8), mk(10, 10), mk(10, 12), mk(10, 0), mk(3, 0), mk(10, 0)]
    run = D.Run(nodes)
    ref = run.call(R.Request(R.CM_TRIGGER, snapshot_count=5, catch_up_entries=4,
                             force=[0, 255, 1, 0, 0, 0, 0], hold=[0, 0, 0, 0, 0, 0, 7]))
    assert ref.flags == [0, R.SNAPPED | R.COMPACTED, 0, R.SNAP_OUT_OF_DATE, R.SNAPPED | R.COMPACTED,
                         0, R.SNAPPED | R.HELD]
    assert [n.first_index for n in run.nodes] == [1, 7, 1, 1, 7, 1, 1]
    # catch_up_entries above applied: compact at 1; NULL force / hold
    run = D.Run([mk(3, 0), mk(10, 0)])
    ref = run.call(R.Request(R.CM_TRIGGER, snapshot_count=2, catch_up_entries=4))
    assert ref.flags == [R.SNAPPED | R.COMPACTED] * 2
    assert [n.first_index for n in run.nodes] == [2, 7]
    assert [r["compact_index"] for r in ref.records] == [1, 6]
