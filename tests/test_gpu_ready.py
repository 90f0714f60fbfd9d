"""qb_dev_ready, qb_dev_advance and qb_dev_unstable_truncate on the device
against tests/ready_ref.py, bit-exact after every call: rflags, the list (the
records, and behind them the pre-filled elements a call must leave alone),
*ready_count, aflags, every column of the state and the accumulated stats.  All
comparisons are integer equality."""
import copy
import importlib
import json
import os

import numpy as np
import pytest
import torch

from tests import ready_pack as P, ready_ref as R

qy = importlib.import_module("etcd_amd.quorum.ready")  # (the package exports the function ready)

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 256  # groups per workgroup trip (qb_ready.hip)
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE + 1, 3 * TILE + 7)
FRACS = ("none", "some", "all")
CAPS = lambda G: (G // 3, G, G // 2)  # noqa: E731  (the list's size, call after call)


def signed(v, dt):
    return np.array([v], dt).view({np.uint64: np.int64, np.uint32: np.int32, np.uint16: np.int16,
                                   np.uint8: np.uint8}[dt])[0].item()


class DeviceRun:
    """A batch of nodes on the device beside its reference copy."""

    def __init__(self, nodes, cap=None, ext=True):
        self.nodes = nodes
        self.G = len(nodes)
        a = P.pack_nodes(nodes)
        if not ext:
            a["ext"] = None
        self.state = qy.ReadyState.from_numpy(a, device=DEV)
        self.stats = dict.fromkeys(R.RSTAT_NAMES, 0)
        self.astats = dict.fromkeys(R.ASTAT_NAMES, 0)
        self.astat_t = torch.zeros(len(R.ASTAT_NAMES), dtype=torch.int64, device=DEV)
        self.new_out(self.G if cap is None else cap)

    def new_out(self, cap):
        """Output buffers pre-filled with a marker (the stats keep counting)."""
        full = lambda n, dt: torch.full((max(n, 1),), signed(P._FILLS[dt], dt),  # noqa: E731
                                        dtype=qy._TORCH[dt], device=DEV)
        stats = self.out.stats if hasattr(self, "out") else torch.zeros(
            len(R.RSTAT_NAMES), dtype=torch.int64, device=DEV)
        self.out = qy.ReadyResult(cap, full(self.G, np.uint16),
                                  {k: full(cap, dt) for k, dt in P.LIST.items()},
                                  full(1, np.uint64), stats)

    def check_state(self, where):
        want = P.pack_nodes(self.nodes)
        got = self.state.numpy()
        for k in got:
            assert np.array_equal(got[k], want[k]), (where, k)

    def ready(self, accept, cap=None, where=""):
        """One call on both sides, everything compared; returns the records."""
        cap = self.out.ready_cap if cap is None else cap
        self.new_out(cap)
        rflags, records, count, st = R.ready_call(self.nodes, accept, cap)
        for k, v in st.items():
            self.stats[k] += v
        qy.ready(self.state, accept=accept, out=self.out)
        torch.cuda.synchronize()
        assert self.out.count() == count, where
        got_rf = self.out.rflags.cpu().numpy().view(np.uint16)
        want_rf = np.array(rflags, np.uint16) if self.G else np.full(1, P.FILL16, np.uint16)
        assert np.array_equal(got_rf, want_rf), (where, "rflags")
        want = P.pack_records(records, cap)
        for k, dt in P.LIST.items():
            got = self.out.cols[k].cpu().numpy().view(dt)
            assert np.array_equal(got, want[k]), (where, k)
        assert self.out.stats_dict() == self.stats, where
        self.check_state(where)
        return records

    def advance(self, recs, where=""):
        aflags, st = R.advance_call(self.nodes, recs)
        for k, v in st.items():
            self.astats[k] += v
        A = len(recs)
        out = qy.AdvanceResult(torch.full((max(A, 1),), 0xA5, dtype=torch.uint8, device=DEV),
                               self.astat_t)
        qy.advance(self.state, qy.AdvanceRecords.from_numpy(P.pack_advance(recs), device=DEV),
                   out=out)
        torch.cuda.synchronize()
        want = np.array(aflags, np.uint8) if A else np.full(1, 0xA5, np.uint8)
        assert np.array_equal(out.aflags.cpu().numpy(), want), (where, "aflags")
        assert out.stats_dict() == self.astats, where
        self.check_state(where)
        return aflags


def cycle_nodes(G, frac, seed):
    nodes = P.seeded_nodes(G, frac, seed)
    if frac == "all" and G >= 64:
        nodes[8:24] = P.auto_leave_nodes(np.random.default_rng(seed + 1), 16)
    return nodes


def test_fuzz_inputs_reach_every_flag_and_stat():
    """On the CPU: the inputs of the tests below make the reference produce
    every QB_RDF_* bit, every QB_AFLAG_* bit and a non-zero value of every
    stat, so no bit goes untested unnoticed."""
    rf_seen = af_seen = 0
    rst = dict.fromkeys(R.RSTAT_NAMES, 0)
    ast = dict.fromkeys(R.ASTAT_NAMES, 0)
    for G in SIZES:
        for fi, frac in enumerate(FRACS):
            nodes = cycle_nodes(G, frac, 1000 + 7 * G + fi)
            rng = np.random.default_rng(G + fi)
            for cap in CAPS(G):
                rflags, records, _, st = R.ready_call(nodes, True, cap)
                aflags, st2 = R.advance_call(nodes, P.advance_records(nodes, records, rng))
                for k, v in st.items():
                    rst[k] += v
                for k, v in st2.items():
                    ast[k] += v
                for f in rflags:
                    rf_seen |= f
                for f in aflags:
                    af_seen |= f
    assert rf_seen == 0x3FF, hex(rf_seen)
    assert af_seen == 0x0F, hex(af_seen)
    assert all(v > 0 for v in rst.values()), rst
    assert all(v > 0 for v in ast.values()), ast


@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("G", sorted(set(SIZES)))
def test_ready_advance_cycle_fuzz(G, frac):
    """Ready (accepting) -> Advance with a host's departures -> Ready again
    with half the list -> Advance -> Ready, on seeded groups."""
    fi = FRACS.index(frac)
    run = DeviceRun(cycle_nodes(G, frac, 1000 + 7 * G + fi))
    rng = np.random.default_rng(G + fi)
    for r_, cap in enumerate(CAPS(G)):
        records = run.ready(True, cap, where=f"ready {r_}")
        run.advance(P.advance_records(run.nodes, records, rng), where=f"advance {r_}")
    run.ready(True, G, where="last ready")


def test_no_groups_sets_the_count_and_touches_nothing():
    run = DeviceRun([])
    assert run.ready(True, 0) == []
    assert run.ready(False, 5) == []


@pytest.mark.parametrize("frac", ("some", "all"))
def test_ready_cap_defers_and_the_next_call_lists(frac):
    """ready_cap in {0, 1, count - 1, count, G}: the groups past it are
    flagged, not listed and not accepted; a second call lists them."""
    G = 3 * TILE + 7
    base = cycle_nodes(G, frac, 77)
    count = R.ready_call(copy.deepcopy(base), False, G)[2]
    assert count >= 2
    for cap in (0, 1, count - 1, count, G):
        run = DeviceRun(copy.deepcopy(base))
        first = run.ready(True, cap, where=f"cap {cap}")
        assert len(first) == min(cap, count)
        deferred = sum(1 for f in R.ready_call(copy.deepcopy(base), False, cap)[0]
                       if f & R.RDF_DEFERRED)
        assert deferred == count - min(cap, count)
        second = run.ready(True, G, where=f"cap {cap}, second call")
        listed = {r.gid for r in first} | {r.gid for r in second}
        assert listed == {r.gid for r in R.ready_call(copy.deepcopy(base), False, G)[1]}


@pytest.mark.parametrize("frac", FRACS)
def test_accept_zero_writes_no_state(frac):
    G = 3 * TILE + 7
    run = DeviceRun(cycle_nodes(G, frac, 31))
    before = {k: v.copy() for k, v in run.state.numpy().items()}
    for cap in (G, 5):
        run.ready(False, cap, where=f"accept 0, cap {cap}")
        after = run.state.numpy()
        for k, v in before.items():
            assert v.tobytes() == after[k].tobytes(), k
    run.ready(True, G, where="the accepting call after")  # the same groups are still there


def test_without_ext_nothing_auto_leaves():
    G = 300
    nodes = cycle_nodes(G, "all", 5)
    for n in nodes:
        n.auto_leave = False
    run = DeviceRun(nodes, ext=False)
    records = run.ready(True)
    flags = run.advance(P.advance_records(run.nodes, records, np.random.default_rng(1)))
    assert not any(f & R.AFLAG_AUTO_LEAVE for f in flags)


@pytest.mark.parametrize("order", ("descending", "shuffled"))
@pytest.mark.parametrize("A", (0, 1, 65, "G"))
def test_advance_in_any_order(A, order):
    """A records in descending and shuffled group order, with every flag."""
    G = 3 * TILE + 7
    run = DeviceRun(cycle_nodes(G, "all", 91))
    records = run.ready(True)
    assert len(records) == G
    rng = np.random.default_rng(3)
    recs = P.advance_records(run.nodes, records, rng)
    recs = recs[:G if A == "G" else A]
    if order == "descending":
        recs = recs[::-1]
    else:
        recs = [recs[i] for i in rng.permutation(len(recs))]
    flags = run.advance(recs, where=f"A {A} {order}")
    if A == "G":
        seen = 0
        for f in flags:
            seen |= f
        assert seen == 0x0F
    run.ready(True, where="ready after advance")


def test_truncate_fold_many_records_on_one_group():
    """unstable.truncateAndAppend's offset, folded in any order: thousands of
    records on one group, records of absent groups, and app_from == 0."""
    G = 300
    run = DeviceRun(cycle_nodes(G, "some", 13))
    rng = np.random.default_rng(17)
    M = 5000
    group = rng.integers(0, G + 3, M).astype(np.uint32)
    group[:3000] = 7
    app_from = rng.integers(0, 40, M).astype(np.uint64)
    app_from[rng.integers(0, M, 500)] = 0
    R.truncate_fold(run.nodes, group.tolist(), app_from.tolist())
    qy.unstable_truncate(run.state, torch.from_numpy(group.view(np.int32)).to(DEV),
                         torch.from_numpy(app_from.view(np.int64)).to(DEV))
    torch.cuda.synchronize()
    run.check_state("truncate fold")
    assert run.nodes[7].offset <= int(app_from[:3000][app_from[:3000] != 0].min())
    run.ready(True, where="ready after the fold")
    qy.unstable_truncate(run.state, torch.zeros(1, dtype=torch.int32, device=DEV),
                         torch.zeros(1, dtype=torch.int64, device=DEV), M=0)
    run.check_state("M == 0")


def golden_cases():
    with open(os.path.join(ROOT, "tests", "golden", "ready_tables.json"), encoding="utf-8") as f:
        return json.load(f)


def test_golden_tables_on_the_device():
    """Every node state of the reference's tables as one batch: the device's
    Ready equals the reference restatement's (which tests/test_ready_ref.py
    holds to the tables' expected values), and so does the Advance."""
    from tests.test_ready_ref import table_nodes
    nodes = table_nodes(golden_cases())
    assert len(nodes) > 40
    run = DeviceRun(nodes)
    records = run.ready(False, where="golden, HasReady")
    records = run.ready(True, where="golden, Ready")
    run.advance([R.record_of(r) for r in records], where="golden, Advance")
    run.ready(True, where="golden, Ready after Advance")
