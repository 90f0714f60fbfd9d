"""qb_dev_follower_step on the device against tests/follower_ref.py,
bit-exact: every in/out array of the groups, resp_type, resp_term, stop_at,
gflags and every stat counter.  The outputs are pre-filled with 0xA5 bytes, so
an element the call must write and did not shows.  All comparisons are integer
equality."""
import ctypes as C

import numpy as np
import pytest
import torch

from etcd_amd import _lib
from etcd_amd.quorum import follower as qf, leader as ql, tick as qt
from tests import follower_pack as P, follower_ref as F

pytestmark = pytest.mark.gpu
DEV = "cuda"


def upload(nodes, recs, cfg):
    a = P.pack_nodes(nodes)
    state = qt.TickState.from_numpy(a["role"], a["election_elapsed"], a["heartbeat_elapsed"],
                                    np.zeros(len(nodes), np.uint32), device=DEV)
    fg = qf.FollowerGroups.from_numpy(a, state, cfg.election_timeout, cfg.check_quorum,
                                      cfg.pre_vote, device=DEV)
    r = P.pack_recs(recs)
    ib = qf.FollowerInbox.from_numpy(r["group"], r["flags"], r["from"], r["term"], r["index"],
                                     r["aux"], device=DEV)
    return fg, ib


def filled_result(G, M):
    need = qf.follower_workspace_bytes(G, M)
    return qf.FollowerResult(torch.full((max(M, 1),), 0xA5, dtype=torch.uint8, device=DEV),
                             torch.full((max(M, 1),), -1, dtype=torch.int64, device=DEV),
                             torch.full((max(G, 1),), 0x5A5A5A5A, dtype=torch.int32, device=DEV),
                             torch.full((max(G, 1),), 0xA5, dtype=torch.uint8, device=DEV),
                             torch.zeros(len(qf.FSTAT_NAMES), dtype=torch.int64, device=DEV),
                             torch.full(((need + 7) // 8,), -1, dtype=torch.int64, device=DEV))


def compare(where, fg, res, G, M, want_groups, want):
    got = fg.numpy()
    for k, w in want_groups.items():
        assert np.array_equal(got[k], w), (where, k, np.nonzero(got[k] != w)[0][:8])
    for k, dt, n in (("resp_type", np.uint8, M), ("resp_term", np.uint64, M),
                     ("stop_at", np.uint32, G), ("gflags", np.uint8, G)):
        g = ql._to_np(getattr(res, k), dt, n)
        assert np.array_equal(g, want[k]), (where, k, np.nonzero(g != want[k])[0][:8])
    assert res.stats_dict() == want["stats"], (where, res.stats_dict(), want["stats"])


def run(where, nodes, recs, cfg):
    """One call on the device beside follower_ref; returns the result."""
    G, M = len(nodes), len(recs)
    fg, ib = upload(nodes, recs, cfg)
    res = qf.follower_step(fg, ib, out=filled_result(G, M))
    want_groups, want = P.expected(nodes, recs, cfg)
    compare(where, fg, res, G, M, want_groups, want)
    res.groups_after = fg.numpy()
    return res, want


# --------------------------------------------------------- golden scenarios ---

SCENARIOS = P.load_tables()["scenarios"]


@pytest.mark.parametrize("sc", SCENARIOS, ids=[s["name"] for s in SCENARIOS])
def test_golden_scenario_on_device(sc):
    """The reference's tests, G = 1 each: the transcribed expectations hold
    for the device's responses and state, and the device equals follower_ref."""
    node = P.scenario_node(sc)
    recs = [(0, r) for r in P.scenario_recs(sc)]
    fg, ib = upload([node], recs, P.scenario_config(sc))
    res = qf.follower_step(fg, ib, out=filled_result(1, len(recs)))
    want_groups, want = P.expected([node], recs, P.scenario_config(sc))
    compare(sc["name"], fg, res, 1, len(recs), want_groups, want)
    after = F.Node(**{k: int(v[0]) for k, v in fg.numpy().items()})
    P.check_scenario(sc, ql._to_np(res.resp_type, np.uint8).tolist(),
                     ql._to_np(res.resp_term, np.uint64).tolist(), after)


def test_golden_scenarios_in_one_batch():
    """Scenarios with one configuration share a call: one group each, their
    records interleaved."""
    by_cfg = {}
    for sc in SCENARIOS:
        by_cfg.setdefault(tuple(sorted(sc["config"].items())), []).append(sc)
    assert sum(len(v) for v in by_cfg.values()) == len(SCENARIOS)
    rng = np.random.default_rng(7)
    for key, scs in by_cfg.items():
        nodes = [P.scenario_node(sc) for sc in scs]
        recs = P.interleave([P.scenario_recs(sc) for sc in scs], rng)
        res, _ = run(f"packed {key}", nodes, recs, P.scenario_config(scs[0]))
        rt = ql._to_np(res.resp_type, np.uint8)
        rterm = ql._to_np(res.resp_term, np.uint64)
        for g, sc in enumerate(scs):
            idx = [i for i, (gg, _) in enumerate(recs) if gg == g]
            after = F.Node(**{k: int(v[g]) for k, v in res.groups_after.items()})
            P.check_scenario(sc, rt[idx].tolist(), rterm[idx].tolist(), after)


# --------------------------------------------------------------------- fuzz ---

@pytest.mark.parametrize("cq,pv", P.FUZZ_CONFIGS)
@pytest.mark.parametrize("seed", P.FUZZ_SEEDS)
def test_fuzz(seed, cq, pv):
    """G = 1000, M = 5000 (tests/follower_pack.py fuzz; what it reaches is
    asserted in tests/test_follower_ref.py), under both settings of
    check_quorum and pre_vote."""
    nodes, recs = P.fuzz(seed)
    res, want = run(f"fuzz seed {seed} cq {cq} pv {pv}", nodes, recs, P.fuzz_config(cq, pv))
    # the mirror's message view: one dict per non-zero resp_type, in batch order
    msgs = list(res.responses())
    nz = np.flatnonzero(want["resp_type"])
    assert [m["i"] for m in msgs] == nz.tolist()
    for m in msgs[:200]:
        g, r = recs[m["i"]]
        assert m["to"] == r.frm and m["term"] == int(want["resp_term"][m["i"]])
        assert m["type"] | (0x80 if m["reject"] else 0) == int(want["resp_type"][m["i"]])
        assert m["context"] == (r.aux if m["type"] == qf.MSG_HEARTBEAT_RESP else 0)


# ------------------------------------------------------------------- shapes ---

def _hb_node(term=3):
    return F.Node(term=term, lead=1, committed=2, last_index=40, last_term=term,
                  role=F.FOLLOWER | F.ROLE_PROMOTABLE, election_elapsed=3, heartbeat_elapsed=2)


def test_one_group_no_records_and_one_record():
    cfg = F.Config(10, True, True)
    res, want = run("G1 M0", [_hb_node()], [], cfg)
    assert want["gflags"].tolist() == [0] and want["stop_at"].tolist() == [F.NO_STOP]
    res, want = run("G1 M1", [_hb_node()], [(0, F.Rec(F.HEARTBEAT, 1, 3, 7, 99))], cfg)
    assert want["resp_type"].tolist() == [F.MSG_HEARTBEAT_RESP]
    assert list(res.responses()) == [{"i": 0, "type": 9, "to": 1, "term": 3, "reject": False,
                                      "context": 99}]


def test_records_across_a_chunk_boundary_and_untouched_groups():
    """G = 257 with records only in groups 255, 256 and 0: every other group's
    state is untouched, gflags 0 and stop_at UINT32_MAX."""
    rng = np.random.default_rng(3)
    nodes = [F.Node(term=int(rng.integers(1, 9)), vote=int(rng.integers(0, 4)),
                    lead=int(rng.integers(0, 4)), committed=int(rng.integers(0, 9)),
                    last_index=20, last_term=1, role=int(rng.integers(0, 4)) | 0x80,
                    election_elapsed=int(rng.integers(0, 20)),
                    heartbeat_elapsed=int(rng.integers(0, 20))) for _ in range(257)]
    recs = []
    for k in range(12):
        for g in (255, 256, 0):
            recs.append((g, F.Rec(int(rng.integers(0, 4)), int(rng.integers(1, 4)),
                                  int(rng.integers(1, 10)), int(rng.integers(0, 20)),
                                  int(rng.integers(0, 3)), bool(k & 1))))
    res, want = run("G257", nodes, recs, F.Config(10, True, False))
    quiet = np.ones(257, bool)
    quiet[[0, 255, 256]] = False
    assert not want["gflags"][quiet].any() and (want["stop_at"][quiet] == F.NO_STOP).all()


def test_one_hot_group_with_rising_terms():
    """All M = 700 records in one group of 300, terms rising through the
    batch: the long run and its sort by batch index.  The records' other
    columns follow no order."""
    rng = np.random.default_rng(11)
    G, M, hot = 300, 700, 137
    nodes = [_hb_node(term=1) for _ in range(G)]
    recs = []
    for i in range(M):
        kind = int(rng.choice([F.HEARTBEAT, F.HEARTBEAT, F.VOTE, F.PREVOTE, F.TIMEOUT_NOW]))
        if kind == F.TIMEOUT_NOW and i < 650:
            kind = F.HEARTBEAT          # (the campaign stop only near the end)
        recs.append((hot, F.Rec(kind, int(rng.integers(1, 4)), 1 + i // 3,
                                int(rng.integers(0, 41)), int(rng.integers(0, 300)),
                                bool(rng.random() < 0.3))))
    res, want = run("hot", nodes, recs, F.Config(10, False, True))
    assert want["stats"]["became_follower"] > 100 and want["stats"]["heartbeats"] > 100


def test_many_records_inside_one_chunk():
    """M = 5000 for 200 groups of one 256-group chunk (25 per group: runs
    past the step kernel's own sort) beside 600 groups without records."""
    nodes, recs = P.fuzz(21, G=800, M=5000)
    recs = [(g % 200 + 256 if g < 800 else g, r) for g, r in recs]
    res, want = run("one chunk", nodes, recs, F.Config(10, True, True))
    assert want["stats"]["after_stop"] > 0 and (want["stop_at"][:256] == F.NO_STOP).all()


def test_stats_accumulate_and_buffers_are_reused():
    nodes, recs = P.fuzz(5, G=64, M=300)
    cfg = F.Config(10, True, False)
    fg, ib = upload(nodes, recs, cfg)
    res = qf.follower_step(fg, ib)
    first = res.stats_dict()
    fg2, _ = upload(nodes, recs, cfg)
    res2 = qf.follower_step(fg2, ib, out=res)
    assert res2 is res and res.stats_dict() == {k: 2 * v for k, v in first.items()}
    _, want = P.expected(nodes, recs, cfg)
    assert first == want["stats"]


# --------------------------------------------------------------- plain ctypes ---

def test_plain_ctypes_call():
    """The C ABI on raw device pointers, without the mirror."""
    lib = _lib.load()
    nodes, recs = P.fuzz(9, G=130, M=600)
    cfg = F.Config(10, True, True)
    G, M = len(nodes), len(recs)
    a, r = P.pack_nodes(nodes), P.pack_recs(recs)
    ptr = C.c_void_p()
    held = []

    def dev(arr):
        arr = np.ascontiguousarray(arr)
        assert lib.qb_malloc(max(arr.nbytes, 8), C.byref(ptr)) == 0
        p = ptr.value
        held.append(p)
        assert lib.qb_copy_h2d_async(p, arr.ctypes.data, arr.nbytes, None) == 0
        assert lib.qb_stream_sync(None) == 0   # (arr may die with this frame)
        return p

    def back(p, dt, n):
        out = np.empty(n, dt)
        assert lib.qb_copy_d2h_async(out.ctypes.data, p, out.nbytes, None) == 0
        assert lib.qb_stream_sync(None) == 0
        return out
    try:
        gp = {k: dev(v) for k, v in a.items()}
        rp = {k: dev(v) for k, v in r.items()}
        outs = {"resp_type": dev(np.full(M, 0xA5, np.uint8)), "resp_term": dev(np.zeros(M, np.uint64)),
                "stop_at": dev(np.zeros(G, np.uint32)), "gflags": dev(np.full(G, 0xA5, np.uint8)),
                "stats": dev(np.zeros(len(qf.FSTAT_NAMES), np.uint64))}
        nws = lib.qb_follower_workspace_bytes(G, M)
        ws = dev(np.zeros(nws, np.uint8))
        fg = qf.FollowerGroupsC(G=G, election_timeout=10, check_quorum=1, pre_vote=1, **gp)
        ib = qf.FollowerInboxC(M=M)
        for k, v in rp.items():
            setattr(ib, k, v)
        assert lib.qb_stream_sync(None) == 0
        rc = lib.qb_dev_follower_step(C.byref(fg), C.byref(ib), outs["resp_type"],
                                      outs["resp_term"], outs["stop_at"], outs["gflags"],
                                      outs["stats"], ws, nws, None)
        assert rc == 0, lib.qb_last_error()
        want_groups, want = P.expected(nodes, recs, cfg)
        for k, w in want_groups.items():
            assert np.array_equal(back(gp[k], w.dtype, G), w), k
        for k, n in (("resp_type", M), ("resp_term", M), ("stop_at", G), ("gflags", G)):
            assert np.array_equal(back(outs[k], want[k].dtype, n), want[k]), k
        st = back(outs["stats"], np.uint64, len(qf.FSTAT_NAMES)).tolist()
        assert dict(zip(qf.FSTAT_NAMES, st)) == want["stats"]
    finally:
        for p in held:
            lib.qb_free(p)


# ----------------------------------------------------------------- round trip ---

def test_heartbeat_round_trip_over_tick_follower_step_and_leader_step():
    """64 groups x 3 voters.  qb_dev_leader_tick's heartbeats become
    follower-step records on two follower tables; their MsgHeartbeatResp
    become QB_IN_HEARTBEAT_RESP records of qb_dev_leader_step.  After it every
    peer slot is RecentActive, and each follower's committed is min(match,
    committed) of its leader."""
    G, n = 64, 3
    lg, base = ql.synth_streaming(G, W=4, D=1, n=n, device=DEV)
    peer = (torch.arange(lg.S, device=DEV) % n) != 0
    lg.t["pstate"][peer] &= 0xF7                      # no peer RecentActive yet
    lg.t["match"][2::n] -= 5                          # slot 2 lags: min() picks match there
    state = qt.TickState.from_numpy(np.full(G, qt.ROLE_LEADER | qt.ROLE_PROMOTABLE, np.uint8),
                                    np.zeros(G, np.uint32), np.zeros(G, np.uint32),
                                    np.full(G, 15, np.uint32), device=DEV)
    tr = lg.tick(state, 10, 1, True)
    assert (ql._to_np(tr.tflags, np.uint8, G) & qt.TFLAG_BEAT).all()
    before = lg.numpy()
    term, committed = before["term"], before["committed"]
    match = before["match"].reshape(G, n)
    hb_commit = ql._to_np(tr.hb_commit, np.uint64, lg.S).reshape(G, n)
    hb_ctx = ql._to_np(tr.hb_ctx, np.uint64, G)
    order = np.random.default_rng(2).permutation(G)
    resp = []
    for k in (1, 2):
        fa = {"term": term.copy(), "vote": np.ones(G, np.uint64), "lead": np.ones(G, np.uint64),
              "committed": np.zeros(G, np.uint64), "last_index": before["last_index"].copy(),
              "last_term": term.copy()}
        st = qt.TickState.from_numpy(np.full(G, qt.ROLE_PROMOTABLE, np.uint8),
                                     np.full(G, 4, np.uint32), np.zeros(G, np.uint32),
                                     np.full(G, 15, np.uint32), device=DEV)
        fg = qf.FollowerGroups.from_numpy(fa, st, 10, True, False, device=DEV)
        ib = qf.FollowerInbox.from_numpy(order, np.zeros(G, np.uint8), np.ones(G, np.uint64),
                                         term[order], hb_commit[order, k], hb_ctx[order], device=DEV)
        res = qf.follower_step(fg, ib)
        msgs = list(res.responses())
        assert len(msgs) == G and all(m["type"] == qf.MSG_HEARTBEAT_RESP for m in msgs)
        got = fg.numpy()
        assert np.array_equal(got["committed"], np.minimum(match[:, k], committed))
        assert not got["election_elapsed"].any()
        resp += [(int(order[m["i"]]), k, m["context"], m["term"]) for m in msgs]
    grp, slot, ctx, rterm = (np.array(c, np.uint64) for c in zip(*resp))
    ib = ql.LeaderInbox.from_numpy(grp.astype(np.uint32), slot.astype(np.uint8),
                                   np.full(len(grp), ql.IN_HEARTBEAT_RESP, np.uint8), ctx, rterm,
                                   device=DEV)
    out = lg.step(ib)
    assert out.stats["applied"] == 2 * G
    pstate = lg.numpy()["pstate"].reshape(G, n)
    assert (pstate[:, 1:] & ql.PR_RECENT_ACTIVE).all()
