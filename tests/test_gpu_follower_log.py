"""qb_dev_follower_log_step on the device against tests/append_ref.py,
bit-exact: every in/out array of the groups, the run table, meta, all six
response / output columns, stop_at, gflags and all 16 counters.  The outputs
are pre-filled with 0xA5 bytes, so an element the call must write and did not
— or must not write and did — shows; the run table's rows past a group's count
hold a marker the same way.  All comparisons are integer equality."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from etcd_amd import _lib
from etcd_amd.quorum import follower as qf, leader as ql, tick as qt
from oracle import leader_ref as L
from tests import append_pack as AP, append_ref as A, follower_pack as P, follower_ref as F
from tests import leader_pack as LP
from tests.test_append_ref import check_fuzz_coverage

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL64 = np.uint64(AP.FILL)
M_COLS = (("resp_type", np.uint8), ("resp_term", np.uint64), ("resp_index", np.uint64),
          ("resp_hint", np.uint64), ("resp_log_term", np.uint64), ("app_from", np.uint64))


def upload(nodes, recs, cfg, log0=None, app_arrays=None):
    a = P.pack_nodes(nodes)
    state = qt.TickState.from_numpy(a["role"], a["election_elapsed"], a["heartbeat_elapsed"],
                                    np.zeros(len(nodes), np.uint32), device=DEV)
    fg = qf.FollowerGroups.from_numpy(a, state, cfg.election_timeout, cfg.check_quorum,
                                      cfg.pre_vote, device=DEV)
    lg0 = log0 if log0 is not None else AP.pack_log(nodes)
    lg = qf.FollowerLog.from_numpy(lg0["meta"], lg0["first_index"], lg0["run_start"],
                                   lg0["run_term"], a, device=DEV)
    r, ap = AP.pack_recs(recs)
    if app_arrays is not None:
        ap = app_arrays
    ib = qf.FollowerInbox.from_numpy(r["group"], r["flags"], r["from"], r["term"], r["index"],
                                     r["aux"], device=DEV)
    app = qf.FollowerAppInbox.from_numpy(ap["commit"], ap["ent_off"], ap["ent_term"],
                                         ap["ent_len"], device=DEV)
    return fg, lg, ib, app


def filled_result(G, M):
    need = qf.follower_log_workspace_bytes(G, M)

    def col():
        return torch.from_numpy(np.full(max(M, 1), FILL64).view(np.int64)).to(DEV)
    return qf.FollowerLogResult(torch.full((max(M, 1),), 0xA5, dtype=torch.uint8, device=DEV), col(),
                                torch.full((max(G, 1),), 0x5A5A5A5A, dtype=torch.int32, device=DEV),
                                torch.full((max(G, 1),), 0xA5, dtype=torch.uint8, device=DEV),
                                torch.zeros(len(qf.FLSTAT_NAMES), dtype=torch.int64, device=DEV),
                                torch.full(((need + 7) // 8,), -1, dtype=torch.int64, device=DEV),
                                None, col(), col(), col(), col())


def compare(where, fg, lg, res, G, M, want_groups, want_log, want):
    got = fg.numpy()
    for k, w in want_groups.items():
        assert np.array_equal(got[k], w), (where, k, np.nonzero(got[k] != w)[0][:8])
    gl = lg.numpy()
    for k, w in want_log.items():
        assert np.array_equal(gl[k], w), (where, k, np.argwhere(gl[k] != w)[:8])
    for k, dt in M_COLS:
        g = ql._to_np(getattr(res, k), dt, M)
        assert np.array_equal(g, want[k]), (where, k, np.nonzero(g != want[k])[0][:8])
    for k, dt in (("stop_at", np.uint32), ("gflags", np.uint8)):
        g = ql._to_np(getattr(res, k), dt, G)
        assert np.array_equal(g, want[k]), (where, k, np.nonzero(g != want[k])[0][:8])
    assert res.stats_dict() == want["stats"], (where, res.stats_dict(), want["stats"])


def run(where, nodes, recs, cfg, log0=None, app_arrays=None, want_from=None):
    """One call on the device beside append_ref; returns (result, expected
    outputs).  want_from: the records the restatement steps when the device
    is handed doctored arrays that mean the same."""
    G, M = len(nodes), len(recs)
    fg, lg, ib, app = upload(nodes, recs, cfg, log0, app_arrays)
    res = qf.follower_log_step(fg, lg, ib, app, out=filled_result(G, M))
    want_groups, want_log, want = AP.expected(nodes, want_from or recs, cfg, log0)
    compare(where, fg, lg, res, G, M, want_groups, want_log, want)
    res.groups_after, res.log_after = fg.numpy(), lg.numpy()
    lg.validate(fg)   # the table the step leaves holds the invariant it needs
    return res, want


# --------------------------------------------------------- golden scenarios ---

SCENARIOS = AP.scenarios()


@pytest.mark.parametrize("sc", SCENARIOS, ids=[s[0] for s in SCENARIOS])
def test_golden_scenario_on_device(sc):
    """The reference's tables, G = 1 each (tests/test_append_ref.py holds the
    restatement to their expectations)."""
    name, cfg, node, recs = sc
    run(name, [node], [(0, r) for r in recs], cfg)


def test_golden_scenarios_in_one_batch():
    """All of them as the groups of one batch, their records interleaved."""
    rng = np.random.default_rng(7)
    nodes = [sc[2] for sc in SCENARIOS]
    recs = P.interleave([sc[3] for sc in SCENARIOS], rng)
    _, want = run("packed", nodes, recs, SCENARIOS[0][1])
    assert want["stats"]["app_rejected"] >= 12 and want["stats"]["app_truncated"] >= 4


# ------------------------------------------------------------- kinds 0 to 4 ---

@pytest.mark.parametrize("cq,pv", ((True, False), (False, True)))
def test_other_kinds_equal_follower_step(cq, pv):
    """Without FIN_APP records the outputs and the state are those of
    qb_dev_follower_step on the same input (the old call is the oracle; its
    kind 5 is a bad kind there, so the fuzz's kinds above 4 are cut to 6 / 7),
    and meta and the run table are untouched."""
    base, recs = P.fuzz(4, G=300, M=1500)
    recs = [(g, r if r.kind != 5 else F.Rec(6, r.frm, r.term, r.index, r.aux, r.force))
            for g, r in recs]
    cfg = P.fuzz_config(cq, pv)
    nodes = []
    for n in base:   # a log of the node's (last_index, last_term): one run behind the dummy
        terms = [0] + [n.last_term] * n.last_index if n.last_index else [n.last_term]
        ln = A.new_node(terms, **{k: getattr(n, k) for k in (
            "term", "vote", "lead", "committed", "role", "election_elapsed", "heartbeat_elapsed")})
        assert (ln.last_index, ln.last_term) == (n.last_index, n.last_term)
        nodes.append(ln)
    G, M = len(nodes), len(recs)
    res, _ = run("kinds 0-4", nodes, recs, cfg)
    a = P.pack_nodes(nodes)
    state = qt.TickState.from_numpy(a["role"], a["election_elapsed"], a["heartbeat_elapsed"],
                                    np.zeros(G, np.uint32), device=DEV)
    fg = qf.FollowerGroups.from_numpy(a, state, cfg.election_timeout, cfg.check_quorum,
                                      cfg.pre_vote, device=DEV)
    r = P.pack_recs(recs)
    ib = qf.FollowerInbox.from_numpy(r["group"], r["flags"], r["from"], r["term"], r["index"],
                                     r["aux"], device=DEV)
    old = qf.follower_step(fg, ib)
    for k, v in fg.numpy().items():
        assert np.array_equal(res.groups_after[k], v), k
    for k, dt, n in (("resp_type", np.uint8, M), ("resp_term", np.uint64, M),
                     ("stop_at", np.uint32, G), ("gflags", np.uint8, G)):
        assert np.array_equal(ql._to_np(getattr(res, k), dt, n), ql._to_np(getattr(old, k), dt, n)), k
    so, sn = old.stats_dict(), res.stats_dict()
    assert {k: sn[k] for k in so} == so and not any(sn[k] for k in sn if k not in so)
    lg0 = AP.pack_log(nodes)
    for k in ("meta", "run_start", "run_term"):
        assert np.array_equal(res.log_after[k], lg0[k]), k
    assert not ql._to_np(res.resp_index, np.uint64, M).any()
    assert not ql._to_np(res.app_from, np.uint64, M).any()
    assert (ql._to_np(res.resp_hint, np.uint64, M) == FILL64).all()


def test_follower_step_still_drops_kind_5():
    n = F.Node(term=3, last_index=4, last_term=3)
    a = P.pack_nodes([n])
    state = qt.TickState.from_numpy(a["role"], a["election_elapsed"], a["heartbeat_elapsed"],
                                    np.zeros(1, np.uint32), device=DEV)
    fg = qf.FollowerGroups.from_numpy(a, state, 10, False, False, device=DEV)
    one = np.ones(1, np.uint64)
    ib = qf.FollowerInbox.from_numpy(np.zeros(1, np.uint32), np.full(1, 5, np.uint8), one, 3 * one,
                                     4 * one, 3 * one, device=DEV)
    res = qf.follower_step(fg, ib)
    assert res.stats_dict()["bad_kind"] == 1 and not list(res.responses())


# ------------------------------------------------------------------- shapes ---

CFG = F.Config(10, True, True)


def follower(terms, first=1, term=None, committed=None, **kw):
    n = A.new_node(terms, first, term=terms[-1] if term is None else term, lead=2,
                   role=F.FOLLOWER | F.ROLE_PROMOTABLE, election_elapsed=3, heartbeat_elapsed=2,
                   **kw)
    n.committed = first - 1 if committed is None else committed
    return n


def steady(n, k=3, commit=None):
    """The next k entries of the node's term behind its end."""
    return AP.app(2, n.term, n.last_index, n.last_term, [n.last_term] * k,
                  n.last_index + 1 if commit is None else commit)


def test_one_group_and_the_mirror_views():
    n = follower([0, 1, 1, 2], term=2)
    res, want = run("G1 M0", [n], [], CFG)
    assert want["gflags"].tolist() == [0] and want["stop_at"].tolist() == [F.NO_STOP]
    recs = [(0, steady(n, 2, commit=4)), (0, AP.app(2, 2, 7, 2, [2])), (0, AP.app(2, 1, 0, 0, []))]
    res, want = run("G1 M3", [n], recs, CFG)
    assert list(res.responses()) == [
        {"i": 0, "type": 4, "to": 2, "term": 2, "reject": False, "context": 0, "index": 5,
         "hint": 0, "log_term": 0},
        {"i": 1, "type": 4, "to": 2, "term": 2, "reject": True, "context": 0, "index": 7,
         "hint": 5, "log_term": 2},
        {"i": 2, "type": 4, "to": 2, "term": 2, "reject": False, "context": 0, "index": 0,
         "hint": 0, "log_term": 0}]       # the lower term, answered (raft.go:906)
    assert list(res.appends()) == [{"i": 0, "from": 4}]
    assert res.groups_after["committed"].tolist() == [4]
    assert want["gflags"].tolist() == [A.FFLAG_APPENDED | F.FFLAG_HARDSTATE]
    # the steady record touched neither the table nor meta
    assert np.array_equal(res.log_after["run_start"], AP.pack_log([n])["run_start"])


def test_tile_boundary_and_the_run_major_stride():
    """G = 257, records in groups 255, 256 and 0 only; each of the three logs
    has its own run count, so a wrong stride reads another group's run."""
    rng = np.random.default_rng(3)
    nodes = [follower(AP.cap_runs([0] + AP._rand_log(rng, int(rng.integers(3, 20)), 1, 0.3)),
                      first=int(f)) for f in rng.choice([1, 9], 257)]
    nodes[255] = follower([0, 1, 2, 3, 4, 5, 6])
    nodes[256] = follower([0, 1, 1, 1, 4, 4])
    nodes[0] = follower([2, 2, 2, 3], first=1 << 33)
    recs = []
    for g in (255, 256, 0):
        n = nodes[g]
        d = n.first_index - 1
        recs += [(g, AP.app(2, n.term, d + 2, n.terms[2], [n.terms[3], 9, 9], d + 3)),  # two truncate
                 (g, AP.app(2, n.term, d + 4, 77, [5])),                               # rejected
                 (g, AP.app(2, n.term, d + 5, 9, [9, 10]))]                            # behind it
    res, want = run("G257", nodes, recs, CFG)
    quiet = np.ones(257, bool)
    quiet[[0, 255, 256]] = False
    assert not want["gflags"][quiet].any() and (want["stop_at"][quiet] == F.NO_STOP).all()
    assert want["stats"]["app_truncated"] == 2 and want["stats"]["app_rejected"] == 3
    assert want["stats"]["app_accepted"] == 6


@pytest.mark.parametrize("n_recs", (16, 17))
def test_inline_and_long_run_boundary(n_recs):
    """A group with 16 and with 17 records of mixed kinds, beside 40 groups
    with one record each."""
    rng = np.random.default_rng(n_recs)
    nodes = [follower([0, 1, 1, 2, 2, 3], term=3) for _ in range(41)]
    hot = []
    n = nodes[7]
    end = n.last_index
    for j in range(n_recs):
        k = j % 4
        if k == 0:
            hot.append(AP.app(2, 3, end, 3, [3, 3], end + 1))
            end += 2
        elif k == 1:
            hot.append(F.Rec(F.HEARTBEAT, 2, 3, end, 5))           # Commit = the new end
        elif k == 2:
            hot.append(F.Rec(F.PREVOTE, 3, 4, end, 3, True))       # up to date only with the new end
        else:
            hot.append(AP.app(2, 3, end, 3, [3], 0))               # at the committed end
            end += 1
    per_group = [[steady(x, 1)] for x in nodes]
    per_group[7] = hot
    recs = P.interleave(per_group, rng)
    res, want = run(f"run of {n_recs}", nodes, recs, CFG)
    assert res.groups_after["last_index"][7] == end
    assert res.groups_after["committed"][7] == end - 1
    assert want["stats"]["granted"] == n_recs // 4


def test_one_group_with_300_records():
    """One group holds the whole batch: appends whose terms rise every 43
    records (runs appended, the 8th reached), truncating retries, rejects,
    heartbeats and votes between them.  (A shadow node stepped by the
    restatement tells the generator where the log stands.)"""
    rng = np.random.default_rng(11)
    nodes = [follower([0, 1, 1], term=1) for _ in range(20)]
    recs, shadow = [], copy.deepcopy(nodes[13])
    for i in range(300):
        t = 1 + i // 43
        r = rng.random()
        li = shadow.last_index
        if r < 0.5:
            at = max(shadow.committed, li - int(rng.integers(0, 4)))
            et = t + int(rng.random() < 0.2)                          # (now and then a term ahead)
            rec = AP.app(2, t, at, shadow.log_term(at), [et] * int(rng.integers(0, 4)),
                         max(at, 2) - 2)
        elif r < 0.6:
            rec = AP.app(2, t, li + 2, t, [t])                        # past the end: rejected
        elif r < 0.8:
            rec = F.Rec(F.HEARTBEAT, 2, t, int(rng.integers(0, 3)), 1)
        else:
            rec = F.Rec(F.PREVOTE, 3, t + 1, li, shadow.last_term, True)
        trial = copy.deepcopy(shadow)
        if A.step_batch([trial], [(0, rec)], CFG)["stop_at"][0] != F.NO_STOP:   # (a 9th run)
            rec = F.Rec(F.HEARTBEAT, 2, t, 0, 1)
            trial = copy.deepcopy(shadow)
            A.step_batch([trial], [(0, rec)], CFG)
        recs.append((13, rec))
        shadow = trial
    res, want = run("hot 300", nodes, recs, CFG)
    st = want["stats"]
    assert st["after_stop"] == 0 and st["app_accepted"] > 50 and st["app_rejected"] > 10
    assert st["app_truncated"] > 5 and st["granted"] > 20
    assert (res.log_after["meta"][13] >> 16) & 0xF >= 6


def test_eight_runs_then_a_ninth():
    """An append that reaches exactly 8 runs; the same one with one more term
    needs a 9th: stop, nothing changed, the record behind it not stepped."""
    base = [0, 1, 2, 3, 4, 5, 6]                       # 7 runs, the dummy's included
    fits, not_ = follower(base, term=9), follower(base, term=9)
    recs = [(0, AP.app(2, 9, 6, 6, [6, 7, 7], 8)), (0, steady(fits, 1)),
            (1, AP.app(2, 9, 6, 6, [6, 7, 8], 8)), (1, F.Rec(F.HEARTBEAT, 2, 9, 2, 0))]
    res, want = run("8 / 9 runs", [fits, not_], recs, CFG)
    assert (res.log_after["meta"] >> 16 & 0xF).tolist() == [8, 7]
    assert want["gflags"].tolist() == [A.FFLAG_APPENDED | F.FFLAG_HARDSTATE, A.FFLAG_LOG_RUNS]
    assert want["stop_at"].tolist() == [F.NO_STOP, 2] and want["stats"]["after_stop"] == 1
    assert res.groups_after["last_index"].tolist() == [9, 6]
    # a 9-run group that first truncates fits again
    n = follower(base + [7], term=9)
    res, want = run("truncate to fit", [n], [(0, AP.app(2, 9, 4, 4, [8, 9, 9]))], CFG)
    assert (res.log_after["meta"] >> 16 & 0xF).tolist() == [7] and want["stats"]["app_truncated"] == 1


def test_truncation_drops_runs_and_merges_into_the_kept_one():
    n = follower([0, 1, 1, 1, 2, 3, 3, 4, 5], first=5, term=6)
    # entries 7, 8 match; 9.. conflict: runs t2 t3 t4 t5 go, the message's t1s merge into run t1
    recs = [(0, AP.app(2, 6, 5, 1, [1, 1, 1, 1, 6], 9))]
    res, want = run("drop and merge", [n], recs, CFG)
    assert (res.log_after["meta"][0] >> 16) & 0xF == 3          # dummy t0 | t1 | t6
    assert res.log_after["run_start"][:3, 0].tolist() == [4, 5, 10]
    assert res.log_after["run_term"][:3, 0].tolist() == [0, 1, 6]
    assert list(res.appends()) == [{"i": 0, "from": 8}]
    assert want["stats"]["entries_appended"] == 3 and want["stats"]["app_truncated"] == 1


def test_entry_run_shapes():
    """A record with no entries, one with 12 entry runs, zero-length runs
    (first, middle and last), and ent_off above E."""
    nodes = [follower([0, 1, 1]) for _ in range(5)]
    twelve = [1, 1, 2, 2, 2, 3, 4, 4, 5, 6, 6, 7, 8, 9, 9, 10, 11, 12]   # 12 runs: a ninth table run
    recs = [(0, AP.app(2, 1, 2, 1, [], 2)),
            (1, AP.app(2, 1, 2, 1, twelve)),
            (2, AP.app(2, 1, 1, 1, [1, 2, 2, 3])),
            (3, AP.app(2, 1, 2, 1, [4, 4])),
            (4, AP.app(2, 1, 2, 1, [1, 5]))]
    inbox, ap = AP.pack_recs(recs)
    # doctor the runs: record 2 gets zero-length runs around its own; record
    # 4's runs leave the arrays and its offsets lie above E (read as E: no
    # entries), so record 3's end does too (read as E: its own runs, the last)
    et, el, off = ap["ent_term"].tolist(), ap["ent_len"].tolist(), ap["ent_off"].tolist()
    lo, hi = off[2], off[3]
    et[lo:hi] = [9, 1, 9, 2, 3, 9]
    el[lo:hi] = [0, 1, 0, 2, 1, 0]
    grow = 6 - (hi - lo)
    off = off[:3] + [o + grow for o in off[3:]]
    del et[off[4]:off[5]], el[off[4]:off[5]]
    assert off[4] == len(et)
    off[4], off[5] = len(et) + 7, len(et) + 40
    ap = {"commit": ap["commit"], "ent_off": np.array(off, np.uint32),
          "ent_term": np.array(et, np.uint64), "ent_len": np.array(el, np.uint32)}
    want_from = recs[:4] + [(4, AP.app(2, 1, 2, 1, []))]
    res, want = run("entry runs", nodes, recs, CFG, app_arrays=ap, want_from=want_from)
    assert want["gflags"][1] == A.FFLAG_LOG_RUNS and want["stats"]["app_accepted"] == 4
    assert res.groups_after["last_index"].tolist() == [2, 2, 5, 4, 2]


def test_twelve_entry_runs_mostly_inside_the_log():
    """A record of 12 entry runs (zero-length ones between them, two adjacent
    runs of one term) whose first 11 or 12 entries the log already holds:
    only the tail is appended, once behind the end and once over a conflicting
    last entry (a run dropped, the message's run merged into the kept one),
    both ending at exactly 8 runs."""
    runs = [(1, 2), (9, 0), (2, 2), (9, 0), (3, 2), (9, 0), (4, 2), (9, 0), (5, 2), (6, 1), (6, 1),
            (7, 3)]
    ents = [t for t, n in runs for _ in range(n)]
    assert len(runs) == 12 and ents == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 7]
    nodes = [follower([0] + ents[:12], term=7),            # 7 runs; append at 13
             follower([0] + ents[:11] + [8], term=8)]      # 8 runs; conflict at 12
    recs = [(g, AP.app(2, 8, 0, 0, ents, 14)) for g in (0, 1)]
    _, ap = AP.pack_recs(recs)
    ap = {"commit": ap["commit"], "ent_off": np.array([0, 12, 24], np.uint32),
          "ent_term": np.array([t for t, _ in runs] * 2, np.uint64),
          "ent_len": np.array([n for _, n in runs] * 2, np.uint32)}
    res, want = run("12 runs", nodes, recs, CFG, app_arrays=ap)
    assert list(res.appends()) == [{"i": 0, "from": 13}, {"i": 1, "from": 12}]
    assert (res.log_after["meta"] >> 16 & 0xF).tolist() == [8, 8]
    for g in (0, 1):
        assert res.log_after["run_start"][:8, g].tolist() == [0, 1, 3, 5, 7, 9, 11, 13]
        assert res.log_after["run_term"][:8, g].tolist() == [0, 1, 2, 3, 4, 5, 6, 7]
    assert res.groups_after["last_index"].tolist() == [15, 15]
    assert res.groups_after["committed"].tolist() == [14, 14]
    assert want["stats"]["entries_appended"] == 3 + 4 and want["stats"]["app_truncated"] == 1


def test_vote_and_heartbeat_behind_an_append_see_the_new_log():
    a, b = follower([0, 1, 1], term=2), follower([0, 1, 1], term=2)
    a.lead = b.lead = 0
    recs = [(0, F.Rec(F.VOTE, 3, 2, 3, 1)),                   # (3, t1) is up to date against (2, t1)
            (1, AP.app(2, 2, 2, 1, [2, 2], 0)),               # b's log becomes (4, t2)
            (1, F.Rec(F.PREVOTE, 3, 3, 3, 1)),                # ... so this is rejected
            (1, F.Rec(F.PREVOTE, 3, 3, 4, 2)),                # and this granted
            (1, F.Rec(F.HEARTBEAT, 2, 2, 4, 0)),              # Commit 4 is in range only now
            (0, F.Rec(F.HEARTBEAT, 3, 2, 4, 0))]              # a: commitTo would panic
    res, want = run("sees the new log", [a, b], recs, F.Config(10, False, True))  # (no lease)
    assert want["resp_type"].tolist() == [F.MSG_VOTE_RESP, A.MSG_APP_RESP,
                                          F.MSG_PREVOTE_RESP | F.REJECT, F.MSG_PREVOTE_RESP,
                                          F.MSG_HEARTBEAT_RESP, 0]
    assert res.groups_after["committed"].tolist() == [0, 4]
    assert want["gflags"][0] & F.FFLAG_COMMIT_RANGE


def test_each_stop_with_records_behind_it():
    """LOG_CONFLICT in both forms (the gap, and a conflict at or below
    committed), LOG_RUNS, COMMIT_RANGE from a MsgApp, and a HOST record:
    stop_at is the record, nothing of it is applied — not even its higher term
    — and the records behind it count as AFTER_STOP.

    The conflict at or below committed (log.go:94-95, the panic case of
    TestLogMaybeAppend) is behind handleAppendEntries' Index < committed
    answer unless the entries' indexes wrap: the last group's log ends at
    2^64 - 1 and is committed to its end; the MsgApp at Index = 2^64 - 1 has
    the entries [0, 3]: the first wraps to index 0 and "matches" term 0
    there, the second conflicts at ci = 1 <= committed."""
    top = (1 << 64) - 1
    eight = [0, 1, 2, 3, 4, 5, 6, 7]
    nodes = [follower([0, 1, 1], term=1), follower(eight, term=7), follower([0, 1, 1], term=1),
             follower([0, 1, 1], term=1), follower([1, 1, 1], first=top - 2, term=1)]
    assert nodes[4].last_index == top - 1
    # (behind the steady record each log ends one further: 3, 8, 3, 3, 2^64 - 1)
    stops = [AP.app(2, 5, 4, 0, [3]),              # LogTerm 0 matches past the end; a gap
             AP.app(2, 9, 8, 7, [8]),              # a 9th run
             AP.app(2, 5, 3, 1, [0, 0], 5),        # zero terms match past the end; Commit there
             F.Rec(F.HOST, 2, 5),
             AP.app(2, 5, top, 1, [0, 3], 7)]      # wraps: a conflict at 1, below committed
    recs = []
    for g, s in enumerate(stops):
        recs += [(g, steady(nodes[g], 1)), (g, s)]
    for g in range(5):
        recs += [(g, F.Rec(F.HEARTBEAT, 2, 9, 0, 0)), (g, AP.app(2, 9, 0, 0, []))]
    res, want = run("stops", nodes, recs, CFG)
    hs = A.FFLAG_APPENDED | F.FFLAG_HARDSTATE
    assert want["gflags"].tolist() == [hs | A.FFLAG_LOG_CONFLICT, hs | A.FFLAG_LOG_RUNS,
                                       hs | F.FFLAG_COMMIT_RANGE, hs | F.FFLAG_HOST_MSG,
                                       hs | A.FFLAG_LOG_CONFLICT]
    assert want["stop_at"].tolist() == [1, 3, 5, 7, 9] and want["stats"]["after_stop"] == 10
    assert res.groups_after["term"].tolist() == [1, 7, 1, 1, 1]
    assert res.groups_after["last_index"].tolist() == [3, 8, 3, 3, top]
    assert res.groups_after["committed"].tolist() == [3, 8, 3, 3, top]
    assert not want["resp_type"][10:].any() and not want["app_from"][1:10:2].any()
    assert not want["app_from"][10:].any()


def test_indexes_and_terms_near_2_to_64():
    top = (1 << 64) - 1
    first = top - 40
    t = top - 9
    n = follower([t, t, t + 1, t + 1, t + 3], first=first, term=t + 5)
    d = first - 1
    recs = [(0, AP.app(2, t + 5, d + 4, t + 3, [t + 3, t + 5, t + 5], d + 1)),     # appends
            (0, AP.app(2, t + 5, d + 2, t + 1, [t + 1, t + 4, t + 6, t + 6], d + 3)),  # truncates
            (0, AP.app(2, t + 5, d + 30, t + 7, [t + 7])),                          # rejected: hint
            (0, AP.app(2, t + 5, d + 5, t + 9, [])),                                # rejected inside
            (0, F.Rec(F.VOTE, 3, t + 6, d + 7, t + 6, True)),
            (0, AP.app(3, t + 9, d + 6, t + 6, [t + 9] * 31, top))]                 # to 2^64 - 4
    res, want = run("near 2^64", [n], recs, CFG)
    assert res.groups_after["last_index"].tolist() == [d + 37] and d + 37 == top - 4
    assert res.groups_after["committed"].tolist() == [top - 4]
    assert want["stats"]["app_rejected"] == 2 and want["stats"]["granted"] == 1
    assert want["resp_hint"][2] == d + 6 and want["resp_log_term"][3] == t + 6


# --------------------------------------------------------------------- fuzz ---

@pytest.mark.parametrize("cq,pv", P.FUZZ_CONFIGS)
@pytest.mark.parametrize("seed", AP.FUZZ_SEEDS)
def test_fuzz(seed, cq, pv):
    """G = 600, M = 2400 (tests/append_pack.py fuzz), under both settings of
    check_quorum and pre_vote.  What the batch reaches is asserted on the
    restatement's own counters before the device is compared."""
    nodes, recs = AP.fuzz(seed)
    cfg = P.fuzz_config(cq, pv)
    _, _, want0 = AP.expected(nodes, recs, cfg)
    check_fuzz_coverage(want0, len(recs))
    res, want = run(f"fuzz seed {seed} cq {cq} pv {pv}", nodes, recs, cfg)
    msgs = list(res.responses())
    assert [m["i"] for m in msgs] == np.flatnonzero(want["resp_type"]).tolist()
    for m in msgs[:300]:
        i = m["i"]
        assert m["term"] == int(want["resp_term"][i])
        if m["type"] == qf.MSG_APP_RESP:
            assert m["index"] == int(want["resp_index"][i])
            if m["reject"]:
                assert (m["hint"], m["log_term"]) == (int(want["resp_hint"][i]),
                                                      int(want["resp_log_term"][i]))
    assert [a["i"] for a in res.appends()] == np.flatnonzero(want["app_from"]).tolist()


def test_stats_accumulate_and_buffers_are_reused():
    nodes, recs = AP.fuzz(5, G=64, M=300)
    fg, lg, ib, app = upload(nodes, recs, CFG)
    res = qf.follower_log_step(fg, lg, ib, app)
    first = res.stats_dict()
    fg2, lg2, _, _ = upload(nodes, recs, CFG)
    res2 = qf.follower_log_step(fg2, lg2, ib, app, out=res)
    assert res2 is res and res.stats_dict() == {k: 2 * v for k, v in first.items()}
    assert first == AP.expected(nodes, recs, CFG)[2]["stats"]
    # a follower_step result lacks the MsgApp columns: refused by name
    plain = qf.FollowerResult(res.resp_type, res.resp_term, res.stop_at, res.gflags, res.stats,
                              res.workspace)
    with pytest.raises(_lib.QuorumBatchError, match="resp_index is missing from the result"):
        qf.follower_log_step(fg2, lg2, ib, app, out=plain)


# --------------------------------------------------------------- plain ctypes ---

def test_plain_ctypes_call():
    """The C ABI on raw device pointers, without the mirror."""
    lib = _lib.load()
    nodes, recs = AP.fuzz(9, G=130, M=600)
    G, M = len(nodes), len(recs)
    a, lg0 = P.pack_nodes(nodes), AP.pack_log(nodes)
    r, ap = AP.pack_recs(recs)
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
        lp = {k: dev(v) for k, v in lg0.items()}
        rp = {k: dev(v) for k, v in r.items()}
        app = {k: dev(v) for k, v in ap.items()}
        outs = {k: dev(np.full(M, 0xA5, np.uint8) if dt == np.uint8 else np.full(M, FILL64))
                for k, dt in M_COLS}
        outs.update(stop_at=dev(np.zeros(G, np.uint32)), gflags=dev(np.full(G, 0xA5, np.uint8)),
                    stats=dev(np.zeros(len(qf.FLSTAT_NAMES), np.uint64)))
        nws = lib.qb_follower_workspace_bytes(G, M)   # (the log step's workspace is that call's)
        ws = dev(np.zeros(nws, np.uint8))
        fg = qf.FollowerGroupsC(G=G, election_timeout=10, check_quorum=1, pre_vote=1, **gp)
        lg = qf.FollowerLogC(last_index=gp["last_index"], last_term=gp["last_term"], **lp)
        ib = qf.FollowerInboxC(M=M)
        for k, v in rp.items():
            setattr(ib, k, v)
        ai = qf.FollowerAppInboxC(E=len(ap["ent_term"]), **app)
        ao = qf.FollowerAppOutC(**{k: outs[k] for k in ("resp_index", "resp_hint", "resp_log_term",
                                                        "app_from")})
        rc = lib.qb_dev_follower_log_step(C.byref(fg), C.byref(lg), C.byref(ib), C.byref(ai),
                                          outs["resp_type"], outs["resp_term"], C.byref(ao),
                                          outs["stop_at"], outs["gflags"], outs["stats"], ws, nws,
                                          None)
        assert rc == 0, lib.qb_last_error()
        want_groups, want_log, want = AP.expected(nodes, recs, CFG)
        for k, w in want_groups.items():
            assert np.array_equal(back(gp[k], w.dtype, G), w), k
        for k, w in want_log.items():
            assert np.array_equal(back(lp[k], w.dtype, w.size).reshape(w.shape), w), k
        for k, dt in M_COLS:
            assert np.array_equal(back(outs[k], dt, M), want[k]), k
        for k in ("stop_at", "gflags"):
            assert np.array_equal(back(outs[k], want[k].dtype, G), want[k]), k
        st = back(outs["stats"], np.uint64, len(qf.FLSTAT_NAMES)).tolist()
        assert dict(zip(qf.FLSTAT_NAMES, st)) == want["stats"]
    finally:
        for p in held:
            lib.qb_free(p)


# ----------------------------------------------------------------- round trip ---

def cut_runs(starts, terms, last, lo, n):
    """The terms of the n entries from index lo on, read off a run table."""
    out = []
    for i in range(lo, lo + n):
        assert i <= last
        out.append([t for s, t in zip(starts, terms) if s <= i][-1])
    return out


def test_append_round_trip_over_leader_step_and_follower_log_step():
    """48 groups x 3 voters.  qb_dev_leader_step's QB_MSG_APP become FIN_APP
    records of two follower tables (the entries cut from the leader's run
    table by aux), their MsgAppResp go back as QB_IN_APP_RESP, round by round
    until the leader has nothing to send.  Follower 1 is behind the leader,
    follower 2 has a divergent tail: it rejects, is probed at its hint and
    converges.  Every round both calls equal their restatements."""
    rng = np.random.default_rng(5)
    G, n, cap = 48, 3, 4
    leaders, fnodes = [], {1: [], 2: []}
    for _ in range(G):
        # the leader's terms are even, the other tail's odd: two logs never hold
        # the same (index, term) behind different entries (Log Matching)
        half = AP._rand_log(rng, int(rng.integers(1, 6)), 1, 0.3)
        shared = [2 * t for t in half]
        ltail = [2 * t for t in AP._rand_log(rng, int(rng.integers(2, 9)), half[-1] + 1, 0.25)]
        llog = AP.cap_runs([0] + shared + ltail)
        ltail = llog[1 + len(shared):]
        term = llog[-1]
        starts, rterms = A.runs_of(llog, 1)
        log = L.LogView(1, len(llog) - 1, 0, list(zip(starts, rterms)), 0, 0, 3)
        prs = [L.Progress(match=log.last if s == 0 else 0, next=log.last + 1,
                          state=L.STATE_REPLICATE if s == 0 else L.STATE_PROBE,
                          pending_snapshot=0, recent_active=True, probe_sent=False,
                          inflights=L.Inflights(cap)) for s in range(n)]
        leaders.append(L.LeaderGroup(n, 0b111, 0, term, 0, log, prs))
        behind = [0] + shared + ltail[:int(rng.integers(0, len(ltail)))]
        other = [2 * t + 1 for t in AP._rand_log(rng, int(rng.integers(2, 12)), half[-1], 0.3)]
        split = AP.cap_runs([0] + shared + other, most=6)
        for k, terms in ((1, behind), (2, split)):
            fnodes[k].append(follower(terms, term=term, committed=0))
    eng = ql.LeaderGroups(LP.pack(leaders, cap, 0), cap, 0, device=DEV)
    cfg = F.Config(10, True, False)
    # round 0: a heartbeat response from both followers sets the probes off
    recs = [(g, L.Inbound(L.IN_HEARTBEAT_RESP, k, leaders[g].term)) for g in range(G) for k in (1, 2)]
    rejected = 0
    for rnd in range(40):
        ra = LP.records_arrays(recs)
        res = eng.step(ql.LeaderInbox.from_numpy(ra["group"], ra["slot"], ra["kind"], ra["index"],
                                                 ra["term"], ra["reject"], ra["hint"], ra["log_term"],
                                                 device=DEV))
        for g in leaders:
            g.msgs = []
        L.run_batch(leaders, recs)
        want = [(gi,) + m.key() for gi, g in enumerate(leaders) for m in g.msgs]
        got = [(int(m["group"]), int(m["type"]), int(m["to"]), int(m["index"]), int(m["log_term"]),
                int(m["commit"]), int(m["aux"])) for m in res.msgs]
        assert got == want, f"round {rnd}: leader messages"
        if not got:
            break
        assert all(m[1] == L.MSG_APP for m in got)
        recs = []
        for k in (1, 2):
            mine = [m for m in got if m[2] == k]
            frecs = []
            for gi, _, _, index, log_term, commit, aux in mine:
                lv = leaders[gi].log
                ents = cut_runs([s for s, _ in lv.runs], [t for _, t in lv.runs], lv.last,
                                index + 1, aux)
                frecs.append((gi, AP.app(1, leaders[gi].term, index, log_term, ents, commit)))
            if not frecs:
                continue
            nodes = fnodes[k]
            fres, fwant = run(f"round {rnd} follower {k}", nodes, frecs, cfg)
            # the restatement's nodes move on with the device's
            after = copy.deepcopy(nodes)
            A.step_batch(after, frecs, cfg)
            fnodes[k] = after
            for m in fres.responses():
                assert m["type"] == qf.MSG_APP_RESP and m["to"] == 1
                rejected += m["reject"]
                recs.append((frecs[m["i"]][0],
                             L.Inbound(L.IN_APP_RESP, k, m["term"], m["index"], m["reject"],
                                       m["hint"], m["log_term"])))
    else:
        raise AssertionError("the leaders never fell silent")
    assert rejected >= G // 2                      # the divergent tails were rejected
    for gi, g in enumerate(leaders):
        llog = A.terms_of_runs([s for s, _ in g.log.runs], [t for _, t in g.log.runs], g.log.last)
        for k in (1, 2):
            assert fnodes[k][gi].terms == llog, (gi, k)
            assert g.prs[k].match == g.log.last
        assert g.log.committed == g.log.last       # the leader's own term ends its log
    dev = eng.numpy()
    assert np.array_equal(dev["match"].reshape(G, n), np.array([[p.match for p in g.prs] for g in leaders]))
    assert np.array_equal(dev["committed"], np.array([g.log.committed for g in leaders], np.uint64))
