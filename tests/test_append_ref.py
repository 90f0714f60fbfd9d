"""tests/append_ref.py (the CPU restatement qb_dev_follower_log_step is tested
against) replays the reference's own MsgApp tables, transcribed in
tests/golden/append_tables.json, each at the level the reference's test
calls: findConflict / maybeAppend / handleAppendEntries / Step.  Also the
fuzz generator's coverage conditions, which the GPU test relies on."""
import copy
import importlib.util
import os

import pytest

from tests import append_pack as AP, append_ref as A, follower_pack as P, follower_ref as F

T = AP.load_tables()
ROOT = AP.ROOT


def rows(key):
    return [pytest.param(i, r, id=f"{key}#{i}") for i, r in enumerate(T[key]["rows"])]


def test_golden_file_is_what_the_maker_writes():
    spec = importlib.util.spec_from_file_location(
        "make_append_golden", os.path.join(ROOT, "tests", "golden", "make_append_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.tables() == T


def test_tables_are_complete():
    assert len(T["handle_msg_app"]["rows"]) == 11
    assert len(T["find_conflict"]["rows"]) == 11
    assert len(T["maybe_append"]["rows"]) == 15
    assert len(T["check_msg_app"]["rows"]) == 5
    assert len(T["append_entries"]["rows"]) == 4
    assert len(T["fast_log_rejection"]["rows"]) == 8


@pytest.mark.parametrize("i,r", rows("find_conflict"))
def test_find_conflict(i, r):
    n = A.new_node([0] + T["find_conflict"]["log"])
    assert A._find_conflict(n, r["first"] - 1, r["ents"]) == r["w_conflict"]


@pytest.mark.parametrize("i,r", rows("maybe_append"))
def test_log_maybe_append(i, r):
    tb = T["maybe_append"]
    n = A.new_node([0] + tb["log"], committed=tb["committed"])
    m = AP.app(2, 0, r["index"], r["log_term"], r["ents"], r["commit"])
    if r["w_panic"]:
        with pytest.raises(A.GoPanic):
            A._maybe_append(n, m)
        return
    lasti, ok, _ = A._maybe_append(n, m)
    assert (lasti, ok, n.committed) == (r["w_lasti"], r["w_append"], r["w_commit"])
    if ok and r["ents"]:   # the log ends with the message's entries
        assert n.last_index == lasti and n.terms[-len(r["ents"]):] == r["ents"]


@pytest.mark.parametrize("i,r", rows("handle_msg_app"))
def test_handle_msg_app(i, r):
    tb = T["handle_msg_app"]
    n = A.new_node([0] + tb["log"], term=tb["term"], committed=tb["committed"])
    m = AP.app(2, r["m_term"], r["index"], r["log_term"], r["ents"], r["commit"])
    _, reject, _, _, _ = A._handle_append_entries(n, m, A.new_stats())
    assert (n.last_index, n.committed, reject) == (r["w_index"], r["w_commit"], r["w_reject"])


@pytest.mark.parametrize("i,r", rows("check_msg_app"))
def test_follower_check_msg_app(i, r):
    tb = T["check_msg_app"]
    n = A.new_node([0] + tb["log"], term=tb["term"], lead=tb["lead"], committed=tb["committed"])
    rt, rterm, gf, idx, hint, lterm, _ = A.step_app(
        n, AP.app(tb["from"], tb["term"], r["index"], r["log_term"], []), F.Config(), A.new_stats())
    assert rt & 0x7F == A.MSG_APP_RESP and rterm == tb["term"] and gf == 0
    assert (idx, bool(rt & A.REJECT), hint or 0, lterm or 0) == (
        r["w_index"], r["w_reject"], r["w_hint"], r["w_log_term"])


@pytest.mark.parametrize("i,r", rows("append_entries"))
def test_follower_append_entries(i, r):
    tb = T["append_entries"]
    n = A.new_node([0] + tb["log"], term=tb["term"], lead=tb["lead"])
    out = A.step_app(n, AP.app(tb["from"], tb["term"], r["index"], r["log_term"], r["ents"]),
                     F.Config(), A.new_stats())
    assert n.terms[1:] == r["w_log"]
    # the unstable entries are the ones the host's log takes: from app_from on
    af = out[6]
    assert (n.terms[af:] if af else []) == r["w_unstable"]
    assert bool(out[2] & A.FFLAG_APPENDED) == bool(r["w_unstable"])


@pytest.mark.parametrize("i,r", rows("fast_log_rejection"))
def test_fast_log_rejection_followers_side(i, r):
    tb = T["fast_log_rejection"]
    n = A.new_node([0] + r["follower_log"], term=0)
    lead = r["leader_log"]
    rt, rterm, gf, idx, hint, lterm, _ = A.step_app(
        n, AP.app(tb["from"], tb["term"], len(lead), lead[-1], [tb["term"]]), F.Config(),
        A.new_stats())
    assert rt == A.MSG_APP_RESP | A.REJECT and idx == len(lead) and rterm == tb["term"]
    assert (lterm, hint) == (r["w_hint_term"], r["w_hint_index"])
    assert gf == A.FFLAG_RESET and (n.term, n.lead) == (tb["term"], tb["from"])  # raft.go:876-877


def test_runs_round_trip_and_stops():
    terms = [0, 1, 1, 2, 5, 5, 5, 9]
    starts, rt = A.runs_of(terms, 4)
    assert (starts, rt) == ([3, 4, 6, 7, 10], [0, 1, 2, 5, 9])
    assert A.terms_of_runs(starts, rt, 10) == terms
    cfg, st = F.Config(), A.new_stats()
    # a gap: LogTerm 0 "matches" past the end, the entry does not (LOG_CONFLICT)
    n = A.new_node([0, 1, 1], term=1)
    before = copy.deepcopy(n)
    assert A.step_app(n, AP.app(2, 3, 5, 0, [1]), cfg, st)[:3] == (0, 0, A.FFLAG_LOG_CONFLICT)
    assert n == before and st == A.new_stats()        # not even the higher term is applied
    # zero terms past the end match; committing them is commitTo's panic
    assert A.step_app(n, AP.app(2, 1, 2, 1, [0, 0], 4), cfg, st)[:3] == (0, 0, F.FFLAG_COMMIT_RANGE)
    # log.go:94-95 through raft.Step: only where the entries' indexes wrap (the log
    # ends at 2^64 - 1; entry 0 "matches" at index 0, entry 1 conflicts at 1 <= committed)
    top = (1 << 64) - 1
    n = A.new_node([1, 1, 1], top - 1, term=1, committed=top)
    before = copy.deepcopy(n)
    assert n.last_index == top
    assert A.step_app(n, AP.app(2, 5, top, 1, [0, 3], 7), cfg, st)[:3] == (0, 0, A.FFLAG_LOG_CONFLICT)
    assert n == before and st == A.new_stats()
    # a ninth run
    n = A.new_node([0] + list(range(1, 7)), term=9)
    assert A.step_app(n, AP.app(2, 9, 6, 6, [7]), cfg, st)[2] == A.FFLAG_APPENDED
    assert A.step_app(n, AP.app(2, 9, 7, 7, [8]), cfg, st)[:3] == (0, 0, A.FFLAG_LOG_RUNS)
    assert n.last_index == 7 and st["app_accepted"] == 1


@pytest.mark.parametrize("seed", AP.FUZZ_SEEDS)
@pytest.mark.parametrize("cq,pv", P.FUZZ_CONFIGS)
def test_fuzz_generator_covers_the_paths(seed, cq, pv):
    """The conditions the GPU fuzz asserts before it compares the device."""
    nodes, recs = AP.fuzz(seed)
    _, _, out = AP.expected(nodes, recs, P.fuzz_config(cq, pv))
    check_fuzz_coverage(out, len(recs))


def check_fuzz_coverage(out, M):
    st = out["stats"]
    assert st["after_stop"] <= 0.25 * M, st
    for k in ("app_accepted", "app_truncated", "app_rejected", "app_below_commit",
              "entries_appended", "heartbeats", "granted", "rejected", "became_follower"):
        assert st[k] >= 1, (k, st)
    seen = 0
    for f in out["gflags"].tolist():
        seen |= f
    for name, bit in (("HOST_MSG", F.FFLAG_HOST_MSG), ("CAMPAIGN", F.FFLAG_CAMPAIGN),
                      ("COMMIT_RANGE", F.FFLAG_COMMIT_RANGE), ("LOG_CONFLICT", A.FFLAG_LOG_CONFLICT),
                      ("LOG_RUNS", A.FFLAG_LOG_RUNS), ("APPENDED", A.FFLAG_APPENDED)):
        assert seen & bit, f"no group with {name}"
