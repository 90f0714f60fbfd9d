"""tests/snapshot_ref.py against the reference's own tables
(tests/golden/snapshot_tables.json, transcribed by make_snapshot_golden.py),
and the restatement's own rules where the tables are silent: the stop, the
term filter and the roles.  No GPU."""
import copy
import json
import os

import pytest

from tests import snapshot_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "snapshot_tables.json"), encoding="utf-8") as f:
        return json.load(f)


def make_node(d) -> S.Node:
    return S.Node(id=d["id"], term=d["term"], vote=d["vote"], lead=d["lead"],
                  committed=d["committed"], state=d["state"], first_index=d["first"],
                  terms=list(d["terms"]), offset=d["offset"],
                  snap=tuple(d["snap"]) if d["snap"] else None)


def make_snap(d, frm=0, term=0) -> S.Snap:
    return S.Snap(frm=frm, term=term, index=d["index"], sterm=d["term"], cs=d["cs"])


def check_want(n: S.Node, want: dict, where):
    for k, v in want.items():
        if k == "term_at":
            for i, t in v:
                assert S.log_term(n, i) == t, (where, k, i)
        elif k == "entries":
            assert len(n.terms) - 1 == v, (where, k)
        elif k == "first":
            assert n.first_index == v, (where, k)
        elif k == "snap":
            assert n.snap == tuple(v), (where, k)
        else:
            assert getattr(n, k) == v, (where, k)


def table_nodes(doc):
    """Every (node, Snap) the tables step or restore, as fresh objects: the
    GPU test runs them as one batch."""
    out = []
    for case in doc["restore"] + doc["step"]:
        n = make_node(case["node"])
        for st in case["steps"]:
            m = make_snap(st["snap"], st.get("from", 0), st.get("term", 0))
            out.append((copy.deepcopy(n), m))
            S.step(n, m, S.new_stats())
    for case in doc["log"]:
        i, t = case["restore"]
        out.append((make_node(case["node"]), S.Snap(frm=9, term=0, index=i, sterm=t,
                                                    cs={"voters": [case["node"]["id"]]})))
    return out


@pytest.mark.parametrize("case", golden()["restore"], ids=lambda c: c["name"])
def test_restore_tables(case):
    n = make_node(case["node"])
    for k, st in enumerate(case["steps"]):
        ok, _ = S.restore(n, make_snap(st["snap"]))
        assert ok == st["ok"], (case["name"], k)
        check_want(n, st["want"], (case["name"], k))


@pytest.mark.parametrize("case", golden()["step"], ids=lambda c: c["name"])
def test_step_tables(case):
    n = make_node(case["node"])
    for k, st in enumerate(case["steps"]):
        f, resp = S.step(n, make_snap(st["snap"], st["from"], st["term"]), S.new_stats())
        assert f & S.SNF_RESTORED and resp is not None, case["name"]
        if "resp" in st:
            assert list(resp) == [S.MSG_APP_RESP] + st["resp"], case["name"]
        check_want(n, st["want"], (case["name"], k))
        assert not n.promotable and n.pending & S.RDP_MSGS


@pytest.mark.parametrize("case", golden()["log"], ids=lambda c: c["name"])
def test_log_tables(case):
    n = make_node(case["node"])
    S.log_restore(n, *case["restore"])
    check_want(n, case["want"], case["name"])


def test_the_tables_hold_every_test_the_issue_names():
    names = {c["name"] for part in golden().values() for c in part}
    assert names == {"TestRestore", "TestRestoreWithLearner", "TestRestoreWithVotersOutgoing",
                     "TestRestoreVoterToLearner", "TestRestoreLearnerPromotion",
                     "TestRestoreIgnoreSnapshot", "TestRestoreFromSnapMsg", "TestLogRestore",
                     "TestUnstableRestore", "TestTermWithUnstableSnapshot",
                     "snapshot_succeed_via_app_resp (follower)"}


def test_committed_json_is_what_the_maker_writes(tmp_path, monkeypatch):
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "make_snapshot_golden", os.path.join(ROOT, "tests", "golden", "make_snapshot_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(mod, "HERE", str(tmp_path))
    mod.main()
    with open(tmp_path / "snapshot_tables.json", encoding="utf-8") as f:
        assert json.load(f) == golden()


# ---- the rules the tables do not reach ----
def follower(**kw) -> S.Node:
    d = dict(id=1, term=5, vote=2, lead=2, committed=3, first_index=1, terms=[0, 1, 1, 2, 2, 3],
             offset=6, election_elapsed=4, heartbeat_elapsed=3)
    d.update(kw)
    return S.Node(**d)


MEMBER = {"voters": [1, 2, 3]}


def test_the_stop_leaves_the_node_and_the_stats_but_its_counter_untouched():
    """A zero snapshot term past the log's end matches (term() is 0 outside
    the log) and commitTo panics: nothing applied, the filter's effect included."""
    n = follower(state=S.CANDIDATE)
    before = copy.deepcopy(n)
    st = S.new_stats()
    f, resp = S.step(n, S.Snap(frm=3, term=9, index=6, sterm=0, cs=MEMBER), st)
    assert f == S.SNF_COMMIT_RANGE and resp is None and n == before
    assert st == dict(S.new_stats(), commit_range=1)
    # a non-zero term there restores instead
    f, resp = S.step(n, S.Snap(frm=3, term=9, index=6, sterm=4, cs=MEMBER), st)
    assert f == S.SNF_RESTORED | S.SNF_RESET | S.SNF_HARDSTATE and resp == (S.MSG_APP_RESP, 9, 6)
    assert (n.term, n.vote, n.lead, n.state, n.promotable) == (9, 0, 3, S.FOLLOWER, False)
    assert (n.first_index, n.terms, n.offset, n.snap, n.committed) == (7, [4], 7, (6, 4), 6)


@pytest.mark.parametrize("state", (S.FOLLOWER, S.CANDIDATE, S.LEADER, S.PRE_CANDIDATE))
def test_term_filter_and_roles(state):
    snap = dict(index=4, sterm=2, cs=MEMBER)   # inside the log, matching: fast-forward
    n = follower(state=state)
    f, resp = S.step(n, S.Snap(frm=3, term=4, **snap), S.new_stats())       # lower: ignored
    assert f == S.SNF_STALE and resp is None and n == follower(state=state)
    n = follower(state=state)
    f, resp = S.step(n, S.Snap(frm=3, term=5, **snap), S.new_stats())       # equal
    if state == S.LEADER:
        assert f == S.SNF_ROLE_IGNORED and resp is None and n == follower(state=state)
    else:
        reset = S.SNF_RESET if state != S.FOLLOWER else 0
        assert f == S.SNF_FAST_FORWARD | S.SNF_HARDSTATE | reset
        assert resp == (S.MSG_APP_RESP, 5, 4) and n.committed == 4 and n.lead == 3
        assert (n.vote, n.election_elapsed) == (2, 0) and n.state == S.FOLLOWER
        assert n.heartbeat_elapsed == (0 if reset else 3) and n.promotable
    n = follower(state=state)
    f, resp = S.step(n, S.Snap(frm=3, term=7, **snap), S.new_stats())       # higher: any role
    assert f == S.SNF_FAST_FORWARD | S.SNF_HARDSTATE | S.SNF_RESET
    assert (n.term, n.vote, n.lead, n.state) == (7, 0, 3, S.FOLLOWER) and resp == (S.MSG_APP_RESP, 7, 4)


def test_membership_and_old():
    for cs, member in (({"voters": [1]}, True), ({"learners": [1]}, True),
                       ({"voters_outgoing": [1]}, True), ({"learners_next": [1]}, False),
                       ({"voters": [2, 3]}, False), ({}, False)):
        n = follower()
        f, resp = S.step(n, S.Snap(frm=2, term=5, index=9, sterm=3, cs=cs), S.new_stats())
        assert bool(f & S.SNF_RESTORED) == member and bool(f & S.SNF_NOT_MEMBER) == (not member)
        assert resp == (S.MSG_APP_RESP, 5, 9 if member else 3)
    n = follower()
    f, resp = S.step(n, S.Snap(frm=2, term=0, index=3, sterm=9, cs={}), S.new_stats())  # Term 0: local
    assert f == S.SNF_OLD and resp == (S.MSG_APP_RESP, 5, 3) and n.lead == 2


def test_snapshot_call_refuses_duplicate_groups_and_flags_bad_ones():
    nodes = [follower(), follower()]
    m = S.Snap(frm=2, term=5, index=9, sterm=3, cs=MEMBER)
    with pytest.raises(AssertionError):
        S.snapshot_call(nodes, [(0, m), (0, m)])
    out = S.snapshot_call(nodes, [(5, m), (1, m)], pending=False)
    assert out["sflags"][0] == S.SNF_BAD_GROUP and out["stats"]["bad_group"] == 1
    assert out["sflags"][1] & S.SNF_RESTORED and nodes[1].pending == 0
