"""tests/follower_ref.py against the reference's own tables
(tests/golden/follower_tables.json), its three stop rules, and the fuzz
batches of tests/test_gpu_follower.py: the reference alone must reach every
counter, flag and response type there, or the GPU comparison shows nothing."""
import numpy as np
import pytest

from tests import follower_pack as P, follower_ref as F

TABLES = P.load_tables()["scenarios"]


def test_tables_hold_the_cited_tests():
    names = [sc["name"] for sc in TABLES]
    assert len(set(names)) == len(names)
    count = {k: sum(1 for n in names if n.startswith(k)) for k in (
        "testRecvMsgVote/MsgVote#", "testRecvMsgVote/MsgPreVote#", "TestFollowerVote#",
        "TestVoter#", "TestHandleHeartbeat#", "testVoteFromAnyState/MsgVote/",
        "testVoteFromAnyState/MsgPreVote/", "TestLearnerCanVote",
        "TestLeaderSupersedingWithCheckQuorum/", "TestTransferNonMember")}
    assert list(count.values()) == [21, 21, 6, 9, 2, 4, 4, 1, 3, 1], count


@pytest.mark.parametrize("sc", TABLES, ids=[sc["name"] for sc in TABLES])
def test_golden_scenario(sc):
    node = P.scenario_node(sc)
    recs = [(0, r) for r in P.scenario_recs(sc)]
    rt, rterm, stop, gf, _ = F.step_batch([node], recs, P.scenario_config(sc))
    P.check_scenario(sc, rt, rterm, node)
    assert stop == [F.NO_STOP] and not gf[0] & F.FFLAG_STOPS


def test_host_record_stops_the_group_untouched():
    n = F.Node(term=2, lead=1, last_index=5, last_term=2)
    recs = [(0, F.Rec(F.HEARTBEAT, 1, 2, 3)), (0, F.Rec(F.HOST, 1, 9)),
            (0, F.Rec(F.HEARTBEAT, 1, 2, 4))]
    rt, rterm, stop, gf, st = F.step_batch([n], recs, F.Config())
    assert rt == [F.MSG_HEARTBEAT_RESP, 0, 0] and stop == [1]
    assert gf[0] == F.FFLAG_HOST_MSG | F.FFLAG_HARDSTATE
    assert (n.term, n.committed) == (2, 3) and st["after_stop"] == 1


def test_timeout_now_stops_a_promotable_follower_and_keeps_the_term_filter():
    n = F.Node(term=2, vote=1, lead=1, role=F.LEADER | F.ROLE_PROMOTABLE, election_elapsed=4,
               heartbeat_elapsed=1)
    recs = [(0, F.Rec(F.TIMEOUT_NOW, 1, 2)),   # a leader ignores it
            (0, F.Rec(F.TIMEOUT_NOW, 3, 5)),   # higher term: follower at 5, then the campaign
            (0, F.Rec(F.VOTE, 3, 5))]
    rt, _, stop, gf, st = F.step_batch([n], recs, F.Config())
    assert rt == [0, 0, 0] and stop == [1]
    assert gf[0] == F.FFLAG_CAMPAIGN | F.FFLAG_RESET | F.FFLAG_HARDSTATE
    assert (n.term, n.vote, n.lead, n.state) == (5, 0, 0, F.FOLLOWER)
    assert n.role & F.ROLE_PROMOTABLE and (n.election_elapsed, n.heartbeat_elapsed) == (0, 0)
    assert st["role_ignored"] == 1 and st["became_follower"] == 1 and st["after_stop"] == 1
    for role in (F.FOLLOWER, F.CANDIDATE | F.ROLE_PROMOTABLE, F.PRE_CANDIDATE | F.ROLE_PROMOTABLE):
        m = F.Node(term=2, role=role)
        _, _, stop, gf, st = F.step_batch([m], [(0, F.Rec(F.TIMEOUT_NOW, 1, 2))], F.Config())
        assert stop == [F.NO_STOP] and gf == [0] and st["role_ignored"] == 1


def test_commit_past_the_log_stops_before_anything_is_applied():
    n = F.Node(term=2, vote=3, lead=0, committed=1, last_index=5, last_term=2,
               role=F.CANDIDATE, election_elapsed=7)
    recs = [(0, F.Rec(F.HEARTBEAT, 1, 4, 6)), (0, F.Rec(F.HEARTBEAT, 1, 4, 5))]
    rt, _, stop, gf, st = F.step_batch([n], recs, F.Config())
    assert rt == [0, 0] and stop == [0] and gf[0] == F.FFLAG_COMMIT_RANGE
    assert (n.term, n.vote, n.lead, n.committed, n.role, n.election_elapsed) == (2, 3, 0, 1,
                                                                                F.CANDIDATE, 7)
    assert st["became_follower"] == 0 and st["after_stop"] == 1
    # a leader at the same term never reaches commitTo
    m = F.Node(term=4, role=F.LEADER, last_index=5)
    _, _, stop, gf, st = F.step_batch([m], [(0, F.Rec(F.HEARTBEAT, 1, 4, 6))], F.Config())
    assert stop == [F.NO_STOP] and gf == [0] and st["role_ignored"] == 1
    # committed already past Commit: never decrease, no range check (log.go:238)
    k = F.Node(term=4, committed=9, last_index=5)
    rt, _, stop, _, _ = F.step_batch([k], [(0, F.Rec(F.HEARTBEAT, 1, 4, 8))], F.Config())
    assert rt == [F.MSG_HEARTBEAT_RESP] and stop == [F.NO_STOP] and k.committed == 9


def test_lower_term_answers():
    for cq, pv in P.FUZZ_CONFIGS:
        n = F.Node(term=5)
        recs = [(0, F.Rec(F.HEARTBEAT, 1, 4)), (0, F.Rec(F.PREVOTE, 2, 4)),
                (0, F.Rec(F.VOTE, 2, 4)), (0, F.Rec(F.TIMEOUT_NOW, 2, 4))]
        rt, rterm, _, gf, st = F.step_batch([n], recs, F.Config(10, cq, pv))
        hb = F.MSG_APP_RESP if cq or pv else 0
        assert rt == [hb, F.MSG_PREVOTE_RESP | F.REJECT, 0, 0]
        assert rterm == [5 if hb else 0, 5, 0, 0] and gf == [0]
        assert st["stale_answered"] + st["stale_ignored"] == 4


@pytest.mark.parametrize("seed", P.FUZZ_SEEDS)
def test_fuzz_reaches_every_path(seed):
    """Every counter, group flag and response type is non-zero for each seed
    with check_quorum; without it the lease cannot drop anything (raft.go:855),
    and with neither flag a stale heartbeat gets no MsgAppResp (raft.go:884):
    those two are the only zeros allowed, and they are required."""
    nodes, recs = P.fuzz(seed)
    assert len(nodes) == P.FUZZ_G and len(recs) == P.FUZZ_M
    assert {n.state for n in nodes} == {0, 1, 2, 3}
    for cq, pv in P.FUZZ_CONFIGS:
        _, out = P.expected(nodes, recs, P.fuzz_config(cq, pv))
        zero = {k for k, v in out["stats"].items() if v == 0}
        assert zero == (set() if cq else {"lease_dropped"}), (cq, pv, out["stats"])
        for bit in (F.FFLAG_HOST_MSG, F.FFLAG_CAMPAIGN, F.FFLAG_COMMIT_RANGE, F.FFLAG_RESET,
                    F.FFLAG_HARDSTATE):
            assert (out["gflags"] & bit).any(), (cq, pv, bit)
        types = set(out["resp_type"].tolist())
        want = {0, F.MSG_VOTE_RESP, F.MSG_VOTE_RESP | F.REJECT, F.MSG_HEARTBEAT_RESP,
                F.MSG_PREVOTE_RESP, F.MSG_PREVOTE_RESP | F.REJECT}
        assert types == (want | {F.MSG_APP_RESP} if cq or pv else want), (cq, pv, types)
        assert (out["stop_at"] != F.NO_STOP).sum() == (out["gflags"] & F.FFLAG_STOPS != 0).sum()
        # every record is counted once (became_follower counts calls, not records)
        per_record = sum(v for k, v in out["stats"].items() if k != "became_follower")
        assert per_record + int((out["stop_at"] != F.NO_STOP).sum()) == P.FUZZ_M


def test_interleave_keeps_each_groups_order():
    rng = np.random.default_rng(5)
    per = [[F.Rec(F.HEARTBEAT, g, k) for k in range(n)] for g, n in enumerate((3, 0, 5, 1))]
    out = P.interleave(per, rng)
    assert len(out) == 9
    for g in range(4):
        assert [m.term for gg, m in out if gg == g] == list(range(len(per[g])))
