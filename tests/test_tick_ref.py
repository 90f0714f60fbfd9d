"""tests/tick_ref.py (the CPU restatement of raft.tick()) against the
reference's own tests transcribed in tests/golden/tick_tables.json, hand cases
for each branch of the tick, and the numpy-vectorised restatement the bench
row uses (tests/tick_pack.py np_tick) against tick_ref on a ragged batch."""
import numpy as np
import pytest

from oracle import leader_ref as L
from tests import tick_pack as P, tick_ref as T
from tests.leader_scenarios import msg_dict

SCENARIOS = P.load_tables()["scenarios"]


def run_scenario_ref(sc):
    n = P.build_node(sc)
    for k, op in enumerate(sc["ops"]):
        if op["op"] == "hb_resp":
            n.group.prs[op["slot"]].recent_active = True  # raft.go:1284-1285
            continue
        n.msgs = []
        T.tick(n, sc["election_timeout"], sc["heartbeat_timeout"], sc["check_quorum"])
        P.check_tick_expect(f"{sc['name']} op{k}", op["expect"], [msg_dict(m) for m in n.msgs], n)
    return n


@pytest.mark.parametrize("sc", SCENARIOS, ids=[s["name"] for s in SCENARIOS])
def test_golden_scenarios(sc):
    run_scenario_ref(sc)


def test_golden_covers_the_cited_tests():
    names = {s["name"].split("#")[0] for s in SCENARIOS}
    assert names == {"TestBcastBeat", "TestRecvMsgBeat", "TestLeaderStepdownWhenQuorumActive",
                     "TestLeaderStepdownWhenQuorumLost", "TestLeaderTransferTimeout",
                     "TestLeaderBcastBeat"}


def node(role, ns=3, vin=0b111, vout=0, leader=0, active=(0, 0, 0), match=(9, 4, 7), committed=5,
         ee=0, he=0, rt=10, transferee=L.NO_SLOT, ctx=()):
    g = P.make_group(ns, vin, vout, leader, committed, list(match), list(active), transferee, ctx)
    return T.TickNode(g, role, ee, he, rt)


def active_bits(n):
    return [p.recent_active for p in n.group.prs]


def test_non_leader_counts_and_hups_only_when_promotable():
    for role in (T.FOLLOWER, T.CANDIDATE, T.PRE_CANDIDATE):
        n = node(role | T.ROLE_PROMOTABLE, ee=8, he=3, rt=10)
        assert T.tick(n, 5, 1, True) == 0 and (n.election_elapsed, n.heartbeat_elapsed) == (9, 3)
        assert T.tick(n, 5, 1, True) == T.TFLAG_HUP and n.election_elapsed == 0  # 10 >= 10
        assert n.role == role | T.ROLE_PROMOTABLE and not n.msgs
        n = node(role, ee=20, rt=10)  # not promotable: only counts
        assert T.tick(n, 5, 1, True) == 0 and n.election_elapsed == 21
    n = node(T.FOLLOWER | T.ROLE_PROMOTABLE, ee=15, rt=10)  # already past: >=
    assert T.tick(n, 5, 1, True) == T.TFLAG_HUP


def test_beat_commit_is_min_of_match_and_committed_and_skips_the_leader():
    n = node(T.LEADER, leader=1, ctx=(77, 88))
    assert T.tick(n, 10, 1, False) == T.TFLAG_BEAT
    assert [m.key() for m in n.msgs] == [(8, 0, 0, 0, 5, 88), (8, 2, 0, 0, 5, 88)]
    n = node(T.LEADER, leader=0, he=0)
    assert T.tick(n, 10, 2, False) == 0 and n.heartbeat_elapsed == 1 and not n.msgs
    n.msgs = []
    assert T.tick(n, 10, 2, False) == T.TFLAG_BEAT and n.heartbeat_elapsed == 0
    assert [m.key() for m in n.msgs] == [(8, 1, 0, 0, 4, 0), (8, 2, 0, 0, 5, 0)]


def test_leader_without_progress_beats_everyone_and_activates_nobody():
    n = node(T.LEADER, leader=5, ee=9, active=(1, 1, 0))
    tf = T.tick(n, 10, 1, True)
    assert tf == T.TFLAG_CHECK_QUORUM | T.TFLAG_BEAT and [m.to for m in n.msgs] == [0, 1, 2]
    assert active_bits(n) == [False, False, False]
    n = node(T.LEADER, leader=5, ee=9, active=(1, 0, 0))  # 1 of 3: nobody vouches for the leader
    assert T.tick(n, 10, 1, True) == T.TFLAG_CHECK_QUORUM | T.TFLAG_STEPPED_DOWN


def test_sweep_keeps_the_leader_active_clears_the_rest_learners_included():
    n = node(T.LEADER, ns=4, vin=0b0111, leader=0, active=(0, 1, 0, 1), match=(9, 4, 7, 1), ee=9)
    tf = T.tick(n, 10, 1, True)
    assert tf == T.TFLAG_CHECK_QUORUM | T.TFLAG_BEAT and n.role == T.LEADER
    assert active_bits(n) == [True, False, False, False]
    assert (n.election_elapsed, n.heartbeat_elapsed) == (0, 0) and len(n.msgs) == 3
    # a learner's activity does not count: the leader alone of three voters
    n = node(T.LEADER | T.ROLE_PROMOTABLE, ns=4, vin=0b0111, leader=0, active=(0, 0, 0, 1),
             match=(9, 4, 7, 1), ee=9, he=0, transferee=2)
    tf = T.tick(n, 10, 1, True)
    assert tf == T.TFLAG_CHECK_QUORUM | T.TFLAG_STEPPED_DOWN  # no beat, no TRANSFER_ABORTED
    assert n.role == T.FOLLOWER | T.ROLE_PROMOTABLE and not n.msgs
    assert active_bits(n) == [False] * 4 and n.group.transferee == L.NO_SLOT
    assert (n.election_elapsed, n.heartbeat_elapsed) == (0, 0)


def test_joint_quorum_needs_both_halves_and_an_empty_half_wins():
    n = node(T.LEADER, ns=4, vin=0b0011, vout=0b1100, leader=0, active=(0, 1, 0, 0),
             match=(1, 1, 1, 1), ee=9)
    assert T.tick(n, 10, 1, True) & T.TFLAG_STEPPED_DOWN      # outgoing half silent
    n = node(T.LEADER, ns=4, vin=0b0011, vout=0b1100, leader=0, active=(0, 1, 1, 1),
             match=(1, 1, 1, 1), ee=9)
    assert not T.tick(n, 10, 1, True) & T.TFLAG_STEPPED_DOWN
    n = node(T.LEADER, ns=2, vin=0, vout=0, leader=0, active=(0, 0), match=(1, 1), ee=9)
    assert not T.tick(n, 10, 1, True) & T.TFLAG_STEPPED_DOWN  # no voters at all: VoteWon
    n = node(T.LEADER, ns=1, vin=1, leader=0, active=(0,), match=(3,), ee=9)  # singleton
    assert T.tick(n, 10, 1, True) == T.TFLAG_CHECK_QUORUM | T.TFLAG_BEAT and not n.msgs


def test_without_check_quorum_the_sweep_only_aborts_the_transfer():
    n = node(T.LEADER, ee=9, active=(0, 1, 1), transferee=1)
    tf = T.tick(n, 10, 1, False)
    assert tf == T.TFLAG_TRANSFER_ABORTED | T.TFLAG_BEAT and n.group.transferee == L.NO_SLOT
    assert active_bits(n) == [False, True, True] and n.election_elapsed == 0
    n = node(T.LEADER, ee=3, transferee=1)
    assert T.tick(n, 10, 1, False) == T.TFLAG_BEAT and n.group.transferee == 1


def test_vectorised_restatement_equals_tick_ref():
    """np_tick (what tools/bench_configs.py checks the 4M-group row against)
    == tick_ref on ragged seeded batches, every array and counter, over
    consecutive ticks."""
    for seed, (et, ht, cq), rcap in ((1, (10, 1, 1), 4), (2, (3, 3, 1), 0), (3, (5, 7, 1), 16),
                                     (4, (1, 1, 1), 4), (5, (10, 1, 0), 4)):
        rng = np.random.default_rng(seed)
        nodes = P.random_nodes(rng, 300, rcap, et, ht)
        a, t = P.pack_nodes(nodes, rcap)
        S = int(a["off"][-1])
        hc_r, hx_r = np.full(S, P.FILL, np.uint64), np.full(len(nodes), P.FILL, np.uint64)
        hc_v, hx_v = hc_r.copy(), hx_r.copy()
        for k in range(2 * et + 2):
            mask = rng.random(S) < 0.3
            P.set_recent_active(nodes, a["off"], mask)
            a["pstate"][mask] |= 8
            tf_r, st_r = P.ref_tick(nodes, a["off"], et, ht, cq, hc_r, hx_r)
            tf_v, st_v = P.np_tick(a, t, rcap, et, ht, cq, hc_v, hx_v)
            want_a, want_t = P.pack_nodes(nodes, rcap)
            where = f"seed {seed} tick {k}"
            assert np.array_equal(tf_v, tf_r) and st_v == st_r, where
            for key in want_a:
                assert np.array_equal(a[key], want_a[key]), (where, key)
            for key in want_t:
                assert np.array_equal(t[key], want_t[key]), (where, key)
            assert np.array_equal(hc_v, hc_r) and np.array_equal(hx_v, hx_r), where

