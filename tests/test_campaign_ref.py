"""tests/campaign_ref.py against the reference's own tests of the campaign
path (tests/golden/campaign_tables.json), the packing round trip, and whole
elections through the restatements (tests/campaign_loop.py).  No GPU."""
import copy

import numpy as np
import pytest

from tests import campaign_loop as loop, campaign_pack as P, campaign_ref as R, tick_ref as T

SCENARIOS = P.load_tables()["scenarios"]


def replay(sc, apply):
    """A golden scenario's ops over its node; apply(node, action) -> (cflags,
    requests) runs one action byte."""
    n = P.build_node(sc)
    ids = sc["node"]["ids"]
    slot = {i: s for s, i in enumerate(ids)}
    for k, op in enumerate(sc["ops"]):
        where = f"{sc['name']} op{k}"
        if op["op"] == "vote_resp":
            act = P.record_vote(n, slot[op["from"]], not op["reject"])
            if act != R.CAMP_NONE:
                cf, _ = apply(n, act)
                assert not cf & R.CFLAG_IGNORED, where
            continue
        act = op["action"] | (R.CAMP_PENDING_CONF if op["pending_conf"] else 0)
        cf, reqs = apply(n, act)
        P.check_expect(where, op["expect"], cf, reqs, n, ids)
    P.check_expect(sc["name"], sc["expect_node"], 0, [], n, ids)
    return n


@pytest.mark.parametrize("sc", SCENARIOS, ids=[s["name"] for s in SCENARIOS])
def test_golden_scenarios(sc):
    st = R.new_stats()

    def apply(n, act):
        cf = R.step(n, act, sc["pre_vote"], st)
        return cf, n.reqs
    replay(sc, apply)


def test_golden_file_is_what_the_script_writes(tmp_path):
    import importlib.util
    import json
    import os
    path = os.path.join(P.ROOT, "tests", "golden", "make_campaign_golden.py")
    spec = importlib.util.spec_from_file_location("make_campaign_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert json.loads(json.dumps(mod.scenarios())) == SCENARIOS


def test_single_voter_commits_only_its_own_quorum():
    """becomeLeader's maybeCommit: {self} alone, {self} with learners, and a
    joint config whose outgoing half is {self} but whose incoming half is not."""
    st = R.new_stats()
    for ns, vin, vout, want in ((1, 1, 0, 8), (3, 1, 0, 8), (3, 1, 1, 8), (3, 7, 1, 3), (3, 0, 1, 8)):
        n = P.make_node(ns, vin, vout, 0, term=4, last_index=7, last_term=4, committed=3,
                        role=R.CANDIDATE | R.ROLE_PROMOTABLE)
        cf = R.step(n, R.CAMP_WON, False, st)
        assert cf & R.CFLAG_BECAME_LEADER and n.group.log.committed == want, (ns, vin, vout)
        assert bool(cf & R.CFLAG_HARDSTATE) == (want != 3)
        own = n.group.prs[0]
        assert (own.match, own.next, own.state) == (8, 9, 1)


def test_pack_unpack_round_trip():
    rng = np.random.default_rng(5)
    nodes = P.random_nodes(rng, 300, readq_cap=4)
    a, e = P.pack_nodes(nodes, 4)
    st = R.new_stats()
    acted = copy.deepcopy(nodes)
    for n, act in zip(acted, P.random_actions(rng, 300)):
        R.step(n, int(act), True, st)
    assert [P.state_key(n) for n in acted] != [P.state_key(n) for n in nodes]
    P.unpack_into(acted, a, e, 4)   # back to the packed state
    assert [P.state_key(n) for n in acted] == [P.state_key(n) for n in nodes]
    a2, e2 = P.pack_nodes(acted, 4)
    assert all(np.array_equal(a[k], a2[k]) for k in a) and all(np.array_equal(e[k], e2[k]) for k in e)
    assert sum(st.values()) > 0 and all(st[k] > 0 for k in R.CSTAT_NAMES), st


@pytest.mark.parametrize("pre_vote", [False, True])
def test_three_node_election_reaches_a_leader(pre_vote):
    """One candidate per group with an up-to-date log: tick -> campaign ->
    follower step -> record votes -> tally -> campaign ends with that node
    leading, its peers following it at the new term, and the leader beating."""
    nodes, rand = loop.make_cluster(3, 3, 40)
    for g in range(40):   # exactly one candidate, and its log is the longest
        cand = g % 3
        for j in range(3):
            rand[j][g] = loop.ET if j == cand else loop.LATE
        nodes[cand][g].group.log.last, nodes[cand][g].last_term = 60, 9
    term0 = [nodes[0][g].group.term for g in range(40)]
    c = loop.RefCluster(nodes, rand, pre_vote)
    rounds, tf = loop.run_election(c)
    assert rounds == (3 if pre_vote else 2)
    for g in range(40):
        cand = g % 3
        n = nodes[cand][g]
        assert n.state == R.LEADER and n.lead == cand + 1 and n.group.term == term0[g] + 1
        assert tf[cand][g] & T.TFLAG_BEAT
        own = n.group.prs[cand]
        assert (own.state, own.match, own.next) == (1, 61, 62)
        for j in range(3):
            if j != cand:
                p = n.group.prs[j]
                assert (p.state, p.probe_sent, p.match, p.next) == (0, True, 0, 61)
                f = nodes[j][g]
                assert f.state == R.FOLLOWER and f.vote == cand + 1 and f.group.term == term0[g] + 1


@pytest.mark.parametrize("pre_vote", [False, True])
def test_split_vote_ends_lost_on_every_candidate(pre_vote):
    """All three nodes time out together: each votes for itself and rejects
    the others, every tally is VoteLost and every node is a follower again."""
    nodes, rand = loop.make_cluster(4, 3, 20)
    for g in range(20):
        for j in range(3):
            rand[j][g] = loop.ET
            nodes[j][g].group.log.last, nodes[j][g].last_term = 9, 2   # equal logs
    c = loop.RefCluster(nodes, rand, pre_vote)
    _, tf = loop.run_election(c)
    for j in range(3):
        assert all(n.state == R.FOLLOWER and n.vote == j + 1 and n.lead == 0 for n in nodes[j])
        assert not (tf[j] & T.TFLAG_BEAT).any()


@pytest.mark.parametrize("N", [3, 5])
def test_seeded_elections_elect_at_most_one_leader_per_group(N):
    nodes, rand = loop.make_cluster(11, N, 120)
    log = []
    loop.run_election(loop.RefCluster(nodes, rand, True), log)
    leaders = np.array([[n.state == R.LEADER for n in nodes[j]] for j in range(N)])
    assert leaders.sum(axis=0).max() == 1 and 0 < leaders.sum() < 120
    assert len(log) == 3
