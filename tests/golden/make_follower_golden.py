#!/usr/bin/env python3
"""Write tests/golden/follower_tables.json: the reference's own tests of
raft.Step on a node that receives MsgVote / MsgPreVote / MsgHeartbeat /
MsgTimeoutNow, transcribed as data.

Everything below is inputs and expected outputs read off the reference's test
files (paths relative to the reference's raft/); the node each scenario starts
from is the state the cited test builds before its Step, restated as the
fields the follower step reads (newTestRaft: follower at term 0, no vote, no
leader, both counters 0; becomeFollower / becomePreCandidate / becomeCandidate
/ becomeLeader, raft.go:686-758; a log as (lastIndex, lastTerm)).

A record is {kind, from, term, index, aux, force} with kind 0 MsgHeartbeat
(index = Commit), 1 MsgVote, 2 MsgPreVote (index / aux = Index / LogTerm),
3 MsgTimeoutNow; its "expect" holds the response (type 0 = none) and
"expect_node" the node's fields after the whole scenario.  Nothing here is
executed against the reference at test time; the JSON is committed.
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))

FOLLOWER, CANDIDATE, LEADER, PRE_CANDIDATE = 0, 1, 2, 3
PROMOTABLE = 0x80
HEARTBEAT, VOTE, PREVOTE, TIMEOUT_NOW = 0, 1, 2, 3
VOTE_RESP, HEARTBEAT_RESP, PREVOTE_RESP = 6, 9, 18
RESP_OF = {VOTE: VOTE_RESP, PREVOTE: PREVOTE_RESP}
KIND_NAME = {VOTE: "MsgVote", PREVOTE: "MsgPreVote"}


def node(*, term=0, vote=0, lead=0, committed=0, last_index=0, last_term=0, state=FOLLOWER,
         promotable=True, ee=0, he=0):
    return {"term": term, "vote": vote, "lead": lead, "committed": committed,
            "last_index": last_index, "last_term": last_term,
            "role": state | (PROMOTABLE if promotable else 0),
            "election_elapsed": ee, "heartbeat_elapsed": he}


def rec(kind, frm, term, index=0, aux=0, force=False, *, type, reject, wterm=None):
    """wterm: the response's Term, where the reference's test checks it."""
    expect = {"type": type, "reject": reject}
    if wterm is not None:
        expect["term"] = wterm
    return {"kind": kind, "from": frm, "term": term, "index": index, "aux": aux, "force": force,
            "expect": expect}


def scenario(name, cite, nd, recs, *, et=10, cq=False, pv=False, **expect_node):
    return {"name": name, "cite": cite,
            "config": {"election_timeout": et, "check_quorum": cq, "pre_vote": pv},
            "node": nd, "recs": recs, "expect_node": expect_node}


def scenarios():
    out = []

    # testRecvMsgVote (raft_test.go:1475-1558), for MsgVote and MsgPreVote:
    # node 1 alone, log {1,t2} {2,t2} (lastIndex 2, lastTerm 2), Vote =
    # voteFor, Term = max(lastTerm, logTerm) = the message's term; one
    # response of the matching type with Reject = wreject.
    rows = [(FOLLOWER, 0, 0, 0, True), (FOLLOWER, 0, 1, 0, True), (FOLLOWER, 0, 2, 0, True),
            (FOLLOWER, 0, 3, 0, False),
            (FOLLOWER, 1, 0, 0, True), (FOLLOWER, 1, 1, 0, True), (FOLLOWER, 1, 2, 0, True),
            (FOLLOWER, 1, 3, 0, False),
            (FOLLOWER, 2, 0, 0, True), (FOLLOWER, 2, 1, 0, True), (FOLLOWER, 2, 2, 0, False),
            (FOLLOWER, 2, 3, 0, False),
            (FOLLOWER, 3, 0, 0, True), (FOLLOWER, 3, 1, 0, True), (FOLLOWER, 3, 2, 0, False),
            (FOLLOWER, 3, 3, 0, False),
            (FOLLOWER, 3, 2, 2, False), (FOLLOWER, 3, 2, 1, True),
            (LEADER, 3, 3, 1, True), (PRE_CANDIDATE, 3, 3, 1, True), (CANDIDATE, 3, 3, 1, True)]
    for kind in (VOTE, PREVOTE):
        for i, (state, index, log_term, vote_for, wreject) in enumerate(rows):
            term = max(2, log_term)
            nd = node(term=term, vote=vote_for, last_index=2, last_term=2, state=state)
            out.append(scenario(f"testRecvMsgVote/{KIND_NAME[kind]}#{i}",
                                "raft/raft_test.go:1467-1558", nd,
                                [rec(kind, 2, term, index, log_term, type=RESP_OF[kind],
                                     reject=wreject)]))

    # TestFollowerVote (raft_paper_test.go:237-264): HardState{Term 1, Vote},
    # an empty log; MsgVote{From nvote, Term 1} -> exactly MsgVoteResp{To nvote,
    # Term 1, Reject wreject}.
    for i, (vote, nvote, wreject) in enumerate([(0, 1, False), (0, 2, False), (1, 1, False),
                                                (2, 2, False), (1, 2, True), (2, 1, True)]):
        out.append(scenario(f"TestFollowerVote#{i}", "raft/raft_paper_test.go:237-264",
                            node(term=1, vote=vote),
                            [rec(VOTE, nvote, 1, type=VOTE_RESP, reject=wreject, wterm=1)]))

    # TestVoter (raft_paper_test.go:824-864): a fresh node 1 of {1, 2} with
    # the row's log; MsgVote{From 2, Term 3, LogTerm, Index} -> one
    # MsgVoteResp, Reject = wreject.  ents as (lastIndex, lastTerm).
    for i, ((li, lt), log_term, index, wreject) in enumerate([
            ((1, 1), 1, 1, False), ((1, 1), 1, 2, False), ((2, 1), 1, 1, True),
            ((1, 1), 2, 1, False), ((1, 1), 2, 2, False), ((2, 1), 2, 1, False),
            ((1, 2), 1, 1, True), ((1, 2), 1, 2, True), ((2, 1), 1, 1, True)]):
        out.append(scenario(f"TestVoter#{i}", "raft/raft_paper_test.go:824-864",
                            node(last_index=li, last_term=lt),
                            [rec(VOTE, 2, 3, index, log_term, type=VOTE_RESP, reject=wreject)]))

    # TestHandleHeartbeat (raft_test.go:1281-1309): log {1,t1} {2,t2} {3,t3},
    # electionTimeout 5, becomeFollower(2, 2), committed 2; a heartbeat with
    # Commit 3 commits 3, one with Commit 1 does not decrease it; one
    # MsgHeartbeatResp each.
    for i, (commit, wcommit) in enumerate([(3, 3), (1, 2)]):
        out.append(scenario(f"TestHandleHeartbeat#{i}", "raft/raft_test.go:1281-1309",
                            node(term=2, lead=2, committed=2, last_index=3, last_term=3),
                            [rec(HEARTBEAT, 2, 2, commit, type=HEARTBEAT_RESP, reject=False)],
                            et=5, committed=wcommit))

    # testVoteFromAnyState (raft_test.go:531-603), for both types: node 1 of
    # {1, 2, 3}, Term 1, then the state's transition (follower:
    # becomeFollower(1, 3); pre-candidate: lead None; candidate: Term 2, Vote
    # 1; leader: Term 2, Vote 1, lead 1, its empty entry appended: lastIndex 1,
    # lastTerm 2).  A request from 2 at Term + 1 with LogTerm = that term,
    # Index 42: one response, not rejected.  MsgVote: follower at the new
    # term, Vote 2.  MsgPreVote: state and term unchanged, Vote None or 1.
    states = [(FOLLOWER, node(term=1, lead=3)),
              (CANDIDATE, node(term=2, vote=1, state=CANDIDATE)),
              (LEADER, node(term=2, vote=1, lead=1, last_index=1, last_term=2, state=LEADER)),
              (PRE_CANDIDATE, node(term=1, state=PRE_CANDIDATE))]
    for kind in (VOTE, PREVOTE):
        for state, nd in states:
            new_term = nd["term"] + 1
            want = (dict(state=FOLLOWER, term=new_term, vote=2) if kind == VOTE else
                    dict(state=state, term=nd["term"], vote=nd["vote"]))
            out.append(scenario(f"testVoteFromAnyState/{KIND_NAME[kind]}/state{state}",
                                "raft/raft_test.go:531-603", dict(nd),
                                [rec(kind, 2, new_term, 42, new_term, type=RESP_OF[kind],
                                     reject=False)], **want))

    # TestLearnerCanVote (raft_test.go:396-410): learner 2 (not promotable),
    # becomeFollower(1, None); MsgVote{From 1, Term 2, LogTerm 11, Index 11} ->
    # exactly one message, a MsgVoteResp that does not reject.
    out.append(scenario("TestLearnerCanVote", "raft/raft_test.go:396-410",
                        node(term=1, promotable=False),
                        [rec(VOTE, 1, 2, 11, 11, type=VOTE_RESP, reject=False)]))

    # TestLeaderSupersedingWithCheckQuorum (raft_test.go:1783-1824), node b's
    # view (checkQuorum, electionTimeout 10).  b has ticked electionTimeout
    # times without a leader when a's MsgVote at term 1 arrives: granted.  a
    # wins and replicates its empty entry: b follows a at term 1 with that
    # entry, electionElapsed 0.  c's MsgVote at term 2 (its log: the same
    # entry) arrives inside the lease: dropped without an answer, nothing
    # changes.  After electionTimeout more ticks c's MsgVote at term 3 is
    # granted: b is a follower at term 3 that voted for 3 and knows no leader.
    cq = dict(et=10, cq=True)
    out.append(scenario("TestLeaderSupersedingWithCheckQuorum/b-votes-for-a",
                        "raft/raft_test.go:1783-1824", node(ee=10),
                        [rec(VOTE, 1, 1, 0, 0, type=VOTE_RESP, reject=False, wterm=1)],
                        term=1, vote=1, lead=0, election_elapsed=0, **cq))
    b = node(term=1, vote=1, lead=1, committed=1, last_index=1, last_term=1)
    out.append(scenario("TestLeaderSupersedingWithCheckQuorum/in-lease-drop",
                        "raft/raft_test.go:1783-1824", dict(b),
                        [rec(VOTE, 3, 2, 1, 1, type=0, reject=False)],
                        term=1, vote=1, lead=1, state=FOLLOWER, election_elapsed=0, **cq))
    out.append(scenario("TestLeaderSupersedingWithCheckQuorum/grant-after-timeout",
                        "raft/raft_test.go:1783-1824", dict(b, election_elapsed=10),
                        [rec(VOTE, 3, 3, 1, 1, type=VOTE_RESP, reject=False, wterm=3)],
                        term=3, vote=3, lead=0, state=FOLLOWER, election_elapsed=0, **cq))

    # TestTransferNonMember (raft_test.go:3814-3823), its first Step: node 1 is
    # not in {2, 3, 4} (not promotable), electionTimeout 5; the local
    # MsgTimeoutNow (Term 0) does nothing: still a follower at term 0.
    out.append(scenario("TestTransferNonMember", "raft/raft_test.go:3814-3823",
                        node(promotable=False),
                        [rec(TIMEOUT_NOW, 2, 0, type=0, reject=False)],
                        et=5, state=FOLLOWER, term=0, vote=0))
    return out


def main():
    doc = {"comment": "transcribed by tests/golden/make_follower_golden.py; data only",
           "scenarios": scenarios()}
    with open(os.path.join(HERE, "follower_tables.json"), "w", encoding="utf-8") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
