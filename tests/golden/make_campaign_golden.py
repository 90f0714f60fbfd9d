#!/usr/bin/env python3
"""Write tests/golden/campaign_tables.json: the reference's own tests of
Step(MsgHup) -> hup -> campaign and of the election's outcome, transcribed as
data.

Everything below is inputs and expected outputs read off the reference's test
files (paths relative to the reference's raft/); the node each scenario starts
from is the state the cited test builds before its Step, restated as the
fields the campaign reads (newTestRaft: follower at term 0, no vote, no
leader, an empty log; becomeFollower / becomeCandidate, raft.go:686-706; a log
as (lastIndex, lastTerm, committed)).

A node is {ids (the Progress map's IDs ascending = the slots), voters /
voters_out / self (IDs), term, vote, lead, state, last_index, last_term,
committed, votes (IDs that granted)}; the promotable bit of the role byte is
set on every node, so the membership part of promotable() is the engine's to
find.  An op is
  {"op": "action", "action": QB_CAMP_*, "pending_conf": bool, "expect": {...}}
  {"op": "vote_resp", "from": id, "reject": bool}: RecordVote + TallyVotes on a
      (pre-)candidate, then the action QB_CAMP_WON / QB_CAMP_LOST if decided
      (stepCandidate, raft.go:1399-1414); any other role ignores it.
"expect" holds what the reference's test checks after that Step: state, term,
lead, self_vote, ignored (hup returned early), reqs as [type, to, term, index,
log_term, transfer] in ascending To order (the tests sort their messages);
"expect_node" the same after the whole scenario.  Nothing here is executed
against the reference at test time; the JSON is committed.
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))

FOLLOWER, CANDIDATE, LEADER, PRE_CANDIDATE = 0, 1, 2, 3
NONE, HUP, TRANSFER, WON, LOST = 0, 1, 2, 3, 4
MSG_VOTE, MSG_PREVOTE = 5, 17


def node(ids, self_id, *, voters=None, voters_out=(), term=0, vote=0, lead=0, state=FOLLOWER,
         last_index=0, last_term=0, committed=0, votes=()):
    return {"ids": list(ids), "voters": list(ids if voters is None else voters),
            "voters_out": list(voters_out), "self": self_id, "term": term, "vote": vote,
            "lead": lead, "state": state, "last_index": last_index, "last_term": last_term,
            "committed": committed, "votes": list(votes)}


def action(code, pending_conf=False, **expect):
    return {"op": "action", "action": code, "pending_conf": pending_conf, "expect": expect}


def vote_resp(frm, reject=False):
    return {"op": "vote_resp", "from": frm, "reject": reject}


def scenario(name, cite, nd, ops, *, pre_vote=False, **expect_node):
    return {"name": name, "cite": cite, "pre_vote": pre_vote, "node": nd, "ops": ops,
            "expect_node": expect_node}


def votes_to(peers, term, index=0, log_term=0, transfer=False, type=MSG_VOTE):
    return [[type, p, term, index, log_term, transfer] for p in peers]


def scenarios():
    out = []

    # testNonleaderStartElection (raft_paper_test.go:134-190): peers 1 2 3,
    # becomeFollower(1, 2) or becomeCandidate() (term 0 -> 1, Vote 1, own
    # vote), then ticks past the election timeout: one MsgHup.  Term 2,
    # StateCandidate, Votes[r.id], MsgVote {To 2, Term 2} {To 3, Term 2}
    # (Index / LogTerm 0: the log is empty).
    for name, nd in (("TestFollowerStartElection", node([1, 2, 3], 1, term=1, lead=2)),
                     ("TestCandidateStartNewElection",
                      node([1, 2, 3], 1, term=1, vote=1, state=CANDIDATE, votes=[1]))):
        out.append(scenario(name, "raft/raft_paper_test.go:134-190", nd,
                            [action(HUP, term=2, state=CANDIDATE, self_vote=True,
                                    reqs=votes_to([2, 3], 2))]))

    # TestVoteRequest (raft_paper_test.go:776-823): a MsgApp from 2 at term
    # wterm - 1 leaves the entries in the log (follower of 2 at that term);
    # the election timeout then sends MsgVote to 2 and 3 (sorted) with Term
    # wterm and the last entry's Index / Term.
    for j, (last_index, last_term, wterm) in enumerate([(1, 1, 2), (2, 2, 3)]):
        nd = node([1, 2, 3], 1, term=wterm - 1, lead=2, last_index=last_index, last_term=last_term)
        out.append(scenario(f"TestVoteRequest#{j}", "raft/raft_paper_test.go:776-823", nd,
                            [action(HUP, reqs=votes_to([2, 3], wterm, last_index, last_term))]))

    # TestLeaderElectionInOneRoundRPC (raft_paper_test.go:192-235): a fresh
    # node 1 of `size` peers, MsgHup, then the MsgVoteResp of the table at
    # r.Term (the test ranges over a map: any order; ascending here).  The
    # state after, and Term 1 in every case.
    table = [
        (1, {}, LEADER), (3, {2: True, 3: True}, LEADER), (3, {2: True}, LEADER),
        (5, {2: True, 3: True, 4: True, 5: True}, LEADER), (5, {2: True, 3: True, 4: True}, LEADER),
        (5, {2: True, 3: True}, LEADER),
        (3, {2: False, 3: False}, FOLLOWER), (5, {2: False, 3: False, 4: False, 5: False}, FOLLOWER),
        (5, {2: True, 3: False, 4: False, 5: False}, FOLLOWER),
        (3, {}, CANDIDATE), (5, {2: True}, CANDIDATE), (5, {2: False, 3: False}, CANDIDATE),
        (5, {}, CANDIDATE),
    ]
    for i, (size, votes, wstate) in enumerate(table):
        ops = [action(HUP)] + [vote_resp(p, not v) for p, v in sorted(votes.items())]
        out.append(scenario(f"TestLeaderElectionInOneRoundRPC#{i}",
                            "raft/raft_paper_test.go:192-235", node(range(1, size + 1), 1), ops,
                            state=wstate, term=1))

    # TestSingleNodeCandidate / TestSingleNodePreCandidate (raft_test.go:973-992):
    # a network of one, MsgHup: StateLeader, with and without PreVote.
    for name, pv in (("TestSingleNodeCandidate", False), ("TestSingleNodePreCandidate", True)):
        out.append(scenario(name, "raft/raft_test.go:973-992", node([1], 1),
                            [action(HUP, state=LEADER)], pre_vote=pv))

    # testCampaignWhileLeader (raft_test.go:3337-3364): one peer; MsgHup makes
    # it leader, a second MsgHup leaves it leader at the same term.
    for name, pv in (("TestCampaignWhileLeader", False), ("TestPreCampaignWhileLeader", True)):
        out.append(scenario(name, "raft/raft_test.go:3337-3364", node([1], 1),
                            [action(HUP, state=LEADER, term=1),
                             action(HUP, state=LEADER, term=1, ignored=True)], pre_vote=pv))

    # TestLearnerCampaign (raft_test.go:4051-4081): voters {1}, learner 2.
    # MsgHup at the learner 2: still follower.  MsgHup at 1: leader, lead 1
    # (its own vote is the quorum).  MsgTimeoutNow at 2, by then a follower of
    # 1 at term 1 holding the empty entry: ignored.
    out.append(scenario("TestLearnerCampaign/n2-hup", "raft/raft_test.go:4051-4064",
                        node([1, 2], 2, voters=[1]), [action(HUP, state=FOLLOWER, ignored=True)]))
    out.append(scenario("TestLearnerCampaign/n1-hup", "raft/raft_test.go:4066-4069",
                        node([1, 2], 1, voters=[1]), [action(HUP, state=LEADER, lead=1)]))
    out.append(scenario("TestLearnerCampaign/n2-timeout-now", "raft/raft_test.go:4071-4081",
                        node([1, 2], 2, voters=[1], term=1, lead=1, last_index=1, last_term=1),
                        [action(TRANSFER, state=FOLLOWER, ignored=True)]))

    # TestPromotable (raft_test.go:3296-3313): node 1 with peers {1}, {1 2 3},
    # {}, {2 3}: promotable() true, true, false, false — a MsgHup campaigns or
    # is ignored accordingly (raft.go:766-769).
    for i, (peers, wp) in enumerate([([1], True), ([1, 2, 3], True), ([], False), ([2, 3], False)]):
        out.append(scenario(f"TestPromotable#{i}", "raft/raft_test.go:3296-3313", node(peers, 1),
                            [action(HUP, ignored=not wp)]))

    # testConfChangeCheckBeforeCampaign (raft_test.go:4227-4315), both entry
    # types (the engine sees neither: the host's look at the unapplied
    # entries is QB_CAMP_PENDING_CONF).  Node 2 follows 1 at term 1 with the
    # empty entry and the conf change in its log, committed and not applied:
    # its election timeout leaves it follower, and so does the MsgTimeoutNow
    # of a transfer.  After it applied them, the next MsgTimeoutNow makes it
    # campaign and the vote of 1 makes it leader.  Node 1, then follower of 2
    # at term 2 with everything applied, campaigns at its timeout:
    # StateCandidate.
    for name in ("TestConfChangeCheckBeforeCampaign", "TestConfChangeV2CheckBeforeCampaign"):
        n2 = node([1, 2, 3], 2, term=1, vote=1, lead=1, last_index=2, last_term=1, committed=2)
        out.append(scenario(f"{name}/n2", "raft/raft_test.go:4227-4304", n2,
                            [action(HUP, True, state=FOLLOWER, ignored=True),
                             action(TRANSFER, True, state=FOLLOWER, ignored=True),
                             action(TRANSFER, state=CANDIDATE), vote_resp(1)], state=LEADER))
        n1 = node([1, 2, 3], 1, term=2, vote=2, lead=2, last_index=3, last_term=2, committed=3)
        out.append(scenario(f"{name}/n1", "raft/raft_test.go:4306-4314", n1,
                            [action(HUP, state=CANDIDATE)]))

    # TestLeaderTransferToUpToDateNode (raft_test.go:3435-3456): three peers, 1
    # leader at term 1 with its empty entry everywhere.  MsgTransferLeader:
    # node 2 gets MsgTimeoutNow and runs hup(campaignTransfer) — candidate at
    # term 2, MsgVote to 1 and 3 carrying the "CampaignTransfer" context
    # (raft.go:829-833) — and with the vote of 1 it leads
    # (checkLeaderTransferState: the old leader follows 2).
    nd = node([1, 2, 3], 2, term=1, vote=1, lead=1, last_index=1, last_term=1, committed=1)
    out.append(scenario("TestLeaderTransferToUpToDateNode/n2", "raft/raft_test.go:3435-3456", nd,
                        [action(TRANSFER, state=CANDIDATE, term=2, self_vote=True,
                                reqs=votes_to([1, 3], 2, 1, 1, True)), vote_resp(1)],
                        state=LEADER, lead=2, term=2))

    # TestTransferNonMember (raft_test.go:3814-3824): node 1 is not among the
    # peers 2 3 4; MsgTimeoutNow and two MsgVoteResp leave it follower.
    out.append(scenario("TestTransferNonMember", "raft/raft_test.go:3814-3824", node([2, 3, 4], 1),
                        [action(TRANSFER, state=FOLLOWER, ignored=True), vote_resp(2), vote_resp(3)],
                        state=FOLLOWER))
    return out


def main():
    doc = {"comment": "transcribed by tests/golden/make_campaign_golden.py; data only",
           "scenarios": scenarios()}
    with open(os.path.join(HERE, "campaign_tables.json"), "w", encoding="utf-8") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
