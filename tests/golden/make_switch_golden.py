"""Writes tests/golden/switch_tables.json: the reference's switchToConfig cases
as data.  Each case is one raft node by ID just before ``switched to
configuration`` (the old and new member lists, the log's terms, the Progress
map as confchange.Changer left it, the transferee) and what the reference
asserts or prints right after: the flags, the committed index, the messages
of the next Ready ([type, to, index, log_term, commit, entries]) and Progress
fields.  Transcribed by hand from raft/raft_test.go and raft/testdata/ of the
reference; run from the repository root to regenerate the file."""
import json
import os

LEADER, FOLLOWER = 2, 0
PROBE, REPLICATE = 0, 1
APP = 3


def pr(match, next, state=PROBE, **kw):
    return dict(match=match, next=next, state=state, **kw)


def case(name, source, old_ids, ids, new_voters, *, self_id=1, role=FOLLOWER, term=0, terms=(0,),
         first=1, committed=0, progress=None, transferee=0, voters_out=(), action=1, inflight_cap=2, **expect):
    return dict(inflight_cap=inflight_cap, name=name, source=source, old_ids=old_ids, ids=ids, voters=new_voters,
                voters_out=list(voters_out), self=self_id, role=role, term=term, terms=list(terms),
                first=first, committed=committed,
                progress={str(k): v for k, v in (progress or {}).items()}, transferee=transferee,
                action=action, expect=expect)


# newTestRaft(1, ..., withPeers(...)): a follower at term 0 over an empty log;
# every Progress is Next = 1 (newRaft's restore through confchange.Restore).
CASES = [
    case("TestAddNode", "raft_test.go:3167-3175", [1], [1, 2], [1, 2],
         progress={1: pr(0, 1), 2: pr(0, 0)},
         flags=["switched"], voters=[1, 2], learners=[], is_learner=False, msgs=[]),
    case("TestAddLearner/add_learner_2", "raft_test.go:3178-3192", [1], [1, 2], [1],
         progress={1: pr(0, 1), 2: pr(0, 0)},
         flags=["switched"], voters=[1], learners=[2], is_learner=False, msgs=[]),
    case("TestAddLearner/promote_2", "raft_test.go:3194-3198", [1, 2], [1, 2], [1, 2],
         progress={1: pr(0, 1), 2: pr(0, 0)},
         flags=["switched"], voters=[1, 2], learners=[], is_learner=False, msgs=[]),
    case("TestAddLearner/demote_self", "raft_test.go:3200-3207", [1, 2], [1, 2], [2],
         progress={1: pr(0, 1), 2: pr(0, 0)},
         flags=["switched"], voters=[2], learners=[1], is_learner=True, msgs=[]),
    case("TestAddLearner/promote_self", "raft_test.go:3209-3216", [1, 2], [1, 2], [1, 2],
         progress={1: pr(0, 1), 2: pr(0, 0)},
         flags=["switched"], voters=[1, 2], learners=[], is_learner=False, msgs=[]),
    case("TestRemoveNode", "raft_test.go:3255-3261", [1, 2], [1], [1],
         progress={1: pr(0, 1)},
         flags=["switched"], voters=[1], learners=[], is_learner=False, msgs=[]),
    case("TestRemoveLearner", "raft_test.go:3274-3285", [1, 2], [1], [1],
         progress={1: pr(0, 1)},
         flags=["switched"], voters=[1], learners=[], is_learner=False, msgs=[]),
    # leader at term 1: 1 the empty entry, 2 the conf change (acked by 2:
    # committed), 3 "hello".  Removing 2 lets 3 commit.
    case("TestCommitAfterRemoveNode", "raft_test.go:3370-3431", [1, 2], [1], [1],
         role=LEADER, term=1, terms=[0, 1, 1, 1], committed=2,
         progress={1: pr(3, 4, REPLICATE)},
         flags=["switched", "committed", "sent"], committed_after=3, msgs=[], voters=[1]),
    # node 1 leads 1, 2, 3 at term 1, everyone at index 1; a transfer to 3
    # is pending (MsgTimeoutNow was sent and dropped).
    case("TestLeaderTransferRemoveNode", "raft_test.go:3681-3698", [1, 2, 3], [1, 2], [1, 2],
         role=LEADER, term=1, terms=[0, 1], committed=1, transferee=3,
         progress={1: pr(1, 2, REPLICATE), 2: pr(1, 2, REPLICATE)},
         flags=["switched", "sent", "transfer_aborted"], transferee_after=0, committed_after=1,
         msgs=[]),
    case("TestLeaderTransferDemoteNode", "raft_test.go:3700-3728", [1, 2, 3], [1, 2, 3], [1, 2],
         role=LEADER, term=1, terms=[0, 1], committed=1, transferee=3,
         progress={1: pr(1, 2, REPLICATE), 2: pr(1, 2, REPLICATE), 3: pr(1, 2, REPLICATE)},
         flags=["switched", "sent", "transfer_aborted"], transferee_after=0, committed_after=1,
         learners=[3], msgs=[]),
    # a single-voter leader adds 2: no election, the leader stays leader and
    # probes the new member at once.
    case("TestAddNodeCheckQuorum", "raft_test.go:3221-3251", [1], [1, 2], [1, 2],
         role=LEADER, term=1, terms=[0, 1], committed=1,
         progress={1: pr(1, 2, REPLICATE), 2: pr(0, 1)},
         flags=["switched", "sent"], committed_after=1, role_after=LEADER,
         msgs=[[APP, 2, 0, 0, 1, 1]], progress_after={"2": {"probe_sent": True, "next": 1}}),
    # add-nodes ... index=2: the log starts behind a snapshot at 2 (term 1); 3
    # is the leader's empty entry, 4 the conf change, both committed by the
    # single voter.  initProgress gives 2 Next = LastIndex = 4.
    case("confchange_v1_add_single", "testdata/confchange_v1_add_single.txt:33-49", [1], [1, 2],
         [1, 2], role=LEADER, term=1, terms=[1, 1, 1], first=3, committed=4,
         progress={1: pr(4, 5, REPLICATE), 2: pr(0, 4)},
         flags=["switched", "sent"], committed_after=4, msgs=[[APP, 2, 3, 1, 4, 1]],
         progress_after={"2": {"probe_sent": True, "next": 4, "match": 0}}),
    # the leader removes itself: it stays leader of a group it is no member
    # of, sends nothing and commits nothing at the switch (2 has acked 6, 3
    # nothing yet).
    case("confchange_v1_remove_leader", "testdata/confchange_v1_remove_leader.txt:85-108",
         [1, 2, 3], [2, 3], [2, 3], role=LEADER, term=1, terms=[1, 1, 1, 1, 1], first=3,
         committed=5, progress={2: pr(6, 7, REPLICATE), 3: pr(2, 7, REPLICATE)},
         flags=["switched", "self_removed"], committed_after=5, msgs=[], own_present=False),
    # --- the joint-config traces.  Every one starts as confchange_v1_add_single
    # does: a snapshot at 2 (term 1), 3 the leader's empty entry, 4 the change.
    case("confchange_v2_add_single_auto", "testdata/confchange_v2_add_single_auto.txt:34-50",
         [1], [1, 2], [1, 2], role=LEADER, term=1, terms=[1, 1, 1], first=3, committed=4,
         progress={1: pr(4, 5, REPLICATE), 2: pr(0, 4)},
         flags=["switched", "sent"], committed_after=4, msgs=[[APP, 2, 3, 1, 4, 1]]),
    # (1 2)&&(1): the incoming half's quorum index is 0, so nothing commits
    # and the new member is probed.
    case("confchange_v2_add_single_explicit/enter", "testdata/confchange_v2_add_single_explicit.txt:34-50",
         [1], [1, 2], [1, 2], voters_out=[1], role=LEADER, term=1, terms=[1, 1, 1], first=3,
         committed=4, progress={1: pr(4, 5, REPLICATE), 2: pr(0, 4)},
         flags=["switched", "sent"], committed_after=4, msgs=[[APP, 2, 3, 1, 4, 1]],
         voters=[1, 2], progress_after={"2": {"probe_sent": True}}),
    # leaving it: 5 and 6 are committed, both members are caught up.
    case("confchange_v2_add_single_explicit/leave", "testdata/confchange_v2_add_single_explicit.txt:138-161",
         [1, 2], [1, 2], [1, 2], role=LEADER, term=1, terms=[1] * 5, first=3, committed=6,
         progress={1: pr(6, 7, REPLICATE), 2: pr(6, 7, REPLICATE)},
         flags=["switched", "sent"], committed_after=6, msgs=[]),
    case("confchange_v2_add_double_auto/enter", "testdata/confchange_v2_add_double_auto.txt:39-62",
         [1], [1, 2, 3], [1, 2, 3], voters_out=[1], role=LEADER, term=1, terms=[1, 1, 1], first=3,
         committed=4, progress={1: pr(4, 5, REPLICATE), 2: pr(0, 4), 3: pr(0, 4)},
         flags=["switched", "sent"], committed_after=4,
         msgs=[[APP, 2, 3, 1, 4, 1], [APP, 3, 3, 1, 4, 1]]),
    # 2 has acked 5; 3 has not answered its probe yet (ProbeSent: paused).
    case("confchange_v2_add_double_auto/leave", "testdata/confchange_v2_add_double_auto.txt:121-139",
         [1, 2, 3], [1, 2, 3], [1, 2, 3], role=LEADER, term=1, terms=[1] * 4, first=3, committed=5,
         progress={1: pr(5, 6, REPLICATE), 2: pr(5, 6, REPLICATE), 3: pr(0, 4, probe_sent=True)},
         flags=["switched", "sent"], committed_after=5, msgs=[]),
    # r2 r3: (1)&&(1 2 3).  2 and 3 have acked 6; 7 and 8 are in flight to
    # them.  The outgoing half holds the commit at 6.
    case("confchange_v2_add_double_auto/enter_removal", "testdata/confchange_v2_add_double_auto.txt:263-274",
         [1, 2, 3], [1, 2, 3], [1], voters_out=[1, 2, 3], role=LEADER, term=1, terms=[1] * 7,
         first=3, committed=6, inflight_cap=256,
         progress={1: pr(8, 9, REPLICATE), 2: pr(6, 9, REPLICATE, ring=[7, 8]),
                   3: pr(6, 9, REPLICATE, ring=[7, 8])},
         flags=["switched", "sent"], committed_after=6, msgs=[], voters=[1, 2, 3], learners=[]),
    case("confchange_v2_add_double_auto/leave_removal", "testdata/confchange_v2_add_double_auto.txt:370-383",
         [1, 2, 3], [1], [1], role=LEADER, term=1, terms=[1] * 8, first=3, committed=9,
         progress={1: pr(9, 10, REPLICATE)},
         flags=["switched", "sent"], committed_after=9, msgs=[], voters=[1]),
    case("confchange_v2_add_double_implicit/enter", "testdata/confchange_v2_add_double_implicit.txt:36-55",
         [1], [1, 2], [1, 2], voters_out=[1], role=LEADER, term=1, terms=[1, 1, 1], first=3,
         committed=4, progress={1: pr(4, 5, REPLICATE), 2: pr(0, 4)},
         flags=["switched", "sent"], committed_after=4, msgs=[[APP, 2, 3, 1, 4, 1]]),
    case("confchange_v2_add_double_implicit/leave", "testdata/confchange_v2_add_double_implicit.txt:106-124",
         [1, 2], [1, 2], [1, 2], role=LEADER, term=1, terms=[1] * 4, first=3, committed=5,
         progress={1: pr(5, 6, REPLICATE), 2: pr(5, 6, REPLICATE)},
         flags=["switched", "sent"], committed_after=5, msgs=[]),
    # r1 v4, explicit: (2 3 4)&&(1 2 3).  The leader stays a voter of the
    # outgoing half, so it goes on and probes 4.
    case("confchange_v2_replace_leader/enter", "testdata/confchange_v2_replace_leader.txt:82-98",
         [1, 2, 3], [1, 2, 3, 4], [2, 3, 4], voters_out=[1, 2, 3], role=LEADER, term=1,
         terms=[1, 1, 1], first=3, committed=4,
         progress={1: pr(4, 5, REPLICATE), 2: pr(4, 5, REPLICATE), 3: pr(4, 5, REPLICATE),
                   4: pr(0, 4)},
         flags=["switched", "sent"], committed_after=4, msgs=[[APP, 4, 3, 1, 4, 1]],
         is_learner=False, voters=[1, 2, 3, 4]),
    # 4 leads at term 2 behind its snapshot at 4 and leaves the joint config:
    # 1 goes, the own slot moves from 3 to 2.
    case("confchange_v2_replace_leader/leave_at_new_leader",
         "testdata/confchange_v2_replace_leader.txt:379-388",
         [1, 2, 3, 4], [2, 3, 4], [2, 3, 4], self_id=4, role=LEADER, term=2, terms=[1, 2, 2],
         first=5, committed=6,
         progress={2: pr(6, 7, REPLICATE), 3: pr(6, 7, REPLICATE), 4: pr(6, 7, REPLICATE)},
         flags=["switched", "sent"], committed_after=6, msgs=[], voters=[2, 3, 4]),
    # the old leader, a follower by now, applies the same entry and is gone.
    case("confchange_v2_replace_leader/leave_at_removed_follower",
         "testdata/confchange_v2_replace_leader.txt:395-402",
         [1, 2, 3, 4], [2, 3, 4], [2, 3, 4], self_id=1, role=FOLLOWER, term=2,
         terms=[1, 1, 1, 2, 2], first=3, committed=6,
         flags=["switched"], committed_after=6, msgs=[], own_present=False),
]

if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "switch_tables.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"cases": CASES}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(CASES)} cases")
