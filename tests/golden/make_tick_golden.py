#!/usr/bin/env python3
"""Write tests/golden/tick_tables.json: the reference's own tests of raft.tick()
on a leader — heartbeat broadcast, CheckQuorum, leader-transfer timeout —
transcribed as data.

Everything below is inputs and expected outputs read off the reference's test
files (paths relative to the reference's raft/); the setup each scenario
starts from is the state the cited test builds before its first tick, restated
as the fields the tick reads (becomeLeader -> reset: every Progress with
Match 0 and RecentActive false, the leader's Match = lastIndex after it
appends its empty entry; both elapsed counters 0; raft.go:590-620, 724-760).
A test that Steps MsgBeat directly is one tick at heartbeatTimeout 1, which
is what the tick does with it (raft.go:678-683).

Slot s is voter ID s+1 (IDs 1..n).  A message is [type, to (slot), index,
log_term, commit, aux (context)] (tests/leader_scenarios.py MSG_FIELDS).
Nothing here is executed against the reference at test time; the JSON is
committed.
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))

FOLLOWER, CANDIDATE, LEADER = 0, 1, 2
PROMOTABLE = 0x80
HEARTBEAT = 8  # pb.MsgHeartbeat


def node(n, role, committed, match, *, active=None, et=10, ht=1, cq=False, transferee=255,
         rand_timeout=None, leader=0):
    """newTestRaft(1, et, ht, withPeers(1..n)): node 1 is slot 0."""
    active = active or [False] * n
    return {"slots": n, "mask_in": (1 << n) - 1, "mask_out": 0, "leader": leader,
            "role": role | PROMOTABLE, "committed": committed, "transferee": transferee,
            "progress": [{"match": m, "recent_active": a} for m, a in zip(match, active)],
            "readq_ctx": [], "election_timeout": et, "heartbeat_timeout": ht,
            "check_quorum": cq, "election_elapsed": 0, "heartbeat_elapsed": 0,
            # randomizedElectionTimeout is et + rand[0, et): the tests below never reach it
            "rand_timeout": et if rand_timeout is None else rand_timeout, "ops": []}


def tick(**expect):
    return {"op": "tick", "expect": expect}


def hb_resp(slot):
    """Step(MsgHeartbeatResp from slot) as far as the tick sees it:
    pr.RecentActive = true (raft.go:1284-1285)."""
    return {"op": "hb_resp", "slot": slot}


def hb(to, commit):
    return [HEARTBEAT, to, 0, 0, commit, 0]


def scenarios():
    out = []

    # TestBcastBeat (raft_test.go:2484-2540).  Snapshot at 1000; becomeLeader
    # appends 1001, then ten entries: lastIndex 1011, committed 1000 (nothing
    # acked).  Progress[2] = slow follower Match 5, Progress[3] Match 1011.
    # wantCommitMap: 2 -> min(1000, 5), 3 -> min(1000, 1011); Index and
    # LogTerm 0, two messages.
    sc = node(3, LEADER, 1000, [1011, 5, 1011])
    sc.update(name="TestBcastBeat", cite="raft/raft_test.go:2484-2540")
    sc["ops"] = [tick(n_msgs=2, msgs_exact=[hb(1, 5), hb(2, 1000)], role=LEADER)]
    out.append(sc)

    # TestRecvMsgBeat (raft_test.go:2543-2577): a leader answers MsgBeat with
    # two MsgHeartbeat; candidate and follower ignore it (their tick is
    # tickElection and sends nothing).  Log {1,t0} {2,t1}, nothing committed.
    for i, (state, wmsg) in enumerate([(LEADER, 2), (CANDIDATE, 0), (FOLLOWER, 0)]):
        sc = node(3, state, 0, [0, 0, 0])
        sc.update(name=f"TestRecvMsgBeat#{i}", cite="raft/raft_test.go:2543-2577")
        sc["ops"] = [tick(n_msgs=wmsg, all_msgs={"type": HEARTBEAT}, role=state)]
        out.append(sc)

    # TestLeaderStepdownWhenQuorumActive (raft_test.go:1748-1764): three
    # peers, electionTimeout 5, checkQuorum; electionTimeout+1 rounds of a
    # heartbeat response from 2 followed by a tick: still leader.
    sc = node(3, LEADER, 0, [1, 0, 0], et=5, cq=True)
    sc.update(name="TestLeaderStepdownWhenQuorumActive", cite="raft/raft_test.go:1748-1764")
    for i in range(5 + 1):
        sc["ops"] += [hb_resp(1), tick(role=LEADER, n_msgs=2)]
    out.append(sc)

    # TestLeaderStepdownWhenQuorumLost (raft_test.go:1766-1781): the same
    # without responses: follower after electionTimeout+1 ticks (the fifth
    # tick's CheckQuorum steps down and sends nothing).
    sc = node(3, LEADER, 0, [1, 0, 0], et=5, cq=True)
    sc.update(name="TestLeaderStepdownWhenQuorumLost", cite="raft/raft_test.go:1766-1781")
    sc["ops"] = [tick(role=LEADER, n_msgs=2) for _ in range(4)]
    sc["ops"] += [tick(role=FOLLOWER, n_msgs=0), tick(role=FOLLOWER, n_msgs=0)]
    out.append(sc)

    # TestLeaderTransferTimeout (raft_test.go:3610-3634): a network of three
    # (electionTimeout 10, heartbeatTimeout 1), 1 elected: entry 1 committed
    # everywhere, 2 and 3 RecentActive from their responses.  3 is isolated
    # and MsgTransferLeader to it sets leadTransferee = 3 and electionElapsed
    # = 0 (raft.go:1361-1363).  heartbeatTimeout ticks later the transfer is
    # still pending; electionTimeout - heartbeatTimeout further ticks abort
    # it, and the node is still leader (checkLeaderTransferState).
    sc = node(3, LEADER, 1, [1, 1, 1], active=[False, True, True], transferee=2)
    sc.update(name="TestLeaderTransferTimeout", cite="raft/raft_test.go:3610-3634")
    sc["ops"] = [tick(role=LEADER, transferee=2)]
    sc["ops"] += [tick(role=LEADER, transferee=2) for _ in range(8)]
    sc["ops"] += [tick(role=LEADER, transferee=255)]
    out.append(sc)

    # TestLeaderBcastBeat (raft_paper_test.go:109-134): heartbeat interval 1,
    # ten entries appended after becomeLeader (lastIndex 11, nothing
    # committed); one tick sends {To: 2} and {To: 3}, MsgHeartbeat with Index
    # 0, LogTerm 0, Commit 0 and no context.
    sc = node(3, LEADER, 0, [11, 0, 0])
    sc.update(name="TestLeaderBcastBeat", cite="raft/raft_paper_test.go:109-134")
    sc["ops"] = [tick(n_msgs=2, msgs_exact=[hb(1, 0), hb(2, 0)], role=LEADER)]
    out.append(sc)
    return out


def main():
    doc = {"comment": "transcribed by tests/golden/make_tick_golden.py; data only",
           "scenarios": scenarios()}
    with open(os.path.join(HERE, "tick_tables.json"), "w", encoding="utf-8") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
