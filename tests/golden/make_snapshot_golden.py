#!/usr/bin/env python3
"""Write tests/golden/snapshot_tables.json: the reference's own tests of the
MsgSnap path at a follower — raft.restore, Step(MsgSnap), raftLog.restore,
unstable.restore and term() over an unstable snapshot — transcribed as data.

Everything below is inputs and expected outputs read off the reference's test
files (paths relative to the reference's raft/).  A node is the state the cited
test has built before the checked call, restated as the fields the path reads:

  id       the node's raft ID
  first    raftLog.firstIndex()
  terms    the terms of [first - 1, lastIndex]: the dummy entry (the snapshot's
           term, 0 for an empty storage) and one per entry
  offset   unstable.offset
  snap     [index, term] of unstable.snapshot or null
  committed, term, vote, lead, state

newTestRaft(id, 10, 1, storage) over an empty storage is a follower at term 0
with an empty log.  A step is either "restore" (raft.restore called directly:
"ok" is its return value) or "step" (raft.Step of a MsgSnap: "resp" is the
MsgAppResp's [Term, Index]).  "want" lists the fields the test checks, by the
names above plus last_index, term_at ([index, term] pairs of raftLog.term),
entries (len of the log's entries) and promotable (the tests' "It should not
campaign before actually applying data": a tick may not campaign).  The config
the tests check after a restore (Voters, Learners, IsLearner) is
confchange.Restore's and is pinned by confchange_datadriven.json.  Nothing is
executed against the reference at test time; the JSON is committed.
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))

FOLLOWER = 0


def node(id_, *, first=1, terms=(0,), offset=1, snap=None, committed=0, term=0, vote=0, lead=0,
         state=FOLLOWER):
    return {"id": id_, "first": first, "terms": list(terms), "offset": offset, "snap": snap,
            "committed": committed, "term": term, "vote": vote, "lead": lead, "state": state}


def cs(voters=(), learners=(), voters_outgoing=(), learners_next=()):
    return {"voters": list(voters), "learners": list(learners),
            "voters_outgoing": list(voters_outgoing), "learners_next": list(learners_next)}


def snap(index, term, conf):
    return {"index": index, "term": term, "cs": conf}


RESTORED = {"last_index": 11, "term_at": [[11, 11]], "committed": 11}


def restore_tables():
    out = []
    s = snap(11, 11, cs(voters=[1, 2, 3]))
    # raft_test.go:2737-2773: restore succeeds, the second call returns false,
    # and randomizedElectionTimeout ticks leave the node a follower.
    out.append({"name": "TestRestore", "src": "raft_test.go:2737-2773", "node": node(1), "steps": [
        {"op": "restore", "snap": s, "ok": True, "want": RESTORED},
        {"op": "restore", "snap": s, "ok": False, "want": dict(RESTORED, promotable=False, state=FOLLOWER)}]})
    s = snap(11, 11, cs(voters=[1, 2], learners=[3]))
    out.append({"name": "TestRestoreWithLearner", "src": "raft_test.go:2776-2819", "node": node(3),
                "steps": [{"op": "restore", "snap": s, "ok": True, "want": RESTORED},
                          {"op": "restore", "snap": s, "ok": False, "want": RESTORED}]})
    s = snap(11, 11, cs(voters=[2, 3, 4], voters_outgoing=[1, 2, 3]))
    out.append({"name": "TestRestoreWithVotersOutgoing", "src": "raft_test.go:2822-2858",
                "node": node(1), "steps": [
                    {"op": "restore", "snap": s, "ok": True, "want": RESTORED},
                    {"op": "restore", "snap": s, "ok": False,
                     "want": dict(RESTORED, promotable=False, state=FOLLOWER)}]})
    s = snap(11, 11, cs(voters=[1, 2], learners=[3]))
    out.append({"name": "TestRestoreVoterToLearner", "src": "raft_test.go:2868-2886",
                "node": node(3), "steps": [{"op": "restore", "snap": s, "ok": True, "want": {}}]})
    s = snap(11, 11, cs(voters=[1, 2, 3]))
    out.append({"name": "TestRestoreLearnerPromotion", "src": "raft_test.go:2890-2913",
                "node": node(3), "steps": [{"op": "restore", "snap": s, "ok": True, "want": {}}]})
    # raft_test.go:2952-2984: entries 1..3 of term 1 appended (unstable),
    # commitTo(1).  A snapshot at the commit index is ignored; one at commit +
    # 1 whose term matches fast-forwards the commit.
    ign = node(1, terms=[0, 1, 1, 1], offset=1, committed=1)
    out.append({"name": "TestRestoreIgnoreSnapshot", "src": "raft_test.go:2952-2984", "node": ign,
                "steps": [
                    {"op": "restore", "snap": snap(1, 1, cs(voters=[1, 2])), "ok": False,
                     "want": {"committed": 1}},
                    {"op": "restore", "snap": snap(2, 1, cs(voters=[1, 2])), "ok": False,
                     "want": {"committed": 2, "last_index": 3}}]})
    return out


def step_tables():
    out = []
    # raft_test.go:3045-3063: node 2 at term 0 steps a MsgSnap{From: 1, Term: 2}.
    out.append({"name": "TestRestoreFromSnapMsg", "src": "raft_test.go:3045-3063", "node": node(2),
                "steps": [{"op": "step", "from": 1, "term": 2,
                           "snap": snap(11, 11, cs(voters=[1, 2])), "want": {"lead": 1}}]})
    # testdata/snapshot_succeed_via_app_resp.txt:48-119, the follower's half:
    # node 3 has no state at all; the heartbeat made it a follower of 1 at
    # term 1 (lines 71-82); then "1->3 MsgSnap Term:1 ... Snapshot: Index:11
    # Term:1 ConfState:Voters:[1 2 3]" is answered with "3->1 MsgAppResp
    # Term:1 Log:0/11" and the Ready holds "HardState Term:1 Commit:11" and
    # the snapshot (lines 106-119).
    out.append({"name": "snapshot_succeed_via_app_resp (follower)",
                "src": "testdata/snapshot_succeed_via_app_resp.txt:48-119",
                "node": node(3, term=1, lead=1),
                "steps": [{"op": "step", "from": 1, "term": 1,
                           "snap": snap(11, 1, cs(voters=[1, 2, 3])), "resp": [1, 11],
                           "want": {"term": 1, "vote": 0, "committed": 11, "last_index": 11,
                                    "term_at": [[11, 1]], "snap": [11, 1], "lead": 1}}]})
    return out


def log_tables():
    out = []
    # log_test.go:580-603: the log over a storage that holds the snapshot
    # (1000, 1000) — what raftLog.restore leaves of an empty log.
    out.append({"name": "TestLogRestore", "src": "log_test.go:580-603", "node": node(1),
                "restore": [1000, 1000],
                "want": {"entries": 0, "first": 1001, "committed": 1000, "offset": 1001,
                         "term_at": [[1000, 1000]]}})
    # log_unstable_test.go:198-217: unstable{entries: [(5, term 1)], offset 5,
    # snapshot (4, 1)}.restore((6, 2)).
    out.append({"name": "TestUnstableRestore", "src": "log_unstable_test.go:198-217",
                "node": node(1, first=5, terms=[1, 1], offset=5, snap=[4, 1], committed=4),
                "restore": [6, 2], "want": {"offset": 7, "entries": 0, "snap": [6, 2]}})
    # log_test.go:717-745: a storage snapshot (100, 1), then restore((105, 1)).
    out.append({"name": "TestTermWithUnstableSnapshot", "src": "log_test.go:717-745",
                "node": node(1, first=101, terms=[1], offset=101, committed=100),
                "restore": [105, 1],
                "want": {"term_at": [[100, 0], [101, 0], [104, 0], [105, 1]]}})
    return out


def main():
    doc = {"restore": restore_tables(), "step": step_tables(), "log": log_tables()}
    with open(os.path.join(HERE, "snapshot_tables.json"), "w", encoding="utf-8") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
