#!/usr/bin/env python3
"""Writes tests/golden/propose_tables.json: the reference's own tests of the
proposal path transcribed as data (paths relative to the reference's raft/).

Each scenario is one node as its test leaves it right before the proposals
(``node``), the two Config knobs the path reads (``config``) and ``steps``:

  {"op": "leader_entry"}                    becomeLeader's empty entry
  {"op": "propose", "n": k, "payload": b,   Step(MsgProp) with k entries of b
   "cc": {"at": i, "payload": b, "leave_joint": bool}}     payload bytes in all
  {"op": "set", ...}                        what the test does to the node by
                                            hand between two Steps
  "repeat": r                               the step r times, the expectation
                                            holding after each

``expect`` holds what the test asserts (or, for a network test, what its
expected log implies at this node): dropped / forward / appended / cc_refused,
n_msgs, msgs ([type, to id, index, log_term, commit, entries]), last_index,
last_term, committed, pending_conf_index, uncommitted_size, log ([term, index]
of every entry behind first_index - 1) and progress per id.

Node ids are the test's; a slot is an id's rank.  State: 0 follower,
1 candidate, 2 leader, 3 pre-candidate.  Progress state: 0 probe, 1 replicate,
2 snapshot.  PayloadSize is len(Data) (util.go:216-218).
"""
import json
import os

APP = 3
NOLIMIT = 1 << 62        # entries per MsgApp under MaxSizePerMsg = noLimit


def pr(match, next_, state=0, **kw):
    d = {"match": match, "next": next_, "state": state, "recent_active": False, "probe_sent": False}
    d.update(kw)
    return d


def node(ids, self_, progress, *, terms, term=1, state=2, lead=None, first=1, committed=0,
         voters=None, voters_out=(), cap=256, **kw):
    d = {"ids": ids, "voters": list(voters if voters is not None else ids),
         "voters_out": list(voters_out), "self": self_, "state": state, "term": term,
         "lead": self_ if lead is None else lead, "first": first, "terms": terms,
         "committed": committed, "applied": 0, "pending_conf_index": 0, "uncommitted_size": 0,
         "inflight_cap": cap, "max_ents": NOLIMIT, "transferee": 0,
         "progress": {str(i): p for i, p in zip(ids, progress)}}
    d.update(kw)
    return d


def fresh_leader(ids, last=0, terms=None):
    """newTestRaft; becomeCandidate; becomeLeader, up to the empty entry:
    reset left every peer probing at next = last + 1, the own Progress
    replicates and holds MaybeUpdate(last + 1) (raft.go:724-745, 638)."""
    prs = [pr(last + 1, last + 2, 1) if i == 1 else pr(0, last + 1) for i in ids]
    return node(ids, 1, prs, terms=terms or [0] * (last + 1))


def prop(n=1, payload=0, expect=None, repeat=None, cc=None):
    d = {"op": "propose", "n": n, "payload": payload, "expect": expect or {}}
    if repeat:
        d["repeat"] = repeat
    if cc:
        d["cc"] = cc
    return d


LE = {"op": "leader_entry", "expect": {"appended": True}}
CC0 = {"at": 0, "payload": 0, "leave_joint": False}
OK = {"appended": True, "dropped": False}


def acked_leader(ids, quiet=()):
    """A network's node 1 after MsgHup and the election's traffic: the empty
    entry at index 1 is committed by the peers that answer (Replicate, match
    1); a nopStepper peer (``quiet``) was probed once and never answered."""
    prs = [pr(1, 2, 1, recent_active=(i != 1)) if i not in quiet else pr(0, 1, 0, probe_sent=True)
           for i in ids]
    n_ack = len(ids) - len(quiet)
    return node(ids, 1, prs, terms=[0, 1], committed=1 if n_ack > len(ids) // 2 else 0)


SCENARIOS = []


def add(name, source, node_, steps, **config):
    cfg = {"max_uncommitted_size": 0, "disable_proposal_forwarding": False}
    cfg.update(config)
    SCENARIOS.append({"name": name, "source": source, "node": node_, "config": cfg, "steps": steps})


# --- raft_test.go:3102-3164 ---------------------------------------------------
add("TestStepConfig", "raft_test.go:3102-3115", fresh_leader([1, 2]),
    [LE, prop(1, 0, dict(OK, last_index=2, pending_conf_index=2), cc=CC0)])
add("TestStepIgnoreConfig", "raft_test.go:3120-3140", fresh_leader([1, 2]),
    [LE, prop(1, 0, dict(OK, last_index=2, pending_conf_index=2), cc=CC0),
     prop(1, 0, dict(OK, cc_refused=True, last_index=3, last_term=1, pending_conf_index=2,
                     log=[[1, 1], [1, 2], [1, 3]]), cc=CC0)])
add("TestNewLeaderPendingConfig/0", "raft_test.go:3144-3164", fresh_leader([1, 2]),
    [dict(LE, expect={"appended": True, "pending_conf_index": 0, "last_index": 1})])
add("TestNewLeaderPendingConfig/1", "raft_test.go:3144-3164", fresh_leader([1, 2], last=1),
    [dict(LE, expect={"appended": True, "pending_conf_index": 1, "last_index": 2})])

# --- raft_test.go:3637-3660 ---------------------------------------------------
n = acked_leader([1, 2, 3])
n["transferee"] = 3
add("TestLeaderTransferIgnoreProposal", "raft_test.go:3637-3660", n,
    [prop(1, 0, {"dropped": True, "appended": False, "last_index": 1, "n_msgs": 0,
                 "progress": {"1": {"match": 1}}})])

# --- raft_test.go:705-723 -----------------------------------------------------
n = node([1], 1, [pr(1, 2, 1)], terms=[0], committed=1)   # campaign committed the entry to come
add("TestSingleNodeCommit", "raft_test.go:705-723", n,
    [LE, prop(1, 9, dict(OK, committed=2, n_msgs=0)), prop(1, 9, dict(OK, committed=3, n_msgs=0))])

# --- raft_test.go:1030-1087 (node 1's side of each network) --------------------
data = 8   # len("somedata")
add("TestProposal/0", "raft_test.go:1035", acked_leader([1, 2, 3]),
    [prop(1, data, dict(OK, log=[[1, 1], [1, 2]], msgs=[[APP, 2, 1, 1, 1, 1], [APP, 3, 1, 1, 1, 1]]))])
add("TestProposal/1", "raft_test.go:1036", acked_leader([1, 2, 3], quiet=(3,)),
    [prop(1, data, dict(OK, log=[[1, 1], [1, 2]], msgs=[[APP, 2, 1, 1, 1, 1]]))])
for j, ids in ((2, [1, 2, 3]), (3, [1, 2, 3, 4])):
    # no quorum answers: node 1 is still a candidate when the proposal arrives
    prs = [pr(0, 1) for _ in ids]
    prs[0] = pr(0, 1)
    add(f"TestProposal/{j}", f"raft_test.go:{1035 + j}",
        node(ids, 1, prs, terms=[0], state=1, lead=0),
        [prop(1, data, {"dropped": True, "appended": False, "last_index": 0, "n_msgs": 0})])
add("TestProposal/4", "raft_test.go:1039", acked_leader([1, 2, 3, 4, 5], quiet=(2, 3)),
    [prop(1, data, dict(OK, log=[[1, 1], [1, 2]], msgs=[[APP, 4, 1, 1, 1, 1], [APP, 5, 1, 1, 1, 1]]))])

# --- raft_test.go:1089-1125 ---------------------------------------------------
for j, quiet in ((0, ()), (1, (3,))):
    follower = node([1, 2, 3], 2, [pr(0, 1), pr(0, 1), pr(0, 1)], terms=[0, 1], state=0, lead=1,
                    committed=1)
    add(f"TestProposalByProxy/{j}/follower", "raft_test.go:1101", follower,
        [prop(1, data, {"forward": True, "appended": False, "dropped": False, "last_index": 1})])
    add(f"TestProposalByProxy/{j}/leader", "raft_test.go:1101-1108", acked_leader([1, 2, 3], quiet),
        [prop(1, data, dict(OK, log=[[1, 1], [1, 2]], last_term=1))])

# --- raft_test.go:179-270 -----------------------------------------------------
E, MAXE = 8, 1024   # len("testdata"), maxEntries
n = node([1, 2, 3], 1, [pr(1, 2, 1), pr(0, 1, 1), pr(0, 1, 1)], terms=[0, 1], cap=2 * 1024)
add("TestUncommittedEntryLimit", "raft_test.go:179-270", n,
    [prop(1, E, dict(OK, n_msgs=2), repeat=MAXE),
     prop(1, E, {"dropped": True, "appended": False, "uncommitted_size": MAXE * E, "n_msgs": 0}),
     {"op": "set", "uncommitted_size": 0},                       # reduceUncommittedSize(propEnts)
     prop(2 * MAXE, 2 * MAXE * E, dict(OK, n_msgs=2, uncommitted_size=2 * MAXE * E)),
     prop(1, E, {"dropped": True, "appended": False, "n_msgs": 0}),
     prop(1, 0, dict(OK, n_msgs=2, uncommitted_size=2 * MAXE * E,
                     last_index=1 + MAXE + 2 * MAXE + 1))],
    max_uncommitted_size=MAXE * E)

# --- raft_paper_test.go:397-427 -------------------------------------------------
add("TestLeaderStartReplication", "raft_paper_test.go:397-427", acked_leader([1, 2, 3]),
    [prop(1, 9, dict(OK, last_index=2, committed=1,
                     msgs=[[APP, 2, 1, 1, 1, 1], [APP, 3, 1, 1, 1, 1]]))])

# --- raft_flow_control_test.go:27-57 --------------------------------------------
n = node([1, 2], 1, [pr(1, 2, 1), pr(0, 1, 1)], terms=[0, 1], cap=256)
add("TestMsgAppFlowControlFull", "raft_flow_control_test.go:27-57", n,
    [prop(1, 8, dict(OK, n_msgs=1), repeat=256),
     {"op": "check", "expect": {"progress": {"2": {"inflights_full": True}}}},
     prop(1, 8, dict(OK, n_msgs=0), repeat=10)])

# --- raft_test.go:2613-2712: mustAppendEntry + sendAppend(2) on two nodes is a
# proposal's appendEntry + bcastAppend ---------------------------------------------
n = node([1, 2], 1, [pr(1, 2, 1), pr(0, 1, 0)], terms=[0, 1])
add("TestSendAppendForProgressProbe", "raft_test.go:2613-2664", n,
    [prop(1, 8, dict(OK, n_msgs=1, msgs=[[APP, 2, 0, 0, 0, 2]],
                     progress={"2": {"probe_sent": True}})),
     prop(1, 8, dict(OK, n_msgs=0, progress={"2": {"probe_sent": True}}), repeat=10),
     prop(1, 8, dict(OK, n_msgs=0, progress={"2": {"probe_sent": True}}), repeat=10),
     prop(1, 8, dict(OK, n_msgs=0, progress={"2": {"probe_sent": True}}), repeat=10)])
n = node([1, 2], 1, [pr(1, 2, 1), pr(0, 1, 1)], terms=[0, 1])
add("TestSendAppendForProgressReplicate", "raft_test.go:2680-2695", n,
    [prop(1, 8, dict(OK, n_msgs=1), repeat=10)])
n = node([1, 2], 1, [pr(1, 2, 1), pr(0, 1, 2, pending_snapshot=10)], terms=[0, 1])
add("TestSendAppendForProgressSnapshot", "raft_test.go:2697-2712", n,
    [prop(1, 8, dict(OK, n_msgs=0), repeat=10)])

# --- node_test.go:217-260 ---------------------------------------------------------
for name, disable, exp in (("r2", False, {"forward": True, "dropped": False}),
                           ("r3", True, {"forward": False, "dropped": True})):
    f = node([1, 2, 3], 2 if name == "r2" else 3, [pr(0, 2), pr(0, 2), pr(0, 2)], terms=[0, 1],
             state=0, lead=1)
    add(f"TestDisableProposalForwarding/{name}", "node_test.go:217-260", f,
        [prop(1, 8, dict(exp, appended=False, n_msgs=0))], disable_proposal_forwarding=disable)

# --- testdata/probe_and_replicate.txt: each leader's tenure while the Figure 7
# logs are built (lines 41-259), checked against the raft-log dumps (269-352) ------
IDS = [1, 2, 3, 4, 5, 6, 7]


def tenure(who, term, log, props, want):
    """``log``: the terms of indexes 10.. at election (index 10 is the
    snapshot, term 1); ``props``: proposals behind the empty entry."""
    last = 10 + len(log) - 1
    prs = [pr(last + 1, last + 2, 1) if i == who else pr(0, last + 1) for i in IDS]
    n_ = node(IDS, who, prs, terms=log, term=term, first=11, committed=10)
    add(f"probe_and_replicate/n{who}_term{term}", "testdata/probe_and_replicate.txt", n_,
        [LE] + [prop(1, 9, dict(OK))] * (props - 1) +
        [prop(1, 9, dict(OK, log=[[t, 11 + k] for k, t in enumerate(want)]))])


tenure(1, 1, [1], 2, [1, 1, 1])
tenure(2, 2, [1, 1, 1, 1], 2, [1, 1, 1, 2, 2, 2])
tenure(7, 3, [1, 1, 1, 1, 2, 2, 2], 4, [1, 1, 1, 2, 2, 2, 3, 3, 3, 3, 3])
tenure(6, 4, [1, 1, 1, 1], 3, [1, 1, 1, 4, 4, 4, 4])
tenure(5, 5, [1, 1, 1, 1, 4, 4], 1, [1, 1, 1, 4, 4, 5, 5])
tenure(4, 6, [1, 1, 1, 1, 4, 4, 5, 5], 3, [1, 1, 1, 4, 4, 5, 5, 6, 6, 6, 6])
tenure(5, 7, [1, 1, 1, 1, 4, 4, 5, 5, 6], 3, [1, 1, 1, 4, 4, 5, 5, 6, 7, 7, 7, 7])

if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "propose_tables.json")
    with open(out, "w", encoding="utf-8") as f:
        json.dump({"scenarios": SCENARIOS}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{out}: {len(SCENARIOS)} scenarios")
