#!/usr/bin/env python3
"""Writes tests/golden/request_tables.json: the reference's own tests of the
MsgReadIndex and MsgTransferLeader paths transcribed as data (paths relative
to the reference's raft/).  Only the parts of a test that pass through
stepLeader's / stepFollower's two cases are here; what follows them (the
heartbeat acks, the MsgTimeoutNow's election) belongs to other calls.

Each scenario is one node as its test leaves it right before the requests
(``node``, the layout of make_propose_golden.py plus ``election_elapsed`` and,
per Progress, ``ring``: the Inflights' indexes, oldest first), the knobs the
paths read (``config``: read_only 0 safe / 1 lease, readq_cap, max_reads) and
``steps``:

  {"op": "read", "ctx": c, "from": id}       Step(MsgReadIndex); from 0 is
                                             From == None (a local request)
  {"op": "transfer", "from": id, "term": t}  Step(MsgTransferLeader); term 0
                                             is a local message
  {"op": "set", ...}                         what the test's network does to
                                             the node between two Steps

``expect`` holds what the test asserts or what its assertions imply at this
node.  read: status (read_state / resp / bcast / bcast_dup / postponed /
forward / dropped / ignored), index (the read index: answered at once, or
queued and answered by the later acks), heartbeats ([to id, commit]), queue
([ctx, index, [ack ids], from id]) and pending (pendingReadIndexMessages is
non-empty).  transfer: msg ([type, to id, index, log_term, commit, entries] or
null), transferee (0 none), started, aborted, forward, election_elapsed.

Node ids are the test's; a slot is an id's rank, an id outside ``ids`` is the
slot past them.  State: 0 follower, 1 candidate, 2 leader, 3 pre-candidate.
Progress state: 0 probe, 1 replicate, 2 snapshot.  A context is the test's
byte string as a big-endian integer (the engine's contexts are 8 bytes).
"""
import json
import os

APP, SNAP, TIMEOUT_NOW = 3, 7, 14
NOLIMIT = 1 << 62        # entries per MsgApp under MaxSizePerMsg = noLimit


def ctx(b):
    assert 0 < len(b) <= 8
    return int.from_bytes(b, "big")


def pr(match, next_, state=0, **kw):
    d = {"match": match, "next": next_, "state": state, "recent_active": False, "probe_sent": False,
         "ring": []}
    d.update(kw)
    return d


def node(ids, self_, progress, *, terms, term=1, state=2, lead=None, first=1, committed=0,
         voters=None, voters_out=(), cap=256, **kw):
    d = {"ids": ids, "voters": list(voters if voters is not None else ids),
         "voters_out": list(voters_out), "self": self_, "state": state, "term": term,
         "lead": self_ if lead is None else lead, "first": first, "terms": terms,
         "committed": committed, "applied": 0, "pending_conf_index": 0, "uncommitted_size": 0,
         "inflight_cap": cap, "max_ents": NOLIMIT, "transferee": 0, "election_elapsed": 0,
         "progress": {str(i): p for i, p in zip(ids, progress)}}
    d.update(kw)
    return d


def settled(ids, who, last, term=1, terms=None, voters=None, state=2, lead=None):
    """A network's node once every entry up to ``last`` is replicated and
    committed everywhere: every Progress replicates at match = last."""
    prs = [pr(last, last + 1, 1, recent_active=(i != who)) for i in ids]
    return node(ids, who, prs, terms=terms or [0] + [term] * last, term=term, committed=last,
                voters=voters, state=state, lead=who if lead is None else lead)


def follower(ids, who, lead, last, term=1, terms=None, voters=None):
    prs = [pr(0, 1) for _ in ids]
    return node(ids, who, prs, terms=terms or [0] + [term] * last, term=term, committed=last,
                voters=voters, state=0, lead=lead)


def read(c, frm, **expect):
    return {"op": "read", "ctx": c, "from": frm, "expect": expect}


def transfer(frm, term=0, **expect):
    return {"op": "transfer", "from": frm, "term": term, "expect": expect}


SCENARIOS = []


def add(name, source, node_, steps, **config):
    cfg = {"read_only": 0, "readq_cap": 4, "max_reads": 1}
    cfg.update(config)
    SCENARIOS.append({"name": name, "source": source, "node": node_, "config": cfg, "steps": steps})


# --- raft_test.go:2177-2337: ten proposals, then a read at a, b, c in turn.  A
# read at b or c is forwarded (From stays the follower's id) and queued at a ----
IDS3 = [1, 2, 3]
for name, src, ro in (("TestReadOnlyOptionSafe", "raft_test.go:2177-2229", 0),
                      ("TestReadOnlyOptionLease", "raft_test.go:2282-2337", 1)):
    for i, (who, wri) in enumerate(((1, 11), (2, 21), (3, 31), (1, 41), (2, 51), (3, 61))):
        c = ctx(b"ctx%d" % (i + 1))
        if who != 1:
            add(f"{name}/{i}/follower", src, follower(IDS3, who, 1, wri),
                [read(c, who, status="forward")], read_only=ro)
        if ro == 0:
            exp = dict(status="bcast", index=wri, heartbeats=[[2, wri], [3, wri]],
                       queue=[[c, wri, [1], who]])
        else:
            exp = dict(status="read_state" if who == 1 else "resp", index=wri, queue=[])
        add(f"{name}/{i}/leader", src, settled(IDS3, 1, wri), [read(c, who, **exp)], read_only=ro)

# --- raft_test.go:2231-2280: one voter and a learner: IsSingleton answers at once
for i, (who, wri) in enumerate(((1, 11), (2, 21), (1, 31), (2, 41))):
    c = ctx(b"ctx%d" % (i + 1))
    src = "raft_test.go:2231-2280"
    if who != 1:
        add(f"TestReadOnlyWithLearner/{i}/learner", src,
            follower([1, 2], 2, 1, wri, voters=[1]), [read(c, who, status="forward")])
    add(f"TestReadOnlyWithLearner/{i}/leader", src, settled([1, 2], 1, wri, voters=[1]),
        [read(c, who, status="read_state" if who == 1 else "resp", index=wri, queue=[])])

# --- raft_test.go:2341-2411: elected at term 2 over a log of term 1 with MsgApp
# dropped, so nothing of term 2 is committed: the read is postponed.  Once index
# 4 commits, the released message is queued at 4 (windex) -------------------------
n = node(IDS3, 1, [pr(3, 4, 1), pr(0, 3, 0, probe_sent=True, recent_active=True),
                   pr(0, 3, 0, probe_sent=True, recent_active=True)],
         terms=[0, 1, 1, 2], term=2, committed=1)
c = ctx(b"ctx")
add("TestReadOnlyForNewLeader", "raft_test.go:2341-2411", n,
    [read(c, 1, status="postponed", pending=True, queue=[]),
     {"op": "set", "terms": [0, 1, 1, 2, 2], "committed": 4, "pending": False,
      "progress": {"1": pr(4, 5, 1), "2": pr(4, 5, 1, recent_active=True),
                   "3": pr(0, 3, 0, probe_sent=True, recent_active=True)}},
     read(c, 1, status="bcast", index=4, heartbeats=[[2, 4], [3, 0]], queue=[[c, 4, [1], 1]])])

# --- rawnode_test.go:587-644: the test stops at raft.step (it swaps the step
# function), so it asserts only the message: a local MsgReadIndex with the
# context, at a single-voter leader.  (somedata2 is 9 bytes; its first 8 here.)
add("TestRawNodeReadIndex", "rawnode_test.go:618-643", settled([1], 1, 1),
    [read(ctx(b"somedata"), 0)])

# --- node_test.go:249-304: the forwarding, From kept --------------------------------
c = ctx(b"testdata")
for who in (2, 3):
    add(f"TestNodeReadIndexToOldLeader/r{who}", "node_test.go:261-283", follower(IDS3, who, 1, 1),
        [read(c, who, status="forward")])
add("TestNodeReadIndexToOldLeader/r1", "node_test.go:285-303",
    follower(IDS3, 1, 3, 2, term=2, terms=[0, 1, 2]),
    [read(c, 2, status="forward"), read(c, 3, status="forward")])


# --- raft_test.go:3435-3799 -----------------------------------------------------------
def elected():
    """newNetwork(nil, nil, nil) after MsgHup at 1: the empty entry of term 1
    is committed everywhere."""
    return settled(IDS3, 1, 1)


def isolated3(extra=0):
    """The same with node 3 cut off before ``extra`` proposals: its MsgApps
    were sent into the void (Replicate, optimistic next, the ring holds them)."""
    n_ = settled(IDS3, 1, 1 + extra)
    n_["progress"]["3"] = pr(1, 2 + extra, 1, recent_active=True, ring=list(range(2, 2 + extra)))
    return n_


TN = lambda to: [TIMEOUT_NOW, to, 0, 0, 0, 0]  # noqa: E731
second_leader = settled(IDS3, 2, 3, term=2, terms=[0, 1, 2, 2])   # node 2 after it took over + a proposal
add("TestLeaderTransferToUpToDateNode", "raft_test.go:3446", elected(),
    [transfer(2, msg=TN(2), transferee=2, started=True, election_elapsed=0)])
add("TestLeaderTransferToUpToDateNode/back", "raft_test.go:3453", second_leader,
    [transfer(1, msg=TN(1), transferee=1, started=True)])
add("TestLeaderTransferToUpToDateNodeFromFollower/follower", "raft_test.go:3474",
    follower(IDS3, 2, 1, 1), [transfer(2, forward=True, msg=None)])
add("TestLeaderTransferToUpToDateNodeFromFollower/leader", "raft_test.go:3474", elected(),
    [transfer(2, term=1, msg=TN(2), transferee=2, started=True)])   # r.send stamped the follower's term
add("TestLeaderTransferToUpToDateNodeFromFollower/back/follower", "raft_test.go:3481",
    follower(IDS3, 1, 2, 3, term=2, terms=[0, 1, 2, 2]), [transfer(1, forward=True, msg=None)])
add("TestLeaderTransferToUpToDateNodeFromFollower/back/leader", "raft_test.go:3481", second_leader,
    [transfer(1, term=2, msg=TN(1), transferee=1, started=True)])
add("TestLeaderTransferToSlowFollower", "raft_test.go:3523-3541", isolated3(1),
    [transfer(3, msg=[APP, 3, 2, 1, 2, 0], transferee=3, started=True)])
n = isolated3(1)    # compacted at applied = 2: the dummy entry is index 2
n.update(first=3, terms=[1], applied=2)
add("TestLeaderTransferAfterSnapshot", "raft_test.go:3543-3573", n,
    [transfer(3, msg=[APP, 3, 2, 1, 2, 0], transferee=3, started=True)])
add("TestLeaderTransferToSelf", "raft_test.go:3589-3598", elected(),
    [transfer(1, msg=None, transferee=0, started=False)])
add("TestLeaderTransferToNonExistingNode", "raft_test.go:3600-3608", elected(),
    [transfer(4, msg=None, transferee=0, started=False)])
add("TestLeaderTransferBack", "raft_test.go:3733-3750", isolated3(),
    [transfer(3, msg=TN(3), transferee=3, started=True),
     transfer(1, msg=None, transferee=0, started=False, aborted=True)])
add("TestLeaderTransferSecondTransferToAnotherNode", "raft_test.go:3754-3771", isolated3(),
    [transfer(3, msg=TN(3), transferee=3, started=True),
     transfer(2, msg=TN(2), transferee=2, started=True, aborted=True)])
add("TestLeaderTransferSecondTransferToSameNode", "raft_test.go:3775-3799", isolated3(),
    [transfer(3, msg=TN(3), transferee=3, started=True, election_elapsed=0),
     {"op": "set", "election_elapsed": 1},                       # heartbeatTimeout ticks
     transfer(3, msg=None, transferee=3, started=False, aborted=False, election_elapsed=1)])

if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "request_tables.json")
    with open(out, "w", encoding="utf-8") as f:
        json.dump({"scenarios": SCENARIOS}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{out}: {len(SCENARIOS)} scenarios")
