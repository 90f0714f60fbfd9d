#!/usr/bin/env python3
"""Write tests/golden/ready_tables.json: the reference's own tests of the Ready
cycle — hasNextEnts / nextEnts / unstableEntries / stableTo on the log, the
bare unstable's stableTo, containsUpdates and the two state comparisons, and
the Ready sequences of four RawNode tests — transcribed as data.

Everything below is inputs and expected outputs read off the reference's test
files (paths relative to the reference's raft/).  A node is the state the
cited test has built before the checked call, restated as the fields the Ready
cycle reads:

  first    raftLog.firstIndex()
  terms    the terms of [first - 1, lastIndex]: the dummy entry (the snapshot's
           term, 0 for an empty storage) and one per entry
  offset   unstable.offset (lastIndex of the storage + 1 when the log was made,
           log.go:73)
  committed / applied, snap ([index, term] of unstable.snapshot or null),
  term / vote / lead / state, prev_soft ([lead, state]) / prev_hard ([term,
  vote, commit]) as NewRawNode leaves them (rawnode.go:52-53), msgs,
  read_states, uncommitted_size.

In a sequence, "then" is what the test's next calls outside the Ready cycle
(Campaign, Propose, Step) leave in those fields; the batched engine has its own
calls for them, whose tables are the other files here.  Nothing is executed
against the reference at test time; the JSON is committed.
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))

FOLLOWER, CANDIDATE, LEADER = 0, 1, 2


def node(first, terms, committed, applied, offset, *, snap=None, term=0, vote=0, lead=0,
         state=FOLLOWER, msgs=False, read_states=False, uncommitted_size=0):
    return {"first": first, "terms": terms, "committed": committed, "applied": applied,
            "offset": offset, "snap": snap, "term": term, "vote": vote, "lead": lead,
            "state": state, "prev_soft": [lead, state], "prev_hard": [term, vote, committed],
            "msgs": msgs, "read_states": read_states, "uncommitted_size": uncommitted_size}


def log_tables():
    # log_test.go:340-371, 373-406: a storage snapshot (index 3, term 1), the
    # entries 4..6 of term 1 appended (unstable), maybeCommit(5, 1), then
    # appliedTo(applied) — appliedTo(0) is a no-op (log.go:247-249).
    snap_log = node(4, [1, 1, 1, 1], 5, 3, 4)
    has_next = {"name": "TestHasNextEnts", "src": "log_test.go:340-371", "node": snap_log,
                "rows": [{"applied_to": 0, "has_next": True}, {"applied_to": 3, "has_next": True},
                         {"applied_to": 4, "has_next": True}, {"applied_to": 5, "has_next": False}]}
    next_ents = {"name": "TestNextEnts", "src": "log_test.go:373-406", "node": snap_log,
                 "rows": [{"applied_to": 0, "want": [4, 5]}, {"applied_to": 3, "want": [4, 5]},
                          {"applied_to": 4, "want": [5, 5]}, {"applied_to": 5, "want": None}]}
    # log_test.go:408-437: entries (1, term 1), (2, term 2); those below
    # `unstable` are in the storage.  want: [first, last, last's term];
    # the test then calls stableTo on the last one and expects offset 3.
    unstable_ents = {"name": "TestUnstableEnts", "src": "log_test.go:408-437",
                     "rows": [{"node": node(1, [0, 1, 2], 0, 0, 3), "want": None, "woffset": 3},
                              {"node": node(1, [0, 1, 2], 0, 0, 1), "want": [1, 2, 2],
                               "woffset": 3}]}
    # log_test.go:473-492: both entries unstable over an empty storage.
    stable_to = {"name": "TestStableTo", "src": "log_test.go:473-492",
                 "node": node(1, [0, 1, 2], 0, 0, 1),
                 "rows": [{"index": 1, "term": 1, "woffset": 2}, {"index": 2, "term": 2, "woffset": 3},
                          {"index": 2, "term": 1, "woffset": 1}, {"index": 3, "term": 1, "woffset": 1}]}
    # log_test.go:494-524: a storage snapshot (index 5, term 2); newEnts is
    # nothing or the one entry (6, term 2).
    bare, one = node(6, [2], 5, 5, 6), node(6, [2, 2], 5, 5, 6)
    rows = []
    for nd, offs in ((bare, (6, 6, 6, 6, 6, 6)), (one, (7, 6, 6, 6, 6, 6))):
        for (i, t), w in zip(((6, 2), (5, 2), (4, 2), (6, 3), (5, 3), (4, 3)), offs):
            rows.append({"node": nd, "index": i, "term": t, "woffset": w})
    with_snap = {"name": "TestStableToWithSnap", "src": "log_test.go:494-524", "rows": rows}
    return [has_next, next_ents, unstable_ents, stable_to, with_snap]


def unstable_table():
    # log_unstable_test.go:219-300, all 11 rows: a bare unstable{entries,
    # offset, snapshot}, stableTo(index, term), then offset and len(entries).
    # entries: the terms of offset, offset + 1, ...
    def row(terms, offset, snap, index, term, woffset, wlen):
        return {"entries": terms, "offset": offset, "snap": snap, "index": index, "term": term,
                "woffset": woffset, "wlen": wlen}
    return {"name": "TestUnstableStableTo", "src": "log_unstable_test.go:219-300", "rows": [
        row([], 0, None, 5, 1, 0, 0),
        row([1], 5, None, 5, 1, 6, 0),
        row([1, 1], 5, None, 5, 1, 6, 1),
        row([2], 6, None, 6, 1, 6, 1),
        row([1], 5, None, 4, 1, 5, 1),
        row([1], 5, None, 4, 2, 5, 1),
        row([1], 5, [4, 1], 5, 1, 6, 0),
        row([1, 1], 5, [4, 1], 5, 1, 6, 1),
        row([2], 6, [5, 1], 6, 1, 6, 1),
        row([1], 5, [4, 1], 4, 1, 5, 1),
        row([2], 5, [4, 2], 4, 1, 5, 1)]}


def node_tables():
    def rd(want, **kw):
        r = {"soft": None, "hard": [0, 0, 0], "entries": 0, "committed": 0, "msgs": 0,
             "snap_index": 0, "want": want}
        r.update(kw)
        return r
    contain = {"name": "TestReadyContainUpdates", "src": "node_test.go:558-577", "rows": [
        rd(False), rd(True, soft=[1, FOLLOWER]), rd(True, hard=[0, 1, 0]), rd(True, entries=1),
        rd(True, committed=1), rd(True, msgs=1), rd(True, snap_index=1)]}
    # against the zero value
    soft = {"name": "TestSoftStateEqual", "src": "node_test.go:779-793", "rows": [
        {"soft": [0, FOLLOWER], "equal": True}, {"soft": [1, FOLLOWER], "equal": False},
        {"soft": [0, LEADER], "equal": False}]}
    hard = {"name": "TestIsHardStateEqual", "src": "node_test.go:795-811", "rows": [
        {"hard": [0, 0, 0], "equal": True}, {"hard": [0, 1, 0], "equal": False},
        {"hard": [0, 0, 1], "equal": False}, {"hard": [1, 0, 0], "equal": False}]}
    return [contain, soft, hard]


def ready(flags, *, soft=None, hard=(0, 0, 0), entries=None, committed=None, snap_index=0):
    """An expected Ready: flags by name (must_sync included), and the parts."""
    return {"op": "ready", "flags": sorted(flags), "soft": soft, "hard": list(hard),
            "entries": entries, "committed": committed, "snap_index": snap_index}


def sequences():
    seqs = []
    # rawnode_test.go:658-762.  The storage is bootstrapped with a snapshot at
    # index 1, term 0 (first index 2); NewRawNode: HardState{Commit: 1}.
    # Campaign (a single voter wins at once) appends the empty entry 2 at
    # term 1 and commits it; Propose("foo") appends entry 3 (payload 3) and
    # commits it.  Advance: the entries are stable, entries 2..3 applied
    # (payload 0 + 3).
    seqs.append({"name": "TestRawNodeStart", "src": "rawnode_test.go:658-762",
                 "node": node(2, [0], 1, 1, 2),
                 "steps": [
                     {"op": "has_ready", "want": False},
                     {"op": "then", "set": {"term": 1, "vote": 1, "lead": 1, "state": LEADER,
                                            "terms": [0, 1, 1], "committed": 3,
                                            "uncommitted_size": 3}},
                     {"op": "has_ready", "want": True},
                     ready(["soft", "hard", "entries", "committed", "must_sync"], soft=[1, LEADER],
                           hard=(1, 1, 3), entries=[2, 3, 1], committed=[2, 3]),
                     {"op": "advance", "payload": 3},
                     {"op": "has_ready", "want": False}]})
    # rawnode_test.go:764-793.  Storage: entries (1, term 1), (2, term 1),
    # HardState{Term: 1, Commit: 1}; nothing applied yet.
    seqs.append({"name": "TestRawNodeRestart", "src": "rawnode_test.go:764-793",
                 "node": node(1, [0, 1, 1], 1, 0, 3, term=1),
                 "steps": [ready(["committed"], committed=[1, 1]),
                           {"op": "advance", "payload": 0},
                           {"op": "has_ready", "want": False}]})
    # rawnode_test.go:795-833.  Storage: a snapshot (index 2, term 1), the
    # entry (3, term 1), HardState{Term: 1, Commit: 3}.
    seqs.append({"name": "TestRawNodeRestartFromSnapshot", "src": "rawnode_test.go:795-833",
                 "node": node(3, [1, 1], 3, 2, 4, term=1),
                 "steps": [ready(["committed"], committed=[3, 3]),
                           {"op": "advance", "payload": 3},
                           {"op": "has_ready", "want": False}]})
    # rawnode_test.go:882-952.  Storage: entries 1..11 of term 1,
    # HardState{Term: 1, Vote: 1, Commit: 10}.  MaxSizePerMsg makes limitSize
    # cut the first CommittedEntries after entry 9 ("trim_to"); the test then
    # Steps a MsgHeartbeat{From: 1, Term: 1, Commit: 11}: lead = 1, committed =
    # 11 and a MsgHeartbeatResp in r.msgs.  The next Ready must start at 10.
    seqs.append({"name": "TestRawNodeCommitPaginationAfterRestart",
                 "src": "rawnode_test.go:882-952",
                 "node": node(1, [0] + [1] * 11, 10, 0, 12, term=1, vote=1),
                 "steps": [ready(["committed"], committed=[1, 10]),
                           {"op": "advance", "trim_to": 9, "payload": 9},
                           {"op": "then", "set": {"lead": 1, "committed": 11, "msgs": True}},
                           ready(["soft", "hard", "committed", "msgs"], soft=[1, FOLLOWER],
                                 hard=(1, 1, 11), committed=[10, 11]),
                           {"op": "advance", "payload": 5}]})
    return seqs


def main():
    doc = {"log": log_tables(), "unstable": unstable_table(), "node": node_tables(),
           "sequences": sequences()}
    with open(os.path.join(HERE, "ready_tables.json"), "w", encoding="utf-8") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
