#!/usr/bin/env python3
"""Write tests/golden/compact_tables.json: the reference's own tests of
MemoryStorage.CreateSnapshot / Compact and of the log behind a compaction,
transcribed as data.

Everything below is inputs and expected outputs read off the reference's test
files (paths relative to the reference's raft/).  A case is one storage as the
cited test has built it, and the calls it makes on it in order:

  runs     the entries of MemoryStorage.ents, dummy entry first, run-length
           encoded as [first index, term, count]
  unstable the entries of raftLog.unstable behind them, encoded the same way
  snap     [index, term] of ms.snapshot.Metadata
  applied  raftLog.applied (the last stable index where the test has no raftLog:
           a bare MemoryStorage has no notion of it)
  steps    {"op": "snapshot" | "compact", "i": the argument, "err": null |
           "ErrCompacted" | "ErrSnapOutOfDate" | "panic", "want": {...}}

"want" lists what the test checks after the call: index / term / len
(ms.ents[0].Index, ms.ents[0].Term, len(ms.ents)), first (FirstIndex()), snap
([index, term] of the returned snapshot), left (len(raftLog.allEntries())),
last_index, term_at ([index, term] pairs of raftLog.term), unstable ([len,
first index] of raftLog.unstableEntries()).

TestCompactionSideEffects gives every index its own term (1000 terms); a log
here holds eight runs, so it is scaled: the dummy entry's term 0 and seven
terms of 143 entries, term(i) = 1 + (i - 1) // 143.  What the test checks is
unchanged: every term from the compaction index on, lastIndex, the unstable
entries.  Nothing is executed against the reference at test time; the JSON is
committed.
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))

ENTS_345 = [[3, 3, 1], [4, 4, 1], [5, 5, 1]]


def case(name, src, runs, steps, *, unstable=(), snap=(0, 0), applied=None):
    stable_last = runs[-1][0] + runs[-1][2] - 1
    return {"name": name, "src": src, "runs": [list(r) for r in runs],
            "unstable": [list(r) for r in unstable], "snap": list(snap),
            "applied": stable_last if applied is None else applied, "steps": steps}


def step(op, i, err=None, **want):
    return {"op": op, "i": i, "err": err, "want": want}


def storage_tables():
    out = []
    # storage_test.go:122-142: FirstIndex is 4, and 5 behind Compact(4).
    out.append(case("TestStorageFirstIndex", "storage_test.go:122-142", ENTS_345,
                    [step("compact", 4, first=5)]))
    # storage_test.go:144-176: {i, werr, windex, wterm, wlen}
    for k, (i, err, windex, wterm, wlen) in enumerate([
            (2, "ErrCompacted", 3, 3, 3), (3, "ErrCompacted", 3, 3, 3), (4, None, 4, 4, 2),
            (5, None, 5, 5, 1)]):
        out.append(case(f"TestStorageCompact#{k}", "storage_test.go:144-176", ENTS_345,
                        [step("compact", i, err, index=windex, term=wterm, len=wlen)]))
    # storage_test.go:178-203: {i, werr, wsnap.Metadata.Index / Term}
    for k, (i, err, sidx, sterm) in enumerate([(4, None, 4, 4), (5, None, 5, 5)]):
        out.append(case(f"TestStorageCreateSnapshot#{k}", "storage_test.go:178-203", ENTS_345,
                        [step("snapshot", i, err, snap=[sidx, sterm])]))
    return out


def log_tables():
    out = []
    log1000 = [[0, 0, 1001]]    # NewMemoryStorage's dummy and Append of {Index: i}, i = 1..1000
    # log_test.go:532-578: {lastIndex, compact, wleft, wallow}; committed and
    # applied are lastIndex (maybeCommit + appliedTo).
    out.append(case("TestCompaction#0", "log_test.go:532-578", log1000,
                    [step("compact", 1001, "panic")]))                    # out of upper bound
    out.append(case("TestCompaction#1", "log_test.go:532-578", log1000,
                    [step("compact", 300, left=700), step("compact", 500, left=500),
                     step("compact", 800, left=200), step("compact", 900, left=100)]))
    out.append(case("TestCompaction#2", "log_test.go:532-578", log1000,
                    [step("compact", 300, left=700),
                     step("compact", 299, "ErrCompacted")]))              # out of lower bound
    # log_test.go:277-338, scaled to eight runs (see above): 750 stable entries,
    # 250 unstable, everything committed and applied, Compact(500).
    term = lambda i: 0 if i == 0 else 1 + (i - 1) // 143  # noqa: E731

    def rle(lo, hi):
        runs = []
        for i in range(lo, hi + 1):
            if runs and runs[-1][1] == term(i):
                runs[-1][2] += 1
            else:
                runs.append([i, term(i), 1])
        return runs

    out.append(case("TestCompactionSideEffects", "log_test.go:277-338", rle(0, 750),
                    [step("compact", 500, last_index=1000,
                          term_at=[[j, term(j)] for j in range(500, 1001)], unstable=[250, 751])],
                    unstable=rle(751, 1000), applied=1000))
    return out


def raft_tables():
    out = []
    # raft_test.go:3065-3076 (TestSlowNodeRestore): the leader's election entry
    # and 101 proposals at term 1, all applied (nextEnts), then
    # CreateSnapshot(applied) and Compact(applied).
    out.append(case("TestSlowNodeRestore", "raft_test.go:3075-3076", [[0, 0, 1], [1, 1, 102]],
                    [step("snapshot", 102, snap=[102, 1]),
                     step("compact", 102, index=102, term=1, len=1, first=103)]))
    # raft_test.go:3543-3553 (TestLeaderTransferAfterSnapshot): the election
    # entry and one proposal.
    out.append(case("TestLeaderTransferAfterSnapshot", "raft_test.go:3552-3553",
                    [[0, 0, 1], [1, 1, 2]],
                    [step("snapshot", 2, snap=[2, 1]),
                     step("compact", 2, index=2, term=1, len=1, first=3)]))
    # testdata/snapshot_succeed_via_app_resp.txt:15-30: a storage that starts at
    # a snapshot of index 10 (term 1), the election entry 11, "compact 1 11";
    # line 89 logs the leader's "firstindex: 12" and a snapshot of index 11.
    out.append(case("snapshot_succeed_via_app_resp", "testdata/snapshot_succeed_via_app_resp.txt:15-30",
                    [[10, 1, 2]], [step("compact", 11, index=11, term=1, len=1, first=12)],
                    snap=(10, 1)))
    return out


def main():
    tables = {"storage": storage_tables(), "log": log_tables(), "raft": raft_tables()}
    with open(os.path.join(HERE, "compact_tables.json"), "w") as f:
        json.dump(tables, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
