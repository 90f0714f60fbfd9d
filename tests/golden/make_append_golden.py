#!/usr/bin/env python3
"""Write tests/golden/append_tables.json: the reference's own tests of the
MsgApp path at a follower, transcribed as data.

Everything below is inputs and expected outputs read off the reference's test
files (paths relative to the reference's raft/).  A log is the list of its
entries' terms from index 1 on (every one of these tests starts at index 1
with an empty snapshot, so the dummy entry is index 0, term 0); a message's
entries are the list of their terms, at indexes Index + 1, Index + 2, ...
Nothing here is executed against the reference at test time; the JSON is
committed.

  handle_msg_app     TestHandleMsgApp          raft_test.go:1232-1278
  find_conflict      TestFindConflict          log_test.go:24-56
  maybe_append       TestLogMaybeAppend        log_test.go:155-277
  check_msg_app      TestFollowerCheckMsgApp   raft_paper_test.go:601-639
  append_entries     TestFollowerAppendEntries raft_paper_test.go:646-693
  fast_log_rejection TestFastLogRejection      raft_test.go:4319-4602 (the follower's side)
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def handle_msg_app():
    # storage {1,t1} {2,t2}; becomeFollower(2, None); handleAppendEntries(m)
    # called directly (the message's Term does not pass the term filter).
    # (m.Term, LogTerm, Index, Commit, entries) -> wIndex, wCommit, wReject
    rows = [
        (2, 3, 2, 3, [], 2, 0, True),      # previous log mismatch
        (2, 3, 3, 3, [], 2, 0, True),      # previous log non-exist
        (2, 1, 1, 1, [], 2, 1, False),
        (2, 0, 0, 1, [2], 1, 1, False),
        (2, 2, 2, 3, [2, 2], 4, 3, False),
        (2, 2, 2, 4, [2], 3, 3, False),
        (2, 1, 1, 4, [2], 2, 2, False),
        (1, 1, 1, 3, [], 2, 1, False),     # match entry 1, commit up to last new entry 1
        (1, 1, 1, 3, [2], 2, 2, False),    # match entry 1, commit up to last new entry 2
        (2, 2, 2, 3, [], 2, 2, False),     # match entry 2, commit up to last new entry 2
        (2, 2, 2, 4, [], 2, 2, False),     # commit up to log.last()
    ]
    return {"cite": "raft/raft_test.go:1232-1278", "log": [1, 2], "term": 2, "committed": 0,
            "rows": [{"m_term": t, "log_term": lt, "index": i, "commit": c, "ents": e,
                      "w_index": wi, "w_commit": wc, "w_reject": wr}
                     for t, lt, i, c, e, wi, wc, wr in rows]}


def find_conflict():
    # previousEnts {1,t1} {2,t2} {3,t3}; (index of the first entry, terms) -> wconflict
    rows = [
        (1, [], 0),                      # no conflict, empty ent
        (1, [1, 2, 3], 0),               # no conflict
        (2, [2, 3], 0),
        (3, [3], 0),
        (1, [1, 2, 3, 4, 4], 4),         # no conflict, but has new entries
        (2, [2, 3, 4, 4], 4),
        (3, [3, 4, 4], 4),
        (4, [4, 4], 4),
        (1, [4, 4], 1),                  # conflicts with existing entries
        (2, [1, 4, 4], 2),
        (3, [1, 2, 4, 4], 3),
    ]
    return {"cite": "raft/log_test.go:24-56", "log": [1, 2, 3],
            "rows": [{"first": f, "ents": e, "w_conflict": w} for f, e, w in rows]}


def maybe_append():
    # previousEnts {1,t1} {2,t2} {3,t3}, committed = 1
    li, lt, commit = 3, 3, 1
    # (logTerm, index, committed, entries) -> wlasti, wappend, wcommit, wpanic
    rows = [
        (lt - 1, li, li, [4], 0, False, commit, False),      # not match: term is different
        (lt, li + 1, li, [4], 0, False, commit, False),      # not match: index out of bound
        (lt, li, li, [], li, True, li, False),               # match with the last existing entry
        (lt, li, li + 1, [], li, True, li, False),           # not higher than lastnewi
        (lt, li, li - 1, [], li, True, li - 1, False),       # up to the commit in the message
        (lt, li, 0, [], li, True, commit, False),            # commit do not decrease
        (0, 0, li, [], 0, True, commit, False),              # commit do not decrease
        (lt, li, li, [4], li + 1, True, li, False),
        (lt, li, li + 1, [4], li + 1, True, li + 1, False),
        (lt, li, li + 2, [4], li + 1, True, li + 1, False),  # not higher than lastnewi
        (lt, li, li + 2, [4, 4], li + 2, True, li + 2, False),
        (lt - 1, li - 1, li, [4], li, True, li, False),      # match with the entry in the middle
        (lt - 2, li - 2, li, [4], li - 1, True, li - 1, False),
        (lt - 3, li - 3, li, [4], li - 2, True, li - 2, True),  # conflict with committed entry
        (lt - 2, li - 2, li, [4, 4], li, True, li, False),
    ]
    return {"cite": "raft/log_test.go:155-277", "log": [1, 2, 3], "committed": commit,
            "rows": [{"log_term": a, "index": b, "commit": c, "ents": e, "w_lasti": wl,
                      "w_append": wa, "w_commit": wc, "w_panic": wp}
                     for a, b, c, e, wl, wa, wc, wp in rows]}


def check_msg_app():
    # storage {1,t1} {2,t2}, HardState{Commit: 1}, becomeFollower(2, 2);
    # Step(MsgApp{From: 2, Term: 2, LogTerm, Index}) -> one MsgAppResp{Term: 2, ...}
    rows = [
        (0, 0, 1, False, 0, 0),      # match with committed entries
        (1, 1, 1, False, 0, 0),
        (2, 2, 2, False, 0, 0),      # match with uncommitted entries
        (1, 2, 2, True, 1, 1),       # unmatch with existing entry
        (3, 3, 3, True, 2, 2),       # unexisting entry
    ]
    return {"cite": "raft/raft_paper_test.go:601-639", "log": [1, 2], "term": 2, "lead": 2,
            "committed": 1, "from": 2,
            "rows": [{"log_term": t, "index": i, "w_index": wi, "w_reject": wr, "w_hint": wh,
                      "w_log_term": wl} for t, i, wi, wr, wh, wl in rows]}


def append_entries():
    # storage {1,t1} {2,t2}, becomeFollower(2, 2); Step(MsgApp{From: 2, Term: 2, ...});
    # (index, term, entries) -> the log's entries after, the unstable ones
    rows = [
        (2, 2, [3], [1, 2, 3], [3]),
        (1, 1, [3, 4], [1, 3, 4], [3, 4]),
        (0, 0, [1], [1, 2], []),
        (0, 0, [3], [3], [3]),
    ]
    return {"cite": "raft/raft_paper_test.go:646-693", "log": [1, 2], "term": 2, "lead": 2,
            "committed": 0, "from": 2,
            "rows": [{"index": i, "log_term": t, "ents": e, "w_log": w, "w_unstable": u}
                     for i, t, e, w, u in rows]}


def fast_log_rejection():
    # n1 (leaderLog) becomeCandidate, becomeLeader at term 1: it appends an
    # empty entry of term 1 and, on n2's heartbeat response, sends
    # MsgApp{Term: 1, Index: len(leaderLog), LogTerm: its term, Entries: [that
    # entry]}.  n2 (followerLog; term 0) rejects with (RejectHint, LogTerm).
    # (leaderLog, followerLog) -> rejectHintTerm, rejectHintIndex
    rows = [
        ([1, 2, 2, 4, 4, 4, 4], [1, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3], 3, 7),
        ([1, 2, 2, 3, 4, 4, 4, 5], [1, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3], 3, 8),
        ([1, 1, 1, 1], [1, 2, 2, 4], 1, 1),
        ([1, 1, 1, 1, 1, 1], [1, 2, 2, 4], 1, 1),
        ([1, 1, 1, 1], [1, 2, 2, 4, 4, 4], 1, 1),
        ([1, 1, 1, 4, 5], [1, 1, 1, 4], 4, 4),
        ([2, 5, 5, 5, 5, 5, 5, 5, 5], [2, 4, 4, 4, 4, 4], 4, 6),
        ([2, 2, 2, 2, 2], [2, 4, 4, 4, 4, 4, 4, 4], 2, 1),
    ]
    return {"cite": "raft/raft_test.go:4319-4602", "term": 1, "from": 1,
            "rows": [{"leader_log": a, "follower_log": b, "w_hint_term": t, "w_hint_index": i}
                     for a, b, t, i in rows]}


def tables():
    return {"handle_msg_app": handle_msg_app(), "find_conflict": find_conflict(),
            "maybe_append": maybe_append(), "check_msg_app": check_msg_app(),
            "append_entries": append_entries(), "fast_log_rejection": fast_log_rejection()}


def main():
    with open(os.path.join(HERE, "append_tables.json"), "w", encoding="utf-8") as f:
        json.dump(tables(), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
