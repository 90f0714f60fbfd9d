"""CPU restatement of etcd's MsgApp path at a non-leader — TEST INFRASTRUCTURE
ONLY.

One node, one message at a time, on top of tests/follower_ref.py (which steps
the other record kinds; it is imported, not edited).  Paths are relative to
the reference's ``raft/``:

  Step: term filter                            raft.go:847-920
  stepLeader (no case for MsgApp)              raft.go:991-1370
  stepCandidate MsgApp                         raft.go:1390-1392
  stepFollower MsgApp                          raft.go:1433-1435
  handleAppendEntries                          raft.go:1475-1511
  raftLog.maybeAppend / append                 log.go:88-118
  raftLog.findConflict                         log.go:130-141
  raftLog.findConflictByTerm                   log.go:150-171
  raftLog.commitTo                             log.go:236-244
  raftLog.term / matchTerm                     log.go:268-288, 320-326
  unstable.truncateAndAppend                   log_unstable.go:121-145

The log is a plain list of terms, one per entry: ``terms[k]`` is the term of
index ``first_index - 1 + k`` (``terms[0]`` the dummy entry's).  Every rule is
followed entry by entry as Go does; the engine's run table appears only at
the edges (``runs_of`` / ``terms_of_runs``), so nothing here shares the
kernel's run arithmetic.

A record is tried on a copy of the node: where Go would panic, or the log
would need more than MAX_RUNS term runs, the copy is dropped, the node stays
untouched and the record stops its group.
"""
from __future__ import annotations

import copy
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

from tests import follower_ref as fr
from tests.follower_ref import (CANDIDATE, FFLAG_HARDSTATE, FFLAG_RESET, FOLLOWER, LEADER,  # noqa: F401
                          MSG_APP_RESP, NO_STOP, PRE_CANDIDATE, REJECT, Config, Rec)

APP = 5  # QB_FIN_APP
FFLAG_LOG_CONFLICT, FFLAG_LOG_RUNS, FFLAG_APPENDED = 0x20, 0x40, 0x80
FFLAG_STOPS = fr.FFLAG_STOPS | FFLAG_LOG_CONFLICT | FFLAG_LOG_RUNS
MAX_RUNS = 8
U64 = (1 << 64) - 1
FLSTAT_NAMES = fr.FSTAT_NAMES + ("app_accepted", "app_rejected", "app_below_commit",
                                 "entries_appended", "app_truncated")


class GoPanic(Exception):
    """A logger.Panicf / slice-bounds panic of the reference."""


@dataclass
class LogNode(fr.Node):
    """follower_ref.Node plus the log's terms."""
    first_index: int = 1
    terms: List[int] = field(default_factory=lambda: [0])  # [first_index - 1 .. last_index]

    def sync(self) -> None:
        self.last_index = (self.first_index - 1 + len(self.terms) - 1) & U64
        self.last_term = self.terms[-1]

    # raftLog.term, log.go:268-288 (the storage never errs here)
    def log_term(self, i: int) -> int:
        dummy = self.first_index - 1
        if i < dummy or i > self.last_index:
            return 0
        return self.terms[i - dummy]

    def match_term(self, i: int, term: int) -> bool:       # log.go:320-326
        return self.log_term(i) == term


@dataclass
class AppRec(Rec):
    """A MsgApp: index = Message.Index, aux = Message.LogTerm, the entries'
    terms one per entry (indexes index + 1, ...), commit = Message.Commit."""
    commit: int = 0
    ents: List[int] = field(default_factory=list)


def new_node(terms: List[int], first_index: int = 1, **kw) -> LogNode:
    n = LogNode(first_index=first_index, terms=list(terms), **kw)
    n.sync()
    return n


def runs_of(terms: List[int], first_index: int) -> Tuple[List[int], List[int]]:
    """The run table of a log: (starts, terms), maximal runs of equal term."""
    starts, rterms = [], []
    for k, t in enumerate(terms):
        if not rterms or rterms[-1] != t:
            starts.append((first_index - 1 + k) & U64)
            rterms.append(t)
    return starts, rterms


def terms_of_runs(starts: List[int], rterms: List[int], last_index: int) -> List[int]:
    out = []
    for r, (s, t) in enumerate(zip(starts, rterms)):
        end = starts[r + 1] - 1 if r + 1 < len(starts) else last_index
        out += [t] * (end - s + 1)
    return out


def rle(ents: List[int]) -> List[Tuple[int, int]]:
    """Entry terms -> (term, length) runs, as the app inbox carries them."""
    out: List[List[int]] = []
    for t in ents:
        if out and out[-1][0] == t:
            out[-1][1] += 1
        else:
            out.append([t, 1])
    return [(t, n) for t, n in out]


def _find_conflict(n: LogNode, index: int, ents: List[int]) -> int:
    """log.go:130-141; entry k has Index index + 1 + k."""
    for k, t in enumerate(ents):
        ei = (index + 1 + k) & U64
        if not n.match_term(ei, t):
            return ei
    return 0


def _find_conflict_by_term(n: LogNode, index: int, term: int) -> int:
    """log.go:150-171."""
    if index > n.last_index:
        return index
    while True:
        if n.log_term(index) <= term:
            break
        index = (index - 1) & U64
    return index


def _commit_to(n: LogNode, tocommit: int) -> None:
    """log.go:236-244."""
    if n.committed < tocommit:
        if n.last_index < tocommit:
            raise GoPanic("tocommit out of range")
        n.committed = tocommit


def _maybe_append(n: LogNode, m: AppRec):
    """log.go:88-107 with append (109-118) and unstable.truncateAndAppend
    (log_unstable.go:121-145) over the list.  Returns (lastnewi, ok, ci)."""
    if not n.match_term(m.index, m.aux):
        return 0, False, 0
    lastnewi = (m.index + len(m.ents)) & U64
    ci = _find_conflict(n, m.index, m.ents)
    if ci == 0:
        pass
    elif ci <= n.committed:
        raise GoPanic("conflict with committed entry")      # log.go:94-95
    else:
        offset = (m.index + 1) & U64
        tail = m.ents[ci - offset:]                          # log.go:97-101
        after = ci                                           # ents[0].Index
        if after - 1 < n.committed:                          # log.go:113-115
            raise GoPanic("after out of range")
        if after > n.last_index + 1:                         # u.slice -> mustCheckOutOfBounds
            raise GoPanic("slice out of bound")
        dummy = n.first_index - 1
        assert after > dummy, "an append at or below the dummy entry"
        n.terms = n.terms[:after - dummy] + tail             # truncate, then append
        n.sync()
    _commit_to(n, min(m.commit, lastnewi))                   # log.go:103
    return lastnewi, True, ci


def _handle_append_entries(n: LogNode, m: AppRec, st: dict):
    """raft.go:1475-1511.  Returns (index, reject, hint, log_term, app_from)."""
    if m.index < n.committed:                                # raft.go:1476-1479
        st["app_below_commit"] += 1
        return n.committed, False, None, None, 0
    old_last = n.last_index
    lastnewi, ok, ci = _maybe_append(n, m)
    if ok:                                                   # raft.go:1481-1482
        if len(runs_of(n.terms, n.first_index)[0]) > MAX_RUNS:
            raise OverflowError("a 9th term run")
        st["app_accepted"] += 1
        if ci != 0:
            st["entries_appended"] += (lastnewi - ci + 1) & U64
            if ci <= old_last:
                st["app_truncated"] += 1
        return lastnewi, False, None, None, ci
    hint = _find_conflict_by_term(n, min(m.index, n.last_index), m.aux)   # raft.go:1496-1497
    st["app_rejected"] += 1
    return m.index, True, hint, n.log_term(hint), 0          # raft.go:1498-1509


def step_app(n: LogNode, m: AppRec, cfg: Config, st: dict):
    """raft.Step(MsgApp).  Returns (resp_type, resp_term, flags, index, hint,
    log_term, app_from); hint / log_term are None unless the answer is a
    rejection.  A record that stops leaves ``n`` (and ``st``) untouched."""
    none = (0, None, None, 0)
    if m.term != 0 and m.term < n.term:                      # raft.go:883-919
        if cfg.check_quorum or cfg.pre_vote:
            st["stale_answered"] += 1
            return (MSG_APP_RESP, n.term, 0) + none          # raft.go:906; send: Term = r.Term
        st["stale_ignored"] += 1
        return (0, 0, 0) + none
    t, s = copy.deepcopy(n), dict(st)
    gf = 0
    if m.term != 0 and m.term > t.term:                      # raft.go:876-877
        gf |= fr._become_follower(t, m.term, m.frm, s)
    if t.state == LEADER:                                    # stepLeader: no case
        st["role_ignored"] += 1
        return (0, 0, 0) + none
    if t.state in (CANDIDATE, PRE_CANDIDATE):                # raft.go:1390-1392
        gf |= fr._become_follower(t, m.term, m.frm, s)
    else:                                                    # raft.go:1433-1435
        t.election_elapsed = 0
        t.lead = m.frm
    try:
        index, reject, hint, lterm, app_from = _handle_append_entries(t, m, s)
    except GoPanic as e:
        flag = FFLAG_COMMIT_RANGE if "tocommit" in str(e) else FFLAG_LOG_CONFLICT
        return (0, 0, flag) + none
    except OverflowError:
        return (0, 0, FFLAG_LOG_RUNS) + none
    if app_from:
        gf |= FFLAG_APPENDED
    n.__dict__.update(t.__dict__)
    st.update(s)
    rt = MSG_APP_RESP | (REJECT if reject else 0)
    return rt, n.term, gf, index, hint, lterm, app_from      # send: Term = r.Term


FFLAG_COMMIT_RANGE = fr.FFLAG_COMMIT_RANGE


def new_stats() -> dict:
    return {k: 0 for k in FLSTAT_NAMES}


def step_batch(nodes: List[LogNode], recs: List[Tuple[int, Rec]], cfg: Config,
               st: Optional[dict] = None, on_append=None):
    """follower_ref.step_batch with APP records.  Returns a dict: resp_type,
    resp_term, resp_index, app_from [M] (0 where none), resp_hint,
    resp_log_term [M] (None where not written), stop_at, gflags [G], stats.
    on_append(g, node): called behind every record that changed g's log."""
    st = new_stats() if st is None else st
    G, M = len(nodes), len(recs)
    out = {"resp_type": [0] * M, "resp_term": [0] * M, "resp_index": [0] * M,
           "app_from": [0] * M, "resp_hint": [None] * M, "resp_log_term": [None] * M,
           "stop_at": [NO_STOP] * G, "gflags": [0] * G, "stats": st}
    hard0 = [(n.term, n.vote, n.committed) for n in nodes]
    for i, (g, m) in enumerate(recs):
        if not 0 <= g < G:
            st["bad_group"] += 1
            continue
        if m.kind > APP:
            st["bad_kind"] += 1
            continue
        if out["stop_at"][g] != NO_STOP:
            st["after_stop"] += 1
            continue
        if m.kind == APP:
            rt, rterm, gf, idx, hint, lterm, af = step_app(nodes[g], m, cfg, st)
            out["resp_index"][i], out["app_from"][i] = idx, af
            out["resp_hint"][i], out["resp_log_term"][i] = hint, lterm
            if af and on_append is not None:
                on_append(g, nodes[g])
        else:
            rt, rterm, gf = fr.step(nodes[g], m, cfg, st)
        out["resp_type"][i], out["resp_term"][i] = rt, rterm
        out["gflags"][g] |= gf
        if gf & FFLAG_STOPS:
            out["stop_at"][g] = i
    for g, n in enumerate(nodes):
        if (n.term, n.vote, n.committed) != hard0[g]:
            out["gflags"][g] |= FFLAG_HARDSTATE
    return out
