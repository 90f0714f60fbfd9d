"""CPU restatement of etcd's MsgSnap path at a non-leader — TEST
INFRASTRUCTURE ONLY.

One node, one message at a time, statement by statement as Go has it.  Paths
are relative to the reference's ``raft/``:

  Step: term filter                            raft.go:847-920
  stepLeader (no case for MsgSnap)             raft.go:991-1370
  stepCandidate MsgSnap                        raft.go:1396-1398
  stepFollower MsgSnap                         raft.go:1441-1444
  handleSnapshot / restore                     raft.go:1518-1614
  promotable                                   raft.go:1618-1621
  becomeFollower -> reset                      raft.go:686-693, 590-619
  send (stamps Term on non-vote messages)      raft.go:386-418
  raftLog.firstIndex / lastIndex               log.go:214-234
  raftLog.commitTo                             log.go:236-244
  raftLog.term / matchTerm                     log.go:268-288, 320-326
  raftLog.restore                              log.go:336-340
  unstable.maybeFirstIndex / maybeLastIndex / maybeTerm   log_unstable.go:35-73
  unstable.restore                             log_unstable.go:115-119

The log is a plain list of terms, one per index of [first_index - 1,
last_index] (the dummy entry first): ``terms[k]`` is the term of index
``first_index - 1 + k``.  A restored log is the snapshot alone: its dummy entry
is the snapshot's (index, term) and it has no entries.  The engine's run table
appears only at the edges (tests/snapshot_pack.py), so nothing here shares the
kernel's run arithmetic.

What is modelled of ``reset`` and of ``restore`` is their effect on the fields
the engine's call owns.  Of restore that is the log, the unstable snapshot and
promotable(); the ProgressTracker reset, confchange.Restore and the own slot's
MaybeUpdate stay the host's, and the ``r.state != StateFollower`` branch is
unreachable (both callers have made the node a follower; it is asserted).

A record is tried on a copy of the node: where Go would panic (commitTo past
the last index) the copy is dropped, the node stays untouched and the record
is the stop SNF_COMMIT_RANGE.
"""
from __future__ import annotations

import copy
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

U64 = (1 << 64) - 1
FOLLOWER, CANDIDATE, LEADER, PRE_CANDIDATE = 0, 1, 2, 3
NONE = 0
MSG_APP_RESP = 4
RDP_MSGS = 0x01

SNF_RESTORED, SNF_FAST_FORWARD, SNF_OLD, SNF_NOT_MEMBER = 0x001, 0x002, 0x004, 0x008
SNF_STALE, SNF_ROLE_IGNORED, SNF_RESET, SNF_COMMIT_RANGE = 0x010, 0x020, 0x040, 0x080
SNF_BAD_GROUP, SNF_HARDSTATE = 0x100, 0x200
SNF_ALL = 0x3FF
SSTAT_NAMES = ("restored", "fast_forward", "old", "not_member", "stale", "role_ignored",
               "became_follower", "commit_range", "bad_group")
CS_LISTS = ("voters", "learners", "voters_outgoing", "learners_next")


class Panic(Exception):
    """logger.Panicf of the reference."""


@dataclass
class Node:
    """raft + raftLog + unstable as the MsgSnap path sees them."""
    id: int = 1
    term: int = 0
    vote: int = NONE
    lead: int = NONE
    committed: int = 0
    state: int = FOLLOWER
    promotable: bool = True          # raft.promotable(), as the host keeps it
    role_other: int = 0              # the other bits of the engine's role byte
    election_elapsed: int = 0
    heartbeat_elapsed: int = 0
    first_index: int = 1             # raftLog.firstIndex()
    terms: List[int] = field(default_factory=lambda: [0])  # [first_index - 1 .. last_index]
    offset: int = 1                  # unstable.offset
    snap: Optional[Tuple[int, int]] = None  # unstable.snapshot's (Index, Term)
    pending: int = 0                 # QB_RDP_*: bit 0 = len(r.msgs) > 0

    @property
    def last_index(self) -> int:     # log.go:225-234
        return (self.first_index - 1 + len(self.terms) - 1) & U64

    @property
    def last_term(self) -> int:
        return self.terms[-1]


@dataclass
class Snap:
    """A MsgSnap: From, Term, Snapshot.Metadata.{Index, Term, ConfState}."""
    frm: int = 0
    term: int = 0
    index: int = 0
    sterm: int = 0
    cs: Dict[str, Sequence[int]] = field(default_factory=dict)


def log_term(n: Node, i: int) -> int:
    """log.go:268-288 (the storage never errs here)."""
    dummy = (n.first_index - 1) & U64
    if i < dummy or i > n.last_index:
        return 0
    return n.terms[i - dummy]


def match_term(n: Node, i: int, term: int) -> bool:
    """log.go:320-326."""
    return log_term(n, i) == term


def commit_to(n: Node, tocommit: int) -> None:
    """log.go:236-244."""
    if n.committed < tocommit:
        if n.last_index < tocommit:
            raise Panic(f"tocommit({tocommit}) is out of range [lastIndex({n.last_index})]")
        n.committed = tocommit


def log_restore(n: Node, index: int, term: int) -> None:
    """raftLog.restore (log.go:336-340) + unstable.restore
    (log_unstable.go:115-119): the log is the snapshot alone."""
    n.committed = index
    n.offset = (index + 1) & U64
    n.snap = (index, term)
    n.first_index = (index + 1) & U64     # maybeFirstIndex, log_unstable.go:35-40
    n.terms = [term]                      # maybeLastIndex / maybeTerm: the snapshot's


def become_follower(n: Node, term: int, lead: int, st: dict) -> int:
    """becomeFollower(term, lead) -> reset(term), raft.go:686-693, 590-619."""
    if n.term != term:                     # raft.go:591-594
        n.term = term
        n.vote = NONE
    n.lead = NONE                          # raft.go:595
    n.election_elapsed = 0                 # raft.go:597
    n.heartbeat_elapsed = 0                # raft.go:598
    n.lead = lead                          # raft.go:690
    n.state = FOLLOWER                     # raft.go:691
    st["became_follower"] += 1
    return SNF_RESET


def restore(n: Node, m: Snap) -> Tuple[bool, int]:
    """raft.restore (raft.go:1534-1614) -> (restored, the outcome's flag)."""
    if m.index <= n.committed:                             # raft.go:1535-1537
        return False, SNF_OLD
    assert n.state == FOLLOWER                             # raft.go:1538-1549: unreachable
    found = False                                          # raft.go:1554-1573
    for name in ("voters", "learners", "voters_outgoing"):
        for i in m.cs.get(name, ()):
            if i == n.id:
                found = True
                break
        if found:
            break
    if not found:                                          # raft.go:1574-1580
        return False, SNF_NOT_MEMBER
    if match_term(n, m.index, m.sterm):                    # raft.go:1584-1589
        commit_to(n, m.index)
        return False, SNF_FAST_FORWARD
    log_restore(n, m.index, m.sterm)                       # raft.go:1591
    # raft.go:1593-1609 (the tracker, the config, the own Progress) is the host's
    n.promotable = False                                   # hasPendingSnapshot, raft.go:1618-1621
    return True, SNF_RESTORED


def handle_snapshot(n: Node, m: Snap) -> Tuple[int, int]:
    """raft.go:1518-1529 -> (the outcome's flag, the MsgAppResp's Index)."""
    ok, flag = restore(n, m)
    if ok:
        return flag, n.last_index                          # raft.go:1523
    return flag, n.committed                               # raft.go:1527


def new_stats() -> dict:
    return {k: 0 for k in SSTAT_NAMES}


def step(n: Node, m: Snap, st: dict):
    """raft.Step(MsgSnap).  Returns (sflags, resp) with resp = None or
    (type, term, index).  A record that stops leaves ``n`` untouched."""
    if m.term != 0 and m.term < n.term:                    # raft.go:883-919: ignored
        st["stale"] += 1
        return SNF_STALE, None
    t, s = copy.deepcopy(n), dict(st)
    hard0 = (n.term, n.vote, n.committed)
    f = 0
    if m.term != 0 and m.term > t.term:                    # raft.go:876-877
        f |= become_follower(t, m.term, m.frm, s)
    if t.state == LEADER:                                  # stepLeader: no case
        st["role_ignored"] += 1
        return SNF_ROLE_IGNORED, None
    if t.state in (CANDIDATE, PRE_CANDIDATE):              # raft.go:1396-1398
        f |= become_follower(t, m.term, m.frm, s)
    else:                                                  # raft.go:1441-1444
        t.election_elapsed = 0
        t.lead = m.frm
    try:
        flag, index = handle_snapshot(t, m)
    except Panic:
        st["commit_range"] += 1
        return SNF_COMMIT_RANGE, None
    f |= flag
    s[SSTAT_NAMES[flag.bit_length() - 1]] += 1
    t.pending |= RDP_MSGS                                  # r.send: len(r.msgs) > 0
    if (t.term, t.vote, t.committed) != hard0:
        f |= SNF_HARDSTATE
    n.__dict__.update(t.__dict__)
    st.update(s)
    return f, (MSG_APP_RESP, n.term, index)                # send: Term = r.Term


def snapshot_call(nodes: List[Node], recs: Sequence[Tuple[int, Snap]], st: Optional[dict] = None,
                  pending: bool = True):
    """qb_dev_follower_snapshot over ``nodes`` (in place): records (group,
    Snap) of distinct groups.  pending False: the call has no pending column
    (the nodes' stay as they are).  Returns a dict: sflags, resp_type,
    resp_term, resp_index [R], stats."""
    st = new_stats() if st is None else st
    G, R = len(nodes), len(recs)
    live = [g for g, _ in recs if 0 <= g < G]
    assert len(set(live)) == len(live), "the records of one call name distinct groups"
    out = {"sflags": [0] * R, "resp_type": [0] * R, "resp_term": [0] * R, "resp_index": [0] * R,
           "stats": st}
    for i, (g, m) in enumerate(recs):
        if not 0 <= g < G:
            st["bad_group"] += 1
            out["sflags"][i] = SNF_BAD_GROUP
            continue
        p0 = nodes[g].pending
        f, resp = step(nodes[g], m, st)
        if not pending:
            nodes[g].pending = p0
        out["sflags"][i] = f
        if resp is not None:
            out["resp_type"][i], out["resp_term"][i], out["resp_index"][i] = resp
    return out
