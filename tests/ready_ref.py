"""CPU restatement of etcd's HasReady / Ready / Advance — TEST INFRASTRUCTURE
ONLY.

One RawNode's Ready cycle, statement by statement as Go has it.  Paths are
relative to the reference's ``raft/``:

  RawNode.Ready / readyWithoutAccept / acceptReady   rawnode.go:125-147
  RawNode.HasReady                                   rawnode.go:149-169
  RawNode.Advance                                    rawnode.go:172-179
  NewRawNode's prevSoftSt / prevHardSt               rawnode.go:52-53
  SoftState.equal                                    node.go:45-47
  isHardStateEqual / IsEmptyHardState / IsEmptySnap  node.go:92-104
  Ready.containsUpdates / appliedCursor              node.go:106-123
  newReady / MustSync                                node.go:564-595
  raft.advance                                       raft.go:543-580
  raft.reduceUncommittedSize                         raft.go:1783-1801
  raftLog.unstableEntries / nextEnts / hasNextEnts   log.go:173-201
  raftLog.hasPendingSnapshot                         log.go:203-205
  raftLog.appliedTo / stableTo / stableSnapTo        log.go:246-258
  raftLog.slice / mustCheckOutOfBounds               log.go:343-398
  unstable.maybeTerm / stableTo / stableSnapTo       log_unstable.go:55-113
  unstable.truncateAndAppend                         log_unstable.go:121-145

The log is a list of terms, one per index of [first_index - 1, last_index]
(the dummy entry first), so nothing here shares the kernels' run arithmetic;
the unstable entries are its tail from ``offset`` on.  The entries' bytes are
not modelled: a Ready carries index ranges, and the pagination of
CommittedEntries (limitSize) is the caller's, who passes the cursor it reached
to ``advance``.

Two things are the engine's, not Go's: a state Go panics on (or cannot
reach) is reported as RDF_BAD_LOG / AFLAG_APPLIED_RANGE instead of panicking,
and the automatic leave of a joint config is reported (AFLAG_AUTO_LEAVE)
instead of appended.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

U64 = (1 << 64) - 1
FOLLOWER, CANDIDATE, LEADER, PRE_CANDIDATE = 0, 1, 2, 3

RDF_SOFT, RDF_HARD, RDF_ENTRIES, RDF_SNAPSHOT, RDF_COMMITTED = 0x01, 0x02, 0x04, 0x08, 0x10
RDF_MSGS, RDF_READSTATES, RDF_MUST_SYNC, RDF_BAD_LOG, RDF_DEFERRED = 0x20, 0x40, 0x80, 0x100, 0x200
RDF_NAMES = ("soft", "hard", "entries", "snapshot", "committed", "msgs", "readstates",
             "must_sync", "bad_log", "deferred")
AFLAG_APPLIED_RANGE, AFLAG_AUTO_LEAVE, AFLAG_STABLE_STALE, AFLAG_BAD_GROUP = 0x01, 0x02, 0x04, 0x08
RSTAT_NAMES = RDF_NAMES + ("listed",)
ASTAT_NAMES = ("hardstate", "applied", "auto_leave", "stable", "stable_stale", "snap_stable",
               "applied_range", "bad_group")

HardState = Tuple[int, int, int]   # (Term, Vote, Commit)
SoftState = Tuple[int, int]        # (Lead, RaftState)
EMPTY_HS: HardState = (0, 0, 0)


class Panic(Exception):
    """logger.Panicf, or a slice bound Go's runtime panics on."""


@dataclass
class Node:
    """raft + raftLog + RawNode as the Ready cycle sees them."""
    term: int = 0
    vote: int = 0
    committed: int = 0
    lead: int = 0
    state: int = FOLLOWER
    promotable: bool = True          # not part of the SoftState
    first_index: int = 1             # raftLog.firstIndex()
    terms: List[int] = field(default_factory=lambda: [0])  # [first_index - 1 .. last_index]
    applied: int = 0
    offset: int = 1                  # unstable.offset
    snap: Optional[Tuple[int, int]] = None  # unstable.snapshot's (Index, Term)
    msgs: bool = False               # len(r.msgs) > 0
    read_states: bool = False        # len(r.readStates) != 0
    uncommitted_size: int = 0
    pending_conf_index: int = 0
    auto_leave: bool = False
    prev_soft: SoftState = (0, FOLLOWER)
    prev_hard: HardState = EMPTY_HS

    @property
    def last_index(self) -> int:
        return (self.first_index - 1 + len(self.terms) - 1) & U64

    @property
    def last_term(self) -> int:
        return self.terms[-1]

    def new_raw_node(self) -> "Node":
        """rawnode.go:52-53."""
        self.prev_soft = soft_state(self)
        self.prev_hard = hard_state(self)
        return self


@dataclass
class Ready:
    """node.go:52-90, with index ranges for the entry slices."""
    soft: Optional[SoftState] = None
    hard: HardState = EMPTY_HS
    entries: Optional[Tuple[int, int, int]] = None    # (first, last, last's term)
    committed: Optional[Tuple[int, int]] = None       # (first, last), not paginated
    snap_index: int = 0
    msgs: bool = False
    read_states: bool = False
    must_sync: bool = False


def soft_state(n: Node) -> SoftState:
    return (n.lead, n.state)


def hard_state(n: Node) -> HardState:
    return (n.term, n.vote, n.committed)


def is_empty_hard_state(st: HardState) -> bool:  # node.go:97-99
    return st == EMPTY_HS


def unstable_entries(n: Node) -> Optional[Tuple[int, int, int]]:
    """log.go:173-178: unstable.entries as (offset, last, last's term).  The
    slice has last + 1 - offset entries; fewer than none cannot exist."""
    if n.offset > (n.last_index + 1) & U64:
        raise Panic("unstable.offset past the log's end")
    if n.offset > n.last_index:  # len(l.unstable.entries) == 0
        return None
    return (n.offset, n.last_index, n.last_term)


def must_check_out_of_bounds(n: Node, lo: int, hi: int) -> None:
    """log.go:384-398."""
    if lo > hi:
        raise Panic(f"invalid slice {lo} > {hi}")
    fi = n.first_index
    if lo < fi:
        raise Panic("ErrCompacted")  # nextEnts panics on any error
    length = (n.last_index + 1 - fi) & U64
    if hi > (fi + length) & U64:
        raise Panic(f"slice[{lo},{hi}) out of bound [{fi},{n.last_index}]")


def has_next_ents(n: Node) -> bool:
    """log.go:197-201."""
    off = max((n.applied + 1) & U64, n.first_index)
    return (n.committed + 1) & U64 > off


def next_ents(n: Node) -> Optional[Tuple[int, int]]:
    """log.go:183-193 without limitSize: the range [off, committed]."""
    off = max((n.applied + 1) & U64, n.first_index)
    if (n.committed + 1) & U64 > off:
        must_check_out_of_bounds(n, off, (n.committed + 1) & U64)
        return (off, n.committed)
    return None


def has_pending_snapshot(n: Node) -> bool:
    """log.go:203-205."""
    return n.snap is not None and n.snap[0] != 0


def must_sync(st: HardState, prevst: HardState, entsnum: int) -> bool:
    """node.go:589-595."""
    return entsnum != 0 or st[1] != prevst[1] or st[0] != prevst[0]


def new_ready(n: Node) -> Ready:
    """node.go:564-584."""
    rd = Ready(entries=unstable_entries(n), committed=next_ents(n), msgs=n.msgs)
    if soft_state(n) != n.prev_soft:
        rd.soft = soft_state(n)
    if hard_state(n) != n.prev_hard:
        rd.hard = hard_state(n)
    if n.snap is not None:
        rd.snap_index = n.snap[0]
    if n.read_states:
        rd.read_states = True
    nents = 0 if rd.entries is None else (rd.entries[1] - rd.entries[0] + 1)
    rd.must_sync = must_sync(hard_state(n), n.prev_hard, nents)
    return rd


def contains_updates(rd: Ready) -> bool:
    """node.go:106-110."""
    return (rd.soft is not None or not is_empty_hard_state(rd.hard) or rd.snap_index != 0 or
            rd.entries is not None or rd.committed is not None or rd.msgs or rd.read_states)


def has_ready(n: Node) -> bool:
    """rawnode.go:149-169."""
    if soft_state(n) != n.prev_soft:
        return True
    hs = hard_state(n)
    if not is_empty_hard_state(hs) and hs != n.prev_hard:
        return True
    if has_pending_snapshot(n):
        return True
    if n.msgs or unstable_entries(n) is not None or has_next_ents(n):
        return True
    if n.read_states:
        return True
    return False


def accept_ready(n: Node, rd: Ready) -> None:
    """rawnode.go:139-147."""
    if rd.soft is not None:
        n.prev_soft = rd.soft
    if rd.read_states:
        n.read_states = False
    n.msgs = False


def ready_flags(n: Node) -> Tuple[int, Optional[Ready]]:
    """The engine's rflags of one node (without RDF_DEFERRED) and its Ready;
    RDF_BAD_LOG alone, and no Ready, where Go panics."""
    try:
        rd = new_ready(n)
    except Panic:
        return RDF_BAD_LOG, None
    f = 0
    if rd.soft is not None:
        f |= RDF_SOFT
    if not is_empty_hard_state(rd.hard):
        f |= RDF_HARD
    if rd.entries is not None:
        f |= RDF_ENTRIES
    if rd.snap_index != 0:
        f |= RDF_SNAPSHOT
    if rd.committed is not None:
        f |= RDF_COMMITTED
    if rd.msgs:
        f |= RDF_MSGS
    if rd.read_states:
        f |= RDF_READSTATES
    if rd.must_sync:
        f |= RDF_MUST_SYNC
    assert contains_updates(rd) == has_ready(n) == bool(f & ~RDF_MUST_SYNC)
    return f, rd


@dataclass
class ReadyRecord:
    """One record of the engine's list."""
    gid: int
    flags: int
    hs: HardState
    ent: Tuple[int, int, int]
    apply: Tuple[int, int]
    snap_index: int
    lead: int
    role: int


def ready_call(nodes: Sequence[Node], accept: bool, ready_cap: int):
    """qb_dev_ready over ``nodes``: (rflags, records, ready count, stats).
    Mutates the nodes only through accept_ready."""
    rflags: List[int] = []
    records: List[ReadyRecord] = []
    stats = dict.fromkeys(RSTAT_NAMES, 0)
    count = 0
    for g, n in enumerate(nodes):
        f, rd = ready_flags(n)
        for k, name in enumerate(RDF_NAMES[:9]):
            stats[name] += (f >> k) & 1
        if f & ~RDF_MUST_SYNC:
            if count >= ready_cap:
                f |= RDF_DEFERRED
                stats["deferred"] += 1
            else:
                stats["listed"] += 1
                if rd is None:
                    records.append(ReadyRecord(g, f, EMPTY_HS, (0, 0, 0), (0, 0), 0, n.lead, n.state))
                else:
                    records.append(ReadyRecord(
                        g, f, rd.hard if f & RDF_HARD else EMPTY_HS, rd.entries or (0, 0, 0),
                        rd.committed or (0, 0), rd.snap_index, n.lead, n.state))
                    if accept:
                        accept_ready(n, rd)
            count += 1
        rflags.append(f)
    return rflags, records, count, stats


@dataclass
class AdvanceRecord:
    """What the host hands back of one Ready (struct qb_advance_in)."""
    gid: int
    hs: HardState = EMPTY_HS
    applied_to: int = 0       # Ready.appliedCursor(), node.go:112-123
    applied_payload: int = 0  # sum of PayloadSize over rd.CommittedEntries
    stable_index: int = 0     # rd.Entries' last (Index, Term)
    stable_term: int = 0
    stable_snap: int = 0      # rd.Snapshot.Metadata.Index


def reduce_uncommitted_size(n: Node, s: int) -> None:
    """raft.go:1783-1801 given the entries' payload sum."""
    if n.uncommitted_size == 0:
        return
    if s > n.uncommitted_size:
        n.uncommitted_size = 0
    else:
        n.uncommitted_size -= s


def applied_to(n: Node, i: int) -> None:
    """log.go:246-254."""
    if i == 0:
        return
    if n.committed < i or i < n.applied:
        raise Panic(f"applied({i}) is out of range [prevApplied({n.applied}), committed({n.committed})]")
    n.applied = i


def maybe_term(n: Node, i: int) -> Tuple[int, bool]:
    """log_unstable.go:55-73."""
    if i < n.offset:
        if n.snap is not None and n.snap[0] == i:
            return n.snap[1], True
        return 0, False
    if n.offset > n.last_index:  # maybeLastIndex: no unstable entries
        return 0, False
    if i > n.last_index:
        return 0, False
    k = i - (n.first_index - 1)
    return (n.terms[k] if k >= 0 else 0), True


def stable_to(n: Node, i: int, t: int) -> bool:
    """log_unstable.go:77-89; True iff the offset moved."""
    gt, ok = maybe_term(n, i)
    if not ok:
        return False
    if gt == t and i >= n.offset:
        n.offset = (i + 1) & U64
        return True
    return False


def stable_snap_to(n: Node, i: int) -> bool:
    """log_unstable.go:109-113."""
    if n.snap is not None and n.snap[0] == i:
        n.snap = None
        return True
    return False


def advance(n: Node, rec: AdvanceRecord, stats: Optional[Dict[str, int]] = None) -> int:
    """RawNode.Advance (rawnode.go:172-179) + raft.advance (raft.go:543-580)
    given what the host hands back; returns the aflags."""
    st = stats if stats is not None else dict.fromkeys(ASTAT_NAMES, 0)
    # appliedTo's panic comes first in the engine: nothing is applied
    if rec.applied_to != 0 and (n.committed < rec.applied_to or rec.applied_to < n.applied):
        st["applied_range"] += 1
        return AFLAG_APPLIED_RANGE
    flags = 0
    if not is_empty_hard_state(rec.hs):
        n.prev_hard = rec.hs
        st["hardstate"] += 1
    reduce_uncommitted_size(n, rec.applied_payload)
    new_applied = rec.applied_to
    if new_applied > 0:
        old_applied = n.applied
        applied_to(n, new_applied)
        st["applied"] += 1
        if (n.auto_leave and old_applied <= n.pending_conf_index and
                new_applied >= n.pending_conf_index and n.state == LEADER):
            flags |= AFLAG_AUTO_LEAVE  # the append stays the host's
            st["auto_leave"] += 1
    if rec.stable_index != 0:  # len(rd.Entries) > 0
        if stable_to(n, rec.stable_index, rec.stable_term):
            st["stable"] += 1
        else:
            flags |= AFLAG_STABLE_STALE
            st["stable_stale"] += 1
    if rec.stable_snap != 0:  # !IsEmptySnap(rd.Snapshot)
        if stable_snap_to(n, rec.stable_snap):
            st["snap_stable"] += 1
    return flags


def advance_call(nodes: Sequence[Node], records: Sequence[AdvanceRecord]):
    """qb_dev_advance: (aflags, stats)."""
    stats = dict.fromkeys(ASTAT_NAMES, 0)
    aflags = []
    for rec in records:
        if rec.gid >= len(nodes):
            stats["bad_group"] += 1
            aflags.append(AFLAG_BAD_GROUP)
            continue
        aflags.append(advance(nodes[rec.gid], rec, stats))
    return aflags, stats


def record_of(r: ReadyRecord, applied_to_: Optional[int] = None, payload: int = 0) -> AdvanceRecord:
    """The AdvanceRecord of a Ready the host handled in full (or applied only
    up to ``applied_to_``): appliedCursor, the last entry, the snapshot."""
    cursor = r.apply[1] if r.flags & RDF_COMMITTED else r.snap_index
    if applied_to_ is not None:
        cursor = applied_to_
    return AdvanceRecord(r.gid, r.hs, cursor, payload, r.ent[1] if r.flags & RDF_ENTRIES else 0,
                         r.ent[2] if r.flags & RDF_ENTRIES else 0, r.snap_index)


def truncate_and_append(n: Node, after: int, new_terms: Sequence[int]) -> None:
    """raftLog.append's unstable.truncateAndAppend (log_unstable.go:121-145)
    for entries from index ``after`` on with terms ``new_terms``."""
    k = after - (n.first_index - 1)
    if after == (n.last_index + 1) & U64:
        n.terms.extend(new_terms)           # directly append
    elif after <= n.offset:
        n.offset = after                    # replace the unstable entries
        n.terms[k:] = list(new_terms)
    else:
        n.terms[k:] = list(new_terms)       # truncate to after, then append


def truncate_fold(nodes: Sequence[Node], group: Sequence[int], app_from: Sequence[int]) -> None:
    """qb_dev_unstable_truncate: offset := min(offset, after), which is what
    each of truncateAndAppend's three cases leaves."""
    for g, a in zip(group, app_from):
        if a != 0 and g < len(nodes):
            nodes[g].offset = min(nodes[g].offset, a)
