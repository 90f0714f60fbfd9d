"""qb_dev_log_compact restated by entries, not by runs: MemoryStorage as the
Go has it (storage.go:190-236) — a list of (index, term) with the dummy entry
first — etcdserver's trigger (server/etcdserver/server.go:1096-1117,
1993-2067) around it, and the engine's rules of include/quorum_batch.h ("Log
compaction") around both.  The term-run table is derived from the entry list
afterwards (``runs``), so the kernel's run arithmetic is checked against code
that has none.  Test infrastructure; nothing here is used by the product."""
from __future__ import annotations

import copy
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

M64 = (1 << 64) - 1
CM_EXPLICIT, CM_TRIGGER = 0, 1
SNAPPED, COMPACTED, SNAP_OUT_OF_DATE, ALREADY_COMPACTED = 0x001, 0x002, 0x004, 0x008
OUT_OF_BOUND, PAST_APPLIED, HELD, PENDING_SNAPSHOT = 0x010, 0x020, 0x040, 0x080
BAD_LOG, DEFERRED = 0x100, 0x200
FLAG_NAMES = ("snapped", "compacted", "snap_out_of_date", "already_compacted", "out_of_bound",
              "past_applied", "held", "pending_snapshot", "bad_log", "deferred")
STAT_NAMES = FLAG_NAMES + ("listed", "entries_dropped", "runs_dropped")
MAX_RUNS = 8


class ErrCompacted(Exception):
    pass


class ErrSnapOutOfDate(Exception):
    pass


class Panic(Exception):
    """getLogger().Panicf, or a slice index out of range."""


class MemoryStorage:
    """storage.go:46-56: ents[0] is the dummy entry at the snapshot's (or the
    last compaction's) index; snapshot is its Metadata's (Index, Term)."""

    def __init__(self, ents: Sequence[Tuple[int, int]], snap_index: int = 0, snap_term: int = 0):
        self.ents: List[Tuple[int, int]] = [tuple(e) for e in ents]
        self.snap_index, self.snap_term = snap_index, snap_term

    def last_index(self) -> int:          # storage.go:150-152
        return self.ents[0][0] + len(self.ents) - 1

    def first_index(self) -> int:         # storage.go:161-163
        return self.ents[0][0] + 1

    def create_snapshot(self, i: int) -> Tuple[int, int]:   # storage.go:194-213
        if i <= self.snap_index:
            raise ErrSnapOutOfDate
        offset = self.ents[0][0]
        if i > self.last_index():
            raise Panic(f"snapshot {i} is out of bound lastindex({self.last_index()})")
        if i < offset:                    # ms.ents[i-offset]: the uint64 wraps, the index panics
            raise Panic(f"index out of range [{(i - offset) & M64}]")
        self.snap_index, self.snap_term = i, self.ents[i - offset][1]
        return self.snap_index, self.snap_term

    def compact(self, compact_index: int) -> None:          # storage.go:218-236
        offset = self.ents[0][0]
        if compact_index <= offset:
            raise ErrCompacted
        if compact_index > self.last_index():
            raise Panic(f"compact {compact_index} is out of bound lastindex({self.last_index()})")
        i = compact_index - offset
        self.ents = [self.ents[i]] + self.ents[i + 1:]


def runs(ents: Sequence[Tuple[int, int]]) -> List[Tuple[int, int]]:
    """The term runs of an entry list as (start index, term)."""
    out: List[Tuple[int, int]] = []
    for idx, term in ents:
        if not out or out[-1][1] != term:
            out.append((idx, term))
    return out


@dataclass
class Node:
    """One group.  ``ents`` is the whole log, dummy entry first, through
    last_index; MemoryStorage holds its stable part, the entries below
    ``unstable_offset``.  ``first_zero`` packs first_index as 0 (a state the
    entry list cannot hold)."""
    ents: List[Tuple[int, int]]
    unstable_offset: int
    applied: int
    snap_index: int = 0
    snap_term: int = 0
    usnap_index: int = 0
    first_zero: bool = False

    @property
    def first_index(self) -> int:
        return 0 if self.first_zero else self.ents[0][0] + 1

    @property
    def last_index(self) -> int:
        return self.ents[0][0] + len(self.ents) - 1


@dataclass
class Request:
    """struct qb_compact_in over lists (None: a NULL column)."""
    mode: int
    snap_at: Optional[Sequence[int]] = None
    compact_at: Optional[Sequence[int]] = None
    snapshot_count: int = 0
    catch_up_entries: int = 0
    force: Optional[Sequence[int]] = None
    hold: Optional[Sequence[int]] = None


def _col(c, g):
    return 0 if c is None else int(c[g])


def _storage_of(n: Node) -> Tuple[MemoryStorage, List[Tuple[int, int]]]:
    off = n.ents[0][0]
    cut = n.unstable_offset - off          # stable: [off, unstable_offset - 1]
    return MemoryStorage(n.ents[:cut], n.snap_index, n.snap_term), list(n.ents[cut:])


def decide(n: Node, req: Request, g: int):
    """One group's outcome against a copy of its storage: (flags, the storage
    after, its unstable tail, the compaction index or 0).  Nothing of ``n``
    changes."""
    if req.mode == CM_EXPLICIT:
        s, c = _col(req.snap_at, g), _col(req.compact_at, g)
        do_snap, do_comp = s != 0, c != 0
    else:                                   # shouldSnapshot, server.go:1115-1117
        appl, snapi = n.applied, n.snap_index
        do_snap = do_comp = bool((_col(req.force, g) and appl != snapi) or
                                 ((appl - snapi) & M64) > req.snapshot_count)
        s = appl                            # server.go:1111
        c = appl - req.catch_up_entries if appl > req.catch_up_entries else 1   # server.go:2047-2051
    if not (do_snap or do_comp):
        return 0, None, None, 0
    off, stable_last = n.first_index - 1, n.unstable_offset - 1
    if n.first_index == 0 or stable_last < off or stable_last > n.last_index:
        return BAD_LOG, None, None, 0
    if n.usnap_index != 0:
        return PENDING_SNAPSHOT, None, None, 0
    ms, tail = _storage_of(n)
    f = 0
    if do_snap:
        try:
            ms.create_snapshot(s)
            if s > n.applied:               # the engine's rule; Go has already returned
                f |= PAST_APPLIED
            else:
                f |= SNAPPED
        except ErrSnapOutOfDate:
            f |= SNAP_OUT_OF_DATE
        except Panic:
            f |= OUT_OF_BOUND
        if req.mode == CM_TRIGGER:
            if not f & SNAPPED:
                do_comp = False             # snapshot()'s early return, server.go:2016-2023
            elif _col(req.hold, g):
                f |= HELD                   # server.go:2042-2045
                do_comp = False
    done = 0
    if do_comp:
        try:
            ms.compact(c)
            if c > n.applied:
                f |= PAST_APPLIED
            else:
                f |= COMPACTED
                done = c
        except ErrCompacted:
            f |= ALREADY_COMPACTED
        except Panic:
            f |= OUT_OF_BOUND
    if f & (OUT_OF_BOUND | PAST_APPLIED):   # Go would not have returned: nothing applied
        return f & ~(SNAPPED | COMPACTED), None, None, 0
    return f, ms, tail, done


def new_stats() -> Dict[str, int]:
    return {k: 0 for k in STAT_NAMES}


@dataclass
class Result:
    flags: List[int]
    records: List[dict] = field(default_factory=list)   # the list, in group order
    count: int = 0


def log_compact(nodes: List[Node], req: Request, list_cap: int, stats: Dict[str, int]) -> Result:
    """The call over ``nodes`` in place; ``stats`` accumulates."""
    res = Result([0] * len(nodes))
    for g, n in enumerate(nodes):
        f, ms, tail, c = decide(n, req, g)
        if f & (SNAPPED | COMPACTED):
            pos = res.count
            res.count += 1
            if pos >= list_cap:
                f |= DEFERRED
            else:
                first_before = n.first_index
                before = n.ents
                if f & SNAPPED:
                    n.snap_index, n.snap_term = ms.snap_index, ms.snap_term
                if f & COMPACTED:
                    n.ents = ms.ents + tail
                    stats["entries_dropped"] += len(before) - len(n.ents)
                    stats["runs_dropped"] += len(runs(before)) - len(runs(n.ents))
                res.records.append({"gid": g, "flags": f, "snap_index": n.snap_index,
                                    "snap_term": n.snap_term, "compact_index": c,
                                    "first_before": first_before})
                stats["listed"] += 1
        for b, name in enumerate(FLAG_NAMES):
            stats[name] += (f >> b) & 1
        res.flags[g] = f
    return res


def clone(nodes: List[Node]) -> List[Node]:
    return copy.deepcopy(nodes)
