"""Batched log compaction (include/quorum_batch.h ``qb_dev_log_compact``).

MemoryStorage.CreateSnapshot and Compact (storage.go:190-236) and etcdserver's
policy around them (server/etcdserver/server.go:1096-1117, 1993-2067) for
every group in one call: what the host runs behind FFLAG_LOG_RUNS and
PFLAG_LOG_RUNS.  The call runs in the HIP library over the tensors the other
calls' dataclasses already hold (``FollowerLog`` or the leader's table,
``ReadyState``, the leader's snap_index / snap_term); torch only holds device
memory.  The host's half behind each listed group is in INTEGRATION.md.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np
import torch

from .. import _lib
from ._checks import FLAG, I16, I32, I64, check_tensors
from ._dev import grow_workspace, stats_dict, stream_handle
from ._dev import to_np as _to_np
from .follower import MAX_RUNS, FollowerLog
from .leader import LeaderGroups
from .ready import MAX_GROUPS, ReadyState

CM_EXPLICIT, CM_TRIGGER = 0, 1
CMF_SNAPPED, CMF_COMPACTED, CMF_SNAP_OUT_OF_DATE, CMF_ALREADY_COMPACTED = 0x001, 0x002, 0x004, 0x008
CMF_OUT_OF_BOUND, CMF_PAST_APPLIED, CMF_HELD, CMF_PENDING_SNAPSHOT = 0x010, 0x020, 0x040, 0x080
CMF_BAD_LOG, CMF_DEFERRED = 0x100, 0x200
CMSTAT_NAMES = ("snapped", "compacted", "snap_out_of_date", "already_compacted", "out_of_bound",
                "past_applied", "held", "pending_snapshot", "bad_log", "deferred", "listed",
                "entries_dropped", "runs_dropped")

_P = C.c_void_p
_GROUP_FIELDS = ("first_index", "snap_index", "snap_term", "meta", "run_start", "run_term",
                 "last_index", "applied", "unstable_offset", "usnap_index")
_LIST = {"gid": (np.uint32, I32), "flags": (np.uint16, I16), "snap_index": (np.uint64, I64),
         "snap_term": (np.uint64, I64), "compact_index": (np.uint64, I64),
         "first_before": (np.uint64, I64)}
_TORCH = {np.uint16: torch.int16, np.uint32: torch.int32, np.uint64: torch.int64}


class CompactGroupsC(C.Structure):
    """struct qb_compact_groups (include/quorum_batch.h)."""
    _fields_ = [("G", C.c_uint64)] + [(n, _P) for n in _GROUP_FIELDS]


class CompactInC(C.Structure):
    """struct qb_compact_in."""
    _fields_ = [("mode", C.c_uint32), ("reserved", C.c_uint32), ("snap_at", _P), ("compact_at", _P),
                ("snapshot_count", C.c_uint64), ("catch_up_entries", C.c_uint64), ("force", _P),
                ("hold", _P)]


class CompactOutC(C.Structure):
    """struct qb_compact_out."""
    _fields_ = [("cmflags", _P)] + [(n, _P) for n in _LIST] + [("list_count", _P)]


@dataclass
class CompactRequest:
    """struct qb_compact_in.  Explicit mode: ``snap_at`` / ``compact_at`` [G]
    u64 device columns, 0 = none, either may be None.  Trigger mode: the two
    scalars and the byte columns ``force`` / ``hold`` [G], either may be
    None."""
    mode: int
    snap_at: Optional[torch.Tensor] = None
    compact_at: Optional[torch.Tensor] = None
    snapshot_count: int = 0
    catch_up_entries: int = 0
    force: Optional[torch.Tensor] = None
    hold: Optional[torch.Tensor] = None

    @classmethod
    def explicit(cls, snap_at: Optional[torch.Tensor] = None,
                 compact_at: Optional[torch.Tensor] = None) -> "CompactRequest":
        """CreateSnapshot(snap_at[g]) then Compact(compact_at[g])."""
        return cls(CM_EXPLICIT, snap_at=snap_at, compact_at=compact_at)

    @classmethod
    def trigger(cls, snapshot_count: int, catch_up_entries: int,
                force: Optional[torch.Tensor] = None,
                hold: Optional[torch.Tensor] = None) -> "CompactRequest":
        """etcdserver's triggerSnapshot with Cfg.SnapshotCount and
        Cfg.SnapshotCatchUpEntries."""
        return cls(CM_TRIGGER, snapshot_count=int(snapshot_count),
                   catch_up_entries=int(catch_up_entries), force=force, hold=hold)

    def check(self) -> None:
        """The mode and the scalars (``log_compact`` checks the columns)."""
        if self.mode not in (CM_EXPLICIT, CM_TRIGGER):
            raise _lib.QuorumBatchError(f"compact mode must be CM_EXPLICIT or CM_TRIGGER, got "
                                        f"{self.mode}")
        for what, v in (("snapshot_count", self.snapshot_count),
                        ("catch_up_entries", self.catch_up_entries)):
            if not 0 <= int(v) < 1 << 64:
                raise _lib.QuorumBatchError(f"{what} must be a uint64, got {v}")

    def struct(self) -> CompactInC:
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        return CompactInC(mode=self.mode, reserved=0, snap_at=p(self.snap_at),
                          compact_at=p(self.compact_at), snapshot_count=int(self.snapshot_count),
                          catch_up_entries=int(self.catch_up_entries), force=p(self.force),
                          hold=p(self.hold))


@dataclass
class CompactResult:
    """Device outputs of one call.  ``cmflags`` [G] holds every group's flags;
    the list columns hold records only below min(count, list_cap), the rest
    keeps what the buffers held."""
    G: int
    list_cap: int
    cmflags: torch.Tensor             # [G] u16 (int16 storage) CMF_*
    cols: Dict[str, torch.Tensor]     # the list, [list_cap] each
    list_count: torch.Tensor          # [1] u64
    stats: torch.Tensor               # [len(CMSTAT_NAMES)] u64, accumulated
    _ws: Optional[torch.Tensor] = field(default=None, repr=False)

    def count(self) -> int:
        """Groups that snapped or compacted, listed or deferred (waits for
        the stream)."""
        return int(self.list_count.cpu()[0])

    def listed(self) -> int:
        return min(self.count(), self.list_cap)

    def records(self) -> Dict[str, np.ndarray]:
        """The host's work list, in group order."""
        n = self.listed()
        return {k: _to_np(self.cols[k][:n], dt) for k, (dt, _) in _LIST.items()}

    def flags(self) -> np.ndarray:
        return _to_np(self.cmflags, np.uint16, self.G)

    def stats_dict(self) -> Dict[str, int]:
        return stats_dict(CMSTAT_NAMES, self.stats)


def new_compact_result(G: int, list_cap: int, device) -> CompactResult:
    """Fresh zero-filled output buffers."""
    z = lambda n, dt: torch.zeros(max(n, 1), dtype=_TORCH[dt], device=device)  # noqa: E731
    return CompactResult(int(G), int(list_cap), z(G, np.uint16),
                         {k: z(list_cap, dt) for k, (dt, _) in _LIST.items()},
                         z(1, np.uint64), z(len(CMSTAT_NAMES), np.uint64))


def leader_log(groups: LeaderGroups) -> FollowerLog:
    """The leader table's log columns as a ``FollowerLog`` over the same
    tensors (no copy): what ``log_compact`` takes for a leader."""
    t = groups.t
    return FollowerLog(groups.G, t["meta"], t["first_index"], t["run_start"], t["run_term"])


def log_compact(log: FollowerLog, ready: ReadyState, snap_index: torch.Tensor,
                snap_term: torch.Tensor, request: CompactRequest, *,
                list_cap: Optional[int] = None, out: Optional[CompactResult] = None,
                stream=None) -> CompactResult:
    """Snapshot and compact the logs in place.  The struct is built from the
    tensors the arguments hold, with the same pointers: meta / first_index /
    the run tables of ``log`` (a follower's, or ``leader_log(groups)``),
    last_index / applied / unstable_offset / usnap_index of ``ready``, and
    ``snap_index`` / ``snap_term`` [G] u64 (the leader table's columns).
    ``list_cap``: records the list holds (default G, or ``out``'s); acting
    groups past it are flagged CMF_DEFERRED and left as they are.  ``out``: a
    previous result whose buffers are reused (stats accumulate)."""
    G, r = log.G, ready.t
    if not 0 <= G <= MAX_GROUPS:
        raise _lib.QuorumBatchError(f"G must be 0..{MAX_GROUPS}, got {G}")
    if ready.G != G:
        raise _lib.QuorumBatchError(f"the log has {G} groups, the ready state {ready.G}")
    ptrs = {"first_index": log.first_index, "snap_index": snap_index, "snap_term": snap_term,
            "meta": log.meta, "run_start": log.run_start, "run_term": log.run_term,
            "last_index": r.get("last_index"), "applied": r.get("applied"),
            "unstable_offset": r.get("unstable_offset"), "usnap_index": r.get("usnap_index")}
    for k, v in ptrs.items():
        if v is None:
            raise _lib.QuorumBatchError(f"log_compact: {k} is missing")
    per = {"run_start": MAX_RUNS, "run_term": MAX_RUNS}
    check_tensors(tuple((ptrs[k], k, I32 if k == "meta" else I64, per.get(k, 1) * G)
                        for k in _GROUP_FIELDS))
    request.check()
    dev = log.first_index.device
    if out is None:
        out = new_compact_result(G, G if list_cap is None else int(list_cap), dev)
    elif list_cap is not None:
        out.list_cap = int(list_cap)
    cap = int(out.list_cap)
    if cap < 0:
        raise _lib.QuorumBatchError(f"list_cap must be non-negative, got {cap}")
    for k in _LIST:
        if out.cols.get(k) is None:
            raise _lib.QuorumBatchError(f"log_compact: the list column {k} is missing")
    check_tensors(((log.first_index, "first_index", I64, G), (out.cmflags, "cmflags", I16, G),
                   (out.list_count, "list_count", I64, 1),
                   (out.stats, "stats", I64, len(CMSTAT_NAMES)),
                   (request.snap_at, "snap_at", I64, G), (request.compact_at, "compact_at", I64, G),
                   (request.force, "force", FLAG, G), (request.hold, "hold", FLAG, G)) +
                  tuple((out.cols[k], k, dts, cap) for k, (_, dts) in _LIST.items()))
    need = int(_lib.fn("qb_log_compact_scratch_bytes")(G))
    out._ws = grow_workspace(out._ws, need, dev)
    out.G = G
    cg = CompactGroupsC(G=G, **{k: ptrs[k].data_ptr() for k in _GROUP_FIELDS})
    ci = request.struct()
    co = CompactOutC(cmflags=out.cmflags.data_ptr(), list_count=out.list_count.data_ptr(),
                     **{k: out.cols[k].data_ptr() for k in _LIST})
    _lib.call("qb_dev_log_compact", C.byref(cg), C.byref(ci), cap, C.byref(co),
              out.stats.data_ptr(), out._ws.data_ptr(), out._ws.numel(), stream_handle(dev, stream))
    return out


__all__ = ["CM_EXPLICIT", "CM_TRIGGER", "CMSTAT_NAMES", "CompactRequest", "CompactResult",
           "leader_log", "log_compact", "new_compact_result"]
