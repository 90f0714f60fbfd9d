"""Batched HasReady / Ready / Advance (include/quorum_batch.h ``qb_dev_ready``,
``qb_dev_advance``, ``qb_dev_unstable_truncate``).

RawNode.HasReady, readyWithoutAccept, acceptReady and Advance
(rawnode.go:125-179; newReady node.go:564-595; raft.advance raft.go:543-580)
for every group in one call each: ``ready`` lists the groups with work as
dense records, ``advance`` takes the host's finished records back, and
``unstable_truncate`` folds a follower log step's ``app_from`` into the
unstable offsets.  They run in the HIP library over the step calls' own
arrays and a ``ReadyState``; torch only holds device memory.  What the host
does with each flag is in INTEGRATION.md.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, Mapping, Optional

import numpy as np
import torch

from .. import _lib
from ._checks import I16, I32, I64, U8, check_tensors
from ._dev import grow_workspace, stats_dict, stream_handle
from ._dev import to_dev as _to_dev, to_np as _to_np
from .leader import MAX_RUNS

RDF_SOFT, RDF_HARD, RDF_ENTRIES, RDF_SNAPSHOT, RDF_COMMITTED = 0x01, 0x02, 0x04, 0x08, 0x10
RDF_MSGS, RDF_READSTATES, RDF_MUST_SYNC, RDF_BAD_LOG, RDF_DEFERRED = 0x20, 0x40, 0x80, 0x100, 0x200
RDP_MSGS, RDP_READSTATES = 0x01, 0x02
AFLAG_APPLIED_RANGE, AFLAG_AUTO_LEAVE, AFLAG_STABLE_STALE, AFLAG_BAD_GROUP = 0x01, 0x02, 0x04, 0x08
ROLE_PROMOTABLE = 0x80
MAX_GROUPS = 0xFFFFFFFE
RSTAT_NAMES = ("soft", "hard", "entries", "snapshot", "committed", "msgs", "readstates",
               "must_sync", "bad_log", "deferred", "listed")
ASTAT_NAMES = ("hardstate", "applied", "auto_leave", "stable", "stable_stale", "snap_stable",
               "applied_range", "bad_group")

_P = C.c_void_p
# name -> (numpy dtype, accepted torch dtypes, entries per group)
SHARED = {"term": (np.uint64, I64, 1), "vote": (np.uint64, I64, 1),
          "committed": (np.uint64, I64, 1), "lead": (np.uint64, I64, 1),
          "role": (np.uint8, U8, 1), "first_index": (np.uint64, I64, 1),
          "last_index": (np.uint64, I64, 1), "last_term": (np.uint64, I64, 1),
          "meta": (np.uint32, I32, 1), "run_start": (np.uint64, I64, MAX_RUNS),
          "run_term": (np.uint64, I64, MAX_RUNS), "pending_conf_index": (np.uint64, I64, 1),
          "ext": (np.uint32, I32, 1)}
OWN = {"applied": (np.uint64, I64, 1), "unstable_offset": (np.uint64, I64, 1),
       "usnap_index": (np.uint64, I64, 1), "usnap_term": (np.uint64, I64, 1),
       "prev_term": (np.uint64, I64, 1), "prev_vote": (np.uint64, I64, 1),
       "prev_commit": (np.uint64, I64, 1), "prev_lead": (np.uint64, I64, 1),
       "prev_role": (np.uint8, U8, 1), "pending": (np.uint8, U8, 1),
       "uncommitted_size": (np.uint64, I64, 1)}
COLUMNS = {**SHARED, **OWN}
_LIST = {"ready_gid": (np.uint32, I32), "rd_flags": (np.uint16, I16), "hs_term": (np.uint64, I64),
         "hs_vote": (np.uint64, I64), "hs_commit": (np.uint64, I64), "ent_lo": (np.uint64, I64),
         "ent_hi": (np.uint64, I64), "ent_last_term": (np.uint64, I64),
         "apply_lo": (np.uint64, I64), "apply_hi": (np.uint64, I64),
         "snap_index": (np.uint64, I64), "lead": (np.uint64, I64), "role": (np.uint8, U8)}
_ADV = {"adv_gid": (np.uint32, I32), "hs_term": (np.uint64, I64), "hs_vote": (np.uint64, I64),
        "hs_commit": (np.uint64, I64), "applied_to": (np.uint64, I64),
        "applied_payload": (np.uint64, I64), "stable_index": (np.uint64, I64),
        "stable_term": (np.uint64, I64), "stable_snap": (np.uint64, I64)}
_TORCH = {np.uint8: torch.uint8, np.uint16: torch.int16, np.uint32: torch.int32,
          np.uint64: torch.int64}


class ReadyGroupsC(C.Structure):
    """struct qb_ready_groups (include/quorum_batch.h)."""
    _fields_ = [("G", C.c_uint64)] + [(n, _P) for n in COLUMNS]


class ReadyOutC(C.Structure):
    """struct qb_ready_out."""
    _fields_ = [("rflags", _P)] + [(n, _P) for n in _LIST] + [("ready_count", _P)]


class AdvanceInC(C.Structure):
    """struct qb_advance_in."""
    _fields_ = [(n, _P) for n in _ADV]


@dataclass
class ReadyState:
    """The columns of struct qb_ready_groups as device tensors in ``t``: the
    step calls' own tensors (``SHARED``; ``ext`` may be None) and the eleven
    this module owns (``OWN``)."""
    G: int
    t: Dict[str, Optional[torch.Tensor]]
    _ws: Optional[torch.Tensor] = field(default=None, repr=False)

    @property
    def device(self):
        return self.t["term"].device

    @classmethod
    def from_numpy(cls, arrays: Mapping[str, np.ndarray], device="cuda") -> "ReadyState":
        """Every column from host arrays (``ext`` optional)."""
        dev = torch.device(device)
        G = len(arrays["term"])
        t: Dict[str, Optional[torch.Tensor]] = {}
        for k, (dt, _, per) in COLUMNS.items():
            if k == "ext" and arrays.get("ext") is None:
                t[k] = None
                continue
            if k not in arrays:
                raise _lib.QuorumBatchError(f"ready state: {k} is missing")
            if len(arrays[k]) != per * G:
                raise _lib.QuorumBatchError(f"{k} has {len(arrays[k])} entries, want {per * G}")
            t[k] = _to_dev(arrays[k], dt, dev)
        return cls(G, t)

    @classmethod
    def new_raw_node(cls, shared: Mapping[str, Optional[torch.Tensor]], applied: torch.Tensor,
                     uncommitted_size: torch.Tensor, *,
                     unstable_offset: Optional[torch.Tensor] = None) -> "ReadyState":
        """NewRawNode (rawnode.go:47-55) over the step calls' tensors in
        ``shared``: prevSoftSt / prevHardSt start at the current state,
        nothing is pending, no snapshot, and (unless given) every entry is
        stable: unstable_offset = last_index + 1 (newLogWithSize,
        log.go:56-79)."""
        t = {k: shared.get(k) for k in SHARED}
        G = int(t["term"].numel()) if t["term"] is not None else 0
        t["applied"], t["uncommitted_size"] = applied, uncommitted_size
        t["unstable_offset"] = t["last_index"] + 1 if unstable_offset is None else unstable_offset
        for k in ("usnap_index", "usnap_term"):
            t[k] = torch.zeros_like(t["term"])
        for k, src in (("prev_term", "term"), ("prev_vote", "vote"), ("prev_commit", "committed"),
                       ("prev_lead", "lead")):
            t[k] = t[src].clone()
        t["prev_role"] = t["role"] & 0x7F
        t["pending"] = torch.zeros_like(t["role"])
        s = cls(G, t)
        s.check()
        return s

    def check(self) -> None:
        G = self.G
        if not 0 <= G <= MAX_GROUPS:
            raise _lib.QuorumBatchError(f"G must be 0..{MAX_GROUPS}, got {G}")
        specs = []
        for k, (_, dts, per) in COLUMNS.items():
            if self.t.get(k) is None and k != "ext":
                raise _lib.QuorumBatchError(f"ready state: {k} is missing")
            specs.append((self.t.get(k), k, dts, per * G))
        check_tensors(tuple(specs))

    def struct(self) -> ReadyGroupsC:
        self.check()
        return ReadyGroupsC(G=self.G, **{k: (self.t[k].data_ptr() if self.t[k] is not None else None)
                                         for k in COLUMNS})

    def numpy(self) -> Dict[str, np.ndarray]:
        return {k: _to_np(self.t[k], dt, per * self.G) for k, (dt, _, per) in COLUMNS.items()
                if self.t[k] is not None}


@dataclass
class ReadyResult:
    """Device outputs of one ready call.  ``rflags`` [G] holds every group's
    flags; the list columns hold records only below min(count, ready_cap),
    the rest keeps what the buffers held."""
    ready_cap: int
    rflags: torch.Tensor              # [G] u16 (int16 storage)
    cols: Dict[str, torch.Tensor]     # the list, [ready_cap] each
    ready_count: torch.Tensor         # [1] u64
    stats: torch.Tensor               # [len(RSTAT_NAMES)] u64, accumulated

    def count(self) -> int:
        """Ready groups, listed or deferred (waits for the stream)."""
        return int(self.ready_count.cpu()[0])

    def listed(self) -> int:
        return min(self.count(), self.ready_cap)

    def records(self) -> Dict[str, np.ndarray]:
        n = self.listed()
        return {k: _to_np(self.cols[k][:n], dt) for k, (dt, _) in _LIST.items()}

    def stats_dict(self) -> Dict[str, int]:
        return stats_dict(RSTAT_NAMES, self.stats)


def new_ready_result(G: int, ready_cap: int, device) -> ReadyResult:
    """Fresh zero-filled output buffers."""
    z = lambda n, dt: torch.zeros(max(n, 1), dtype=_TORCH[dt], device=device)  # noqa: E731
    return ReadyResult(int(ready_cap), z(G, np.uint16),
                       {k: z(ready_cap, dt) for k, (dt, _) in _LIST.items()},
                       z(1, np.uint64), z(len(RSTAT_NAMES), np.uint64))


def ready(state: ReadyState, *, accept: bool = True, ready_cap: Optional[int] = None,
          out: Optional[ReadyResult] = None, stream=None) -> ReadyResult:
    """HasReady + Ready for every group.  ``accept``: run acceptReady on the
    listed groups (False: read only).  ``ready_cap``: records the list holds
    (default G, or ``out``'s); ready groups past it are flagged RDF_DEFERRED.
    ``out``: a previous result whose buffers are reused (stats accumulate)."""
    G = state.G
    rg = state.struct()
    dev = state.device
    if out is None:
        out = new_ready_result(G, G if ready_cap is None else int(ready_cap), dev)
    elif ready_cap is not None:
        out.ready_cap = int(ready_cap)
    cap = int(out.ready_cap)
    if cap < 0:
        raise _lib.QuorumBatchError(f"ready_cap must be non-negative, got {cap}")
    check_tensors(((out.rflags, "rflags", I16, G), (out.ready_count, "ready_count", I64, 1),
                   (out.stats, "stats", I64, len(RSTAT_NAMES))) +
                  tuple((out.cols.get(k), k, dts, cap) for k, (_, dts) in _LIST.items()))
    for k in _LIST:
        if out.cols.get(k) is None:
            raise _lib.QuorumBatchError(f"ready: the list column {k} is missing")
    need = int(_lib.fn("qb_ready_scratch_bytes")(G))
    state._ws = grow_workspace(state._ws, need, dev)
    ro = ReadyOutC(rflags=out.rflags.data_ptr(), ready_count=out.ready_count.data_ptr(),
                   **{k: out.cols[k].data_ptr() for k in _LIST})
    _lib.call("qb_dev_ready", C.byref(rg), 1 if accept else 0, cap, C.byref(ro),
              out.stats.data_ptr(), state._ws.data_ptr(), state._ws.numel(),
              stream_handle(dev, stream))
    return out


@dataclass
class AdvanceRecords:
    """struct qb_advance_in: A dense records as device tensors in ``t``."""
    A: int
    t: Dict[str, torch.Tensor]

    @classmethod
    def from_numpy(cls, arrays: Mapping[str, np.ndarray], device="cuda") -> "AdvanceRecords":
        dev = torch.device(device)
        A = len(arrays["adv_gid"])
        t = {}
        for k, (dt, _) in _ADV.items():
            a = arrays.get(k)
            a = np.zeros(A, dt) if a is None else a
            if len(a) != A:
                raise _lib.QuorumBatchError(f"{k} has {len(a)} entries, adv_gid {A}")
            t[k] = _to_dev(a, dt, dev)
        return cls(A, t)


@dataclass
class AdvanceResult:
    aflags: torch.Tensor   # [A] u8 AFLAG_*
    stats: torch.Tensor    # [len(ASTAT_NAMES)] u64, accumulated

    def stats_dict(self) -> Dict[str, int]:
        return stats_dict(ASTAT_NAMES, self.stats)


def advance(state: ReadyState, records: AdvanceRecords, *, out: Optional[AdvanceResult] = None,
            stream=None) -> AdvanceResult:
    """Advance for the ``records.A`` groups the host finished, in place."""
    A = int(records.A)
    if A < 0:
        raise _lib.QuorumBatchError(f"A must be non-negative, got {A}")
    rg = state.struct()
    dev = state.device
    if out is None:
        out = AdvanceResult(torch.zeros(max(A, 1), dtype=torch.uint8, device=dev),
                            torch.zeros(len(ASTAT_NAMES), dtype=torch.int64, device=dev))
    for k in _ADV:
        if records.t.get(k) is None:
            raise _lib.QuorumBatchError(f"advance: the record column {k} is missing")
    check_tensors(tuple((records.t[k], k, dts, A) for k, (_, dts) in _ADV.items()) +
                  ((out.aflags, "aflags", U8, A), (out.stats, "stats", I64, len(ASTAT_NAMES))))
    ai = AdvanceInC(**{k: records.t[k].data_ptr() for k in _ADV})
    _lib.call("qb_dev_advance", C.byref(rg), A, C.byref(ai), out.aflags.data_ptr(),
              out.stats.data_ptr(), stream_handle(dev, stream))
    return out


def unstable_truncate(state: ReadyState, group: torch.Tensor, app_from: torch.Tensor, *,
                      M: Optional[int] = None, stream=None) -> None:
    """unstable_offset[group[i]] = min(it, app_from[i]) for every record with
    app_from[i] != 0: the follower log step's rec_group column and app_from
    output, after the step."""
    M = int(group.numel() if M is None else M)
    if M < 0:
        raise _lib.QuorumBatchError(f"M must be non-negative, got {M}")
    check_tensors(((group, "group", I32, M), (app_from, "app_from", I64, M),
                   (state.t.get("unstable_offset"), "unstable_offset", I64, state.G)))
    if state.t.get("unstable_offset") is None:
        raise _lib.QuorumBatchError("ready state: unstable_offset is missing")
    _lib.call("qb_dev_unstable_truncate", M, group.data_ptr(), app_from.data_ptr(), state.G,
              state.t["unstable_offset"].data_ptr(), stream_handle(state.device, stream))
