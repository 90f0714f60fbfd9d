"""The batched MsgSnap step (include/quorum_batch.h ``qb_dev_follower_snapshot``).

raft.Step for MsgSnap at nodes that are not leading — the term filter,
handleSnapshot and restore (raft.go:847-920, 1396-1398, 1441-1444, 1518-1614;
raftLog.restore log.go:336-340) — for R records of distinct groups in one
call.  The step runs in the HIP library over the tensors the other calls'
dataclasses already hold (``FollowerGroups``, ``FollowerLog``, ``ReadyState``)
and the nodes' own IDs; torch only holds device memory.  What stays the host's
behind each flag is in INTEGRATION.md.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, Iterator, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib
from ._checks import I16, I32, I64, U8, check_tensors
from ._dev import stats_dict, stream_handle
from ._dev import to_dev as _to_dev, to_np as _to_np
from .follower import MAX_RECORDS, MAX_RUNS, MSG_APP_RESP, FollowerGroups, FollowerLog
from .ready import MAX_GROUPS, RDP_MSGS, ReadyState

CS_VOTERS, CS_LEARNERS, CS_VOTERS_OUTGOING, CS_LEARNERS_NEXT = 0, 1, 2, 3
CS_LISTS = ("voters", "learners", "voters_outgoing", "learners_next")  # by CS_* value
SNF_RESTORED, SNF_FAST_FORWARD, SNF_OLD, SNF_NOT_MEMBER = 0x001, 0x002, 0x004, 0x008
SNF_STALE, SNF_ROLE_IGNORED, SNF_RESET, SNF_COMMIT_RANGE = 0x010, 0x020, 0x040, 0x080
SNF_BAD_GROUP, SNF_HARDSTATE = 0x100, 0x200
SSTAT_NAMES = ("restored", "fast_forward", "old", "not_member", "stale", "role_ignored",
               "became_follower", "commit_range", "bad_group")

_P = C.c_void_p
_GROUP_FIELDS = ("self_id", "term", "vote", "lead", "committed", "role", "election_elapsed",
                 "heartbeat_elapsed", "first_index", "last_index", "last_term", "meta", "run_start",
                 "run_term", "unstable_offset", "usnap_index", "usnap_term", "pending")
_RECORD = {"group": (np.uint32, I32), "from": (np.uint64, I64), "term": (np.uint64, I64),
           "snap_index": (np.uint64, I64), "snap_term": (np.uint64, I64)}


class SnapshotGroupsC(C.Structure):
    """struct qb_snapshot_groups (include/quorum_batch.h)."""
    _fields_ = [("G", C.c_uint64), ("election_timeout", C.c_uint32), ("check_quorum", C.c_uint32),
                ("pre_vote", C.c_uint32), ("reserved", C.c_uint32)] + [(n, _P) for n in _GROUP_FIELDS]


class SnapshotInboxC(C.Structure):
    """struct qb_snapshot_inbox."""
    _fields_ = [("R", C.c_uint64)] + [(n, _P) for n in tuple(_RECORD) + ("cs_off", "cs_id", "cs_set")] + [
        ("C", C.c_uint64)]


class SnapshotOutC(C.Structure):
    """struct qb_snapshot_out."""
    _fields_ = [(n, _P) for n in ("sflags", "resp_type", "resp_term", "resp_index")]


def pack_conf_states(conf_states: Sequence[Mapping]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """ConfStates as dicts in ``confchange.restore``'s shape (voters, learners,
    voters_outgoing, learners_next; auto_leave is not sent to the device) ->
    (cs_off [R + 1] u32, cs_id [C] u64, cs_set [C] u8)."""
    off = np.zeros(len(conf_states) + 1, np.uint32)
    ids: List[int] = []
    sets: List[int] = []
    for i, cs in enumerate(conf_states):
        for s, name in enumerate(CS_LISTS):
            for v in cs.get(name, ()):
                ids.append(int(v))
                sets.append(s)
        if len(ids) > 0xFFFFFFFF:
            raise _lib.QuorumBatchError("the ConfStates hold more than 2^32 - 1 IDs")
        off[i + 1] = len(ids)
    return off, np.array(ids, np.uint64), np.array(sets, np.uint8)


@dataclass
class SnapshotInbox:
    """R MsgSnap records (SoA) in ``t``: group, from, term, snap_index,
    snap_term [R], cs_off [R + 1], cs_id / cs_set [C].  ``conf_states`` keeps
    the host's dicts for ``restored_conf_states``; ``groups_host`` the groups,
    for the duplicate check."""
    R: int
    C: int
    t: Dict[str, torch.Tensor]
    conf_states: Optional[List[dict]] = field(default=None, repr=False)
    groups_host: Optional[np.ndarray] = field(default=None, repr=False)

    @classmethod
    def from_numpy(cls, group, frm, term, snap_index, snap_term, conf_states: Sequence[Mapping],
                   device="cuda") -> "SnapshotInbox":
        dev = torch.device(device)
        R = len(group)
        for what, a in (("from", frm), ("term", term), ("snap_index", snap_index),
                        ("snap_term", snap_term), ("conf_states", conf_states)):
            if len(a) != R:
                raise _lib.QuorumBatchError(f"inbox {what} has {len(a)} entries, group has {R}")
        off, ids, sets = pack_conf_states(conf_states)
        cols = {"group": group, "from": frm, "term": term, "snap_index": snap_index,
                "snap_term": snap_term}
        t = {k: _to_dev(cols[k], dt, dev) for k, (dt, _) in _RECORD.items()}
        t["cs_off"] = _to_dev(off, np.uint32, dev)
        t["cs_id"] = _to_dev(ids, np.uint64, dev)
        t["cs_set"] = _to_dev(sets, np.uint8, dev)
        return cls(R, len(ids), t, [dict(cs) for cs in conf_states],
                   np.asarray(group, np.uint32).copy())

    def check(self) -> None:
        R, Cn = self.R, self.C
        if not 0 <= R <= MAX_RECORDS:
            raise _lib.QuorumBatchError(f"inbox record count must be a non-negative integer <= "
                                        f"2^32 - 2, got {R}")
        if not 0 <= int(Cn) < 1 << 64:
            raise _lib.QuorumBatchError(f"C must be a uint64, got {Cn}")
        for k in tuple(_RECORD) + ("cs_off", "cs_id", "cs_set"):
            if self.t.get(k) is None:
                raise _lib.QuorumBatchError(f"snapshot inbox: {k} is missing")
        check_tensors(tuple((self.t[k], "inbox." + k, dts, R) for k, (_, dts) in _RECORD.items()) + (
            (self.t["cs_off"], "inbox.cs_off", I32, R + 1), (self.t["cs_id"], "inbox.cs_id", I64, Cn),
            (self.t["cs_set"], "inbox.cs_set", U8, Cn)))

    def check_distinct(self) -> None:
        """The records of one call name distinct groups."""
        g = self.groups_host if self.groups_host is not None else _to_np(
            self.t["group"], np.uint32, self.R)
        vals, counts = np.unique(g[:self.R], return_counts=True)
        if (counts > 1).any():
            raise _lib.QuorumBatchError(
                f"snapshot inbox: group {int(vals[counts > 1][0])} has more than one record; a "
                f"second snapshot for a group waits for the next call")


@dataclass
class SnapshotResult:
    """Device outputs of one call; every column is record-aligned."""
    sflags: torch.Tensor      # [R] u16 (int16 storage) SNF_*
    resp_type: torch.Tensor   # [R] u8: 0 or MSG_APP_RESP
    resp_term: torch.Tensor   # [R] u64 (int64 storage)
    resp_index: torch.Tensor  # [R] u64
    stats: torch.Tensor       # [len(SSTAT_NAMES)] u64, accumulated
    inbox: Optional[SnapshotInbox] = None

    def stats_dict(self) -> Dict[str, int]:
        return stats_dict(SSTAT_NAMES, self.stats)

    def flags(self) -> np.ndarray:
        return _to_np(self.sflags, np.uint16, self.inbox.R)

    def responses(self) -> Iterator[dict]:
        """The MsgAppResps to send, in record order — after the HardState of
        every record with SNF_HARDSTATE and the snapshot of every record with
        SNF_RESTORED are persisted."""
        ib = self.inbox
        R = ib.R
        if R == 0:
            return
        rt = _to_np(self.resp_type, np.uint8, R)
        term = _to_np(self.resp_term, np.uint64, R)
        index = _to_np(self.resp_index, np.uint64, R)
        frm = _to_np(ib.t["from"], np.uint64, R)
        group = _to_np(ib.t["group"], np.uint32, R)
        for i in np.flatnonzero(rt).tolist():
            yield {"i": i, "group": int(group[i]), "type": int(rt[i]), "to": int(frm[i]),
                   "term": int(term[i]), "index": int(index[i])}


def new_snapshot_result(R: int, device) -> SnapshotResult:
    """Fresh zero-filled output buffers."""
    n = max(R, 1)
    return SnapshotResult(torch.zeros(n, dtype=torch.int16, device=device),
                          torch.zeros(n, dtype=torch.uint8, device=device),
                          torch.zeros(n, dtype=torch.int64, device=device),
                          torch.zeros(n, dtype=torch.int64, device=device),
                          torch.zeros(len(SSTAT_NAMES), dtype=torch.int64, device=device))


def follower_snapshot(groups: FollowerGroups, log: FollowerLog, ready: ReadyState,
                      self_id: torch.Tensor, inbox: SnapshotInbox, *,
                      out: Optional[SnapshotResult] = None, check_distinct: bool = True,
                      stream=None) -> SnapshotResult:
    """Step ``inbox`` into ``groups``, ``log`` and ``ready`` in place.  The
    struct is built from the tensors those hold, with the same pointers:
    term / vote / lead / committed / last_index / last_term and the tick state
    of ``groups``, meta / first_index / the run tables of ``log``, and
    unstable_offset / usnap_index / usnap_term / pending of ``ready``
    (``pending`` may be None).  ``self_id``: [G] u64, the nodes' raft IDs.
    ``check_distinct``: refuse duplicate groups before the C call.  ``out``: a
    previous result whose buffers are reused (stats accumulate)."""
    G, st, t, r = groups.G, groups.state, groups.t, ready.t
    if not 0 <= G <= MAX_GROUPS:
        raise _lib.QuorumBatchError(f"G must be 0..{MAX_GROUPS}, got {G}")
    if log.G != G or ready.G != G:
        raise _lib.QuorumBatchError(f"the log has {log.G} groups, the ready state {ready.G}, "
                                    f"the groups {G}")
    if not 1 <= int(groups.election_timeout) <= 0xFFFFFFFF:
        raise _lib.QuorumBatchError(f"election_timeout must be 1..2^32-1, got "
                                    f"{groups.election_timeout}")
    if self_id is None:
        raise _lib.QuorumBatchError("self_id is missing")
    if check_distinct:  # (on the host's copy of the groups: before any device is needed)
        inbox.check_distinct()
    inbox.check()
    R = inbox.R
    for k in ("unstable_offset", "usnap_index", "usnap_term"):
        if r.get(k) is None:
            raise _lib.QuorumBatchError(f"ready state: {k} is missing")
    ptrs = {"self_id": self_id, "term": t["term"], "vote": t["vote"], "lead": t["lead"],
            "committed": t["committed"], "role": st.role, "election_elapsed": st.election_elapsed,
            "heartbeat_elapsed": st.heartbeat_elapsed, "first_index": log.first_index,
            "last_index": t["last_index"], "last_term": t["last_term"], "meta": log.meta,
            "run_start": log.run_start, "run_term": log.run_term,
            "unstable_offset": r["unstable_offset"], "usnap_index": r["usnap_index"],
            "usnap_term": r["usnap_term"], "pending": r.get("pending")}
    dts = {"role": U8, "election_elapsed": I32, "heartbeat_elapsed": I32, "meta": I32, "pending": U8}
    per = {"run_start": MAX_RUNS, "run_term": MAX_RUNS}
    check_tensors(tuple((ptrs[k], k, dts.get(k, I64), per.get(k, 1) * G) for k in _GROUP_FIELDS) +
                  ((inbox.t["group"], "inbox.group", I32, R),))
    dev = groups.device
    if out is None:
        out = new_snapshot_result(R, dev)
    check_tensors(((t["term"], "term", I64, G), (out.sflags, "sflags", I16, R),
                   (out.resp_type, "resp_type", U8, R), (out.resp_term, "resp_term", I64, R),
                   (out.resp_index, "resp_index", I64, R),
                   (out.stats, "stats", I64, len(SSTAT_NAMES))))
    sg = SnapshotGroupsC(G=G, election_timeout=int(groups.election_timeout),
                         check_quorum=1 if groups.check_quorum else 0,
                         pre_vote=1 if groups.pre_vote else 0, reserved=0,
                         **{k: (v.data_ptr() if v is not None else None) for k, v in ptrs.items()})
    ib = SnapshotInboxC(R=R, C=int(inbox.C), **{k: inbox.t[k].data_ptr() for k in inbox.t})
    so = SnapshotOutC(sflags=out.sflags.data_ptr(), resp_type=out.resp_type.data_ptr(),
                      resp_term=out.resp_term.data_ptr(), resp_index=out.resp_index.data_ptr())
    _lib.call("qb_dev_follower_snapshot", C.byref(sg), C.byref(ib), C.byref(so),
              out.stats.data_ptr(), stream_handle(dev, stream))
    out.inbox = inbox
    return out


def restored_conf_states(inbox: SnapshotInbox, sflags) -> Tuple[np.ndarray, List[dict]]:
    """What to pass to ``confchange.restore`` for the restored records: (their
    groups, their ConfStates as the inbox was given them), in record order;
    LastIndex is the record's snap_index.  ``sflags``: the result's flags (a
    tensor or an array)."""
    if inbox.conf_states is None:
        raise _lib.QuorumBatchError("the inbox was not built from ConfState dicts")
    f = _to_np(sflags, np.uint16, inbox.R) if isinstance(sflags, torch.Tensor) else np.asarray(
        sflags, np.uint16)[:inbox.R]
    idx = np.flatnonzero(f & SNF_RESTORED)
    g = inbox.groups_host if inbox.groups_host is not None else _to_np(
        inbox.t["group"], np.uint32, inbox.R)
    return g[idx].copy(), [inbox.conf_states[i] for i in idx.tolist()]


__all__ = ["SnapshotInbox", "SnapshotResult", "follower_snapshot", "new_snapshot_result",
           "pack_conf_states", "restored_conf_states", "MSG_APP_RESP", "RDP_MSGS"]
