"""The batched proposal (include/quorum_batch.h ``qb_dev_leader_propose``).

Step(MsgProp) -> appendEntry -> bcastAppend (raft.go:1019-1077, 621-642,
1761-1779, 432-522) and the log's share of becomeLeader (raft.go:745-756)
for every group of a ``LeaderGroups`` table in one call.  It runs in the HIP
library over the table's own arrays, the follower step's (lead, last_term),
the tick's role bytes and a ``ProposeState`` (applied, uncommitted_size,
pending_conf_index); torch only holds device memory.  What stays the host's
per flag is in INTEGRATION.md.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import _lib
from ._checks import I32, I64, U8, check_tensors
from ._dev import stats_dict, stream_handle
from ._dev import to_dev as _to_dev, to_np as _to_np
from .campaign import ElectionState
from .leader import MAX_RUNS, LeaderGroups

PROP_NONE, PROP_ENTRIES, PROP_LEADER_ENTRY = 0, 1, 2
PROP_CONF_CHANGE, PROP_CC_LEAVE_JOINT = 0x40, 0x80
MSG_APP, MSG_SNAP = 3, 7
PFLAG_APPENDED, PFLAG_BCAST, PFLAG_COMMITTED, PFLAG_DROPPED = 0x01, 0x02, 0x04, 0x08
PFLAG_FORWARD, PFLAG_CC_REFUSED, PFLAG_LOG_RUNS, PFLAG_BAD = 0x10, 0x20, 0x40, 0x80
PSTAT_NAMES = ("proposals", "entries", "drop_no_progress", "drop_transfer", "drop_size",
               "drop_no_leader", "drop_forwarding", "drop_candidate", "forwarded", "cc_accepted",
               "cc_refused", "msg_app", "msg_snap", "commits", "leader_entries", "log_runs",
               "empty", "ignored_role", "bad_action")

_P = C.c_void_p
_POINTERS = ("off", "cfg", "role", "term", "lead", "first_index", "snap_index", "snap_term",
             "max_ents", "applied", "meta", "committed", "last_index", "last_term", "run_start",
             "run_term", "uncommitted_size", "pending_conf_index", "match", "next",
             "pending_snapshot", "pstate", "infl_pos", "infl_buf")
_IN_POINTERS = ("action", "n_ents", "payload", "cc_at", "cc_payload")
_OUT_POINTERS = ("pflags", "msg_type", "msg_index", "msg_log_term", "msg_n")


class ProposeGroupsC(C.Structure):
    """struct qb_propose_groups (include/quorum_batch.h)."""
    _fields_ = [("G", C.c_uint64), ("inflight_cap", C.c_uint32),
                ("disable_proposal_forwarding", C.c_uint32),
                ("max_uncommitted_size", C.c_uint64)] + [(n, _P) for n in _POINTERS]


class ProposeInC(C.Structure):
    """struct qb_propose_in."""
    _fields_ = [(n, _P) for n in _IN_POINTERS]


class ProposeOutC(C.Structure):
    """struct qb_propose_out."""
    _fields_ = [(n, _P) for n in _OUT_POINTERS]


@dataclass
class ProposeState:
    """What a proposing leader keeps beyond the table and the election state,
    device tensors of G u64 (int64 storage): ``applied`` (raftLog.applied,
    read only), ``uncommitted_size`` and ``pending_conf_index`` (in/out)."""
    applied: torch.Tensor
    uncommitted_size: torch.Tensor
    pending_conf_index: torch.Tensor

    @classmethod
    def from_numpy(cls, applied, uncommitted_size, pending_conf_index, device="cuda"):
        dev = torch.device(device)
        if not len(applied) == len(uncommitted_size) == len(pending_conf_index):
            raise _lib.QuorumBatchError("applied, uncommitted_size and pending_conf_index differ "
                                        "in length")
        return cls(_to_dev(applied, np.uint64, dev), _to_dev(uncommitted_size, np.uint64, dev),
                   _to_dev(pending_conf_index, np.uint64, dev))

    def numpy(self, G: int) -> Dict[str, np.ndarray]:
        return {"applied": _to_np(self.applied, np.uint64, G),
                "uncommitted_size": _to_np(self.uncommitted_size, np.uint64, G),
                "pending_conf_index": _to_np(self.pending_conf_index, np.uint64, G)}


@dataclass
class ProposeInbox:
    """One proposal per group (struct qb_propose_in), device tensors of G
    entries: ``action`` u8 (PROP_* | PROP_CONF_CHANGE | PROP_CC_LEAVE_JOINT),
    ``n_ents`` u32, ``payload`` u64, ``cc_at`` u32, ``cc_payload`` u64."""
    action: torch.Tensor
    n_ents: torch.Tensor
    payload: torch.Tensor
    cc_at: torch.Tensor
    cc_payload: torch.Tensor

    @classmethod
    def from_numpy(cls, action, n_ents, payload, cc_at=None, cc_payload=None, device="cuda"):
        dev = torch.device(device)
        G = len(action)
        cc_at = np.zeros(G, np.uint32) if cc_at is None else cc_at
        cc_payload = np.zeros(G, np.uint64) if cc_payload is None else cc_payload
        for k, a in (("n_ents", n_ents), ("payload", payload), ("cc_at", cc_at),
                     ("cc_payload", cc_payload)):
            if len(a) != G:
                raise _lib.QuorumBatchError(f"{k} has {len(a)} entries, action {G}")
        return cls(_to_dev(action, np.uint8, dev), _to_dev(n_ents, np.uint32, dev),
                   _to_dev(payload, np.uint64, dev), _to_dev(cc_at, np.uint32, dev),
                   _to_dev(cc_payload, np.uint64, dev))


@dataclass
class ProposeResult:
    """Device outputs of one propose call.  msg_type holds a value only in the
    slots of groups with PFLAG_BCAST, msg_index / msg_log_term / msg_n only
    where msg_type is non-zero; the rest keeps what the buffers held."""
    pflags: torch.Tensor        # [G] u8 PFLAG_*
    msg_type: torch.Tensor      # [S] u8: 0 / MSG_APP / MSG_SNAP
    msg_index: torch.Tensor     # [S] u64 (int64 storage)
    msg_log_term: torch.Tensor  # [S] u64
    msg_n: torch.Tensor         # [S] u64
    stats: torch.Tensor         # [len(PSTAT_NAMES)] u64, accumulated
    groups: Optional[LeaderGroups] = None

    def stats_dict(self) -> Dict[str, int]:
        return stats_dict(PSTAT_NAMES, self.stats)

    def messages(self, g: int) -> List[Tuple[int, int, int, int, int, int]]:
        """Group g's messages of this call as (type, to, index, log_term,
        commit, n), ascending slots as bcastAppend emits them: a MSG_APP
        carries n entries from index + 1 and Commit = the group's committed
        index after the call; a MSG_SNAP the snapshot's index and term.
        Empty unless the group's pflags has PFLAG_BCAST."""
        lg = self.groups
        if not 0 <= g < lg.G:
            raise IndexError(g)
        if not int(self.pflags[g].item()) & PFLAG_BCAST:
            return []
        off = _to_np(lg.t["off"][g:g + 2], np.uint32)
        lo, hi = int(off[0]), int(off[1])
        hi = min(hi, lo + _lib.QB_MAX_SLOTS)
        if hi <= lo:
            return []
        commit = int(_to_np(lg.t["committed"][g:g + 1], np.uint64)[0])
        mt = self.msg_type[lo:hi].cpu().numpy()
        idx = _to_np(self.msg_index[lo:hi], np.uint64)
        lt = _to_np(self.msg_log_term[lo:hi], np.uint64)
        n = _to_np(self.msg_n[lo:hi], np.uint64)
        return [(int(mt[k]), k, int(idx[k]), int(lt[k]), commit if mt[k] == MSG_APP else 0,
                 int(n[k])) for k in range(hi - lo) if mt[k]]


def leader_propose(groups: LeaderGroups, election: ElectionState, state: ProposeState,
                   inbox: ProposeInbox, *, max_uncommitted_size: int = 0,
                   disable_proposal_forwarding: bool = False, stream=None,
                   out: Optional[ProposeResult] = None) -> ProposeResult:
    """Apply one proposal per group (``inbox``) to every group, in place.
    ``max_uncommitted_size``: Config.MaxUncommittedEntriesSize, 0 = no limit.
    ``out``: a previous result whose buffers are reused (stats accumulate);
    else fresh zero-filled ones.  ``stream``: a torch stream or a raw
    hipStream_t; default the current stream."""
    G, S, dev, t = groups.G, groups.S, groups.device, groups.t
    fg = election.follower
    st, ft = fg.state, fg.t
    if fg.G != G:
        raise _lib.QuorumBatchError(f"the election state holds {fg.G} groups, the table {G}")
    if not 1 <= int(groups.inflight_cap) <= 4096:
        raise _lib.QuorumBatchError(f"inflight_cap must be 1..4096, got {groups.inflight_cap}")
    if not 0 <= int(max_uncommitted_size) < 1 << 64:
        raise _lib.QuorumBatchError(f"max_uncommitted_size must be a uint64, got "
                                    f"{max_uncommitted_size}")
    if out is None:
        n, s = max(G, 1), max(S, 1)
        out = ProposeResult(torch.zeros(n, dtype=torch.uint8, device=dev),
                            torch.zeros(s, dtype=torch.uint8, device=dev),
                            torch.zeros(s, dtype=torch.int64, device=dev),
                            torch.zeros(s, dtype=torch.int64, device=dev),
                            torch.zeros(s, dtype=torch.int64, device=dev),
                            torch.zeros(len(PSTAT_NAMES), dtype=torch.int64, device=dev))
    K = int(groups.inflight_cap)
    tensors = {"off": (t["off"], I32, G + 1), "cfg": (t["cfg"], I32, G),
               "role": (st.role, U8, G), "term": (ft["term"], I64, G), "lead": (ft["lead"], I64, G),
               "first_index": (t["first_index"], I64, G), "snap_index": (t["snap_index"], I64, G),
               "snap_term": (t["snap_term"], I64, G), "max_ents": (t["max_ents"], I64, G),
               "applied": (state.applied, I64, G), "meta": (t["meta"], I32, G),
               "committed": (ft["committed"], I64, G), "last_index": (ft["last_index"], I64, G),
               "last_term": (ft["last_term"], I64, G),
               "run_start": (t["run_start"], I64, MAX_RUNS * G),
               "run_term": (t["run_term"], I64, MAX_RUNS * G),
               "uncommitted_size": (state.uncommitted_size, I64, G),
               "pending_conf_index": (state.pending_conf_index, I64, G),
               "match": (t["match"], I64, S), "next": (t["next"], I64, S),
               "pending_snapshot": (t["pending_snapshot"], I64, S), "pstate": (t["pstate"], U8, S),
               "infl_pos": (t["infl_pos"], I32, S), "infl_buf": (t["infl_buf"], I64, S * K)}
    ins = {"action": (inbox.action, U8, G), "n_ents": (inbox.n_ents, I32, G),
           "payload": (inbox.payload, I64, G), "cc_at": (inbox.cc_at, I32, G),
           "cc_payload": (inbox.cc_payload, I64, G)}
    outs = {"pflags": (out.pflags, U8, G), "msg_type": (out.msg_type, U8, S),
            "msg_index": (out.msg_index, I64, S), "msg_log_term": (out.msg_log_term, I64, S),
            "msg_n": (out.msg_n, I64, S)}
    check_tensors(tuple((v[0], k, v[1], v[2]) for d in (tensors, ins, outs) for k, v in d.items()) +
                  ((out.stats, "stats", I64, len(PSTAT_NAMES)),))
    # the table's term / committed / last_index are the election state's
    # (ElectionState.for_table builds it so): one set of buffers
    for k in ("term", "committed", "last_index"):
        if ft[k].data_ptr() != t[k].data_ptr():
            raise _lib.QuorumBatchError(f"the election state's {k} is not the table's tensor")
    stream = stream_handle(dev, stream)
    pg = ProposeGroupsC(G=G, inflight_cap=K,
                        disable_proposal_forwarding=1 if disable_proposal_forwarding else 0,
                        max_uncommitted_size=int(max_uncommitted_size),
                        **{k: v[0].data_ptr() for k, v in tensors.items()})
    pin = ProposeInC(**{k: v[0].data_ptr() for k, v in ins.items()})
    pout = ProposeOutC(**{k: v[0].data_ptr() for k, v in outs.items()})
    _lib.call("qb_dev_leader_propose", C.byref(pg), C.byref(pin), C.byref(pout),
              out.stats.data_ptr(), stream)
    out.groups = groups
    return out
