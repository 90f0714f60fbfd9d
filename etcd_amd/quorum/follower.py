"""The batched follower step (include/quorum_batch.h ``qb_dev_follower_step``).

raft.Step (raft.go:847-984) for the inbox of nodes that are not leading:
MsgHeartbeat, MsgVote / MsgPreVote and MsgTimeoutNow for every group of a
``FollowerGroups`` table in one call, each group's records in batch order.
The step runs in the HIP library; torch only holds device memory.  What stays
the host's per flag is in INTEGRATION.md.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Iterator, Optional

import numpy as np
import torch

from .. import _lib
from ._checks import I32, I64, U8, check_tensors
from ._dev import stats_dict, stream_handle
from ._dev import to_dev as _to_dev, to_np as _to_np
from .tick import TickState

FIN_HEARTBEAT, FIN_VOTE, FIN_PREVOTE, FIN_TIMEOUT_NOW, FIN_HOST = 0, 1, 2, 3, 4
FREC_FORCE = 0x80
MSG_APP_RESP, MSG_VOTE_RESP, MSG_HEARTBEAT_RESP, MSG_PREVOTE_RESP = 4, 6, 9, 18
FRESP_REJECT = 0x80
FFLAG_HOST_MSG, FFLAG_CAMPAIGN, FFLAG_COMMIT_RANGE = 0x01, 0x02, 0x04
FFLAG_RESET, FFLAG_HARDSTATE = 0x08, 0x10
NO_STOP = 0xFFFFFFFF
MAX_RECORDS = (1 << 32) - 2
FSTAT_NAMES = ("heartbeats", "granted", "rejected", "lease_dropped", "stale_ignored",
               "stale_answered", "role_ignored", "became_follower", "after_stop", "bad_group",
               "bad_kind")

_P = C.c_void_p
_U64_FIELDS = ("term", "vote", "lead", "committed", "last_index", "last_term")


class FollowerGroupsC(C.Structure):
    """struct qb_follower_groups (include/quorum_batch.h)."""
    _fields_ = [("G", C.c_uint64), ("election_timeout", C.c_uint32), ("check_quorum", C.c_uint32),
                ("pre_vote", C.c_uint32), ("reserved", C.c_uint32)] + [
        (n, _P) for n in _U64_FIELDS + ("role", "election_elapsed", "heartbeat_elapsed")]


class FollowerInboxC(C.Structure):
    """struct qb_follower_inbox."""
    _fields_ = [("M", C.c_uint64)] + [(n, _P) for n in ("group", "flags", "from", "term", "index",
                                                         "aux")]


@dataclass
class FollowerGroups:
    """Per-group state of G nodes, device tensors of G entries: term / vote /
    lead / committed (in/out) and last_index / last_term, u64 held as int64;
    ``state`` carries role and the two elapsed counters — the tick's own
    buffers, shared with ``leader_tick``."""
    G: int
    election_timeout: int
    check_quorum: bool
    pre_vote: bool
    t: Dict[str, torch.Tensor]
    state: TickState

    @classmethod
    def from_numpy(cls, arrays: Dict[str, np.ndarray], state: TickState, election_timeout: int,
                   check_quorum: bool, pre_vote: bool, device="cuda") -> "FollowerGroups":
        dev = torch.device(device)
        missing = [k for k in _U64_FIELDS if k not in arrays]
        if missing:
            raise _lib.QuorumBatchError(f"follower groups lack {', '.join(missing)}")
        G = len(arrays["term"])
        for k in _U64_FIELDS:
            if len(arrays[k]) != G:
                raise _lib.QuorumBatchError(f"{k} has {len(arrays[k])} entries, term has {G}")
        return cls(G, int(election_timeout), bool(check_quorum), bool(pre_vote),
                   {k: _to_dev(arrays[k], np.uint64, dev) for k in _U64_FIELDS}, state)

    @property
    def device(self) -> torch.device:
        return self.t["term"].device

    def numpy(self) -> Dict[str, np.ndarray]:
        out = {k: _to_np(self.t[k], np.uint64, self.G) for k in _U64_FIELDS}
        st = self.state.numpy(self.G)
        out.update({k: st[k] for k in ("role", "election_elapsed", "heartbeat_elapsed")})
        return out


@dataclass
class FollowerInbox:
    """A batch of messages to non-leaders in arrival order (SoA).  flags =
    FIN_* | FREC_FORCE; index = Index (votes) / Commit (heartbeat); aux =
    LogTerm (votes) / the 8-byte context id, 0 = empty (heartbeat)."""
    group: torch.Tensor
    flags: torch.Tensor
    frm: torch.Tensor
    term: torch.Tensor
    index: torch.Tensor
    aux: torch.Tensor
    _m: Optional[int] = None

    @classmethod
    def from_numpy(cls, group, flags, frm, term, index, aux, device="cuda") -> "FollowerInbox":
        dev = torch.device(device)
        m = len(group)
        for what, a in (("flags", flags), ("from", frm), ("term", term), ("index", index),
                        ("aux", aux)):
            if len(a) != m:
                raise _lib.QuorumBatchError(f"inbox {what} has {len(a)} entries, group has {m}")
        ib = cls(_to_dev(group, np.uint32, dev), _to_dev(flags, np.uint8, dev),
                 _to_dev(frm, np.uint64, dev), _to_dev(term, np.uint64, dev),
                 _to_dev(index, np.uint64, dev), _to_dev(aux, np.uint64, dev))
        ib._m = m
        return ib

    @property
    def M(self) -> int:
        return int(self.group.numel()) if self._m is None else self._m

    def check(self) -> None:
        m = self.M
        if not 0 <= m <= MAX_RECORDS:
            raise _lib.QuorumBatchError(f"inbox record count must be a non-negative integer <= "
                                        f"2^32 - 2, got {m}")
        check_tensors(((self.group, "inbox.group", I32, m), (self.flags, "inbox.flags", U8, m),
                       (self.frm, "inbox.from", I64, m), (self.term, "inbox.term", I64, m),
                       (self.index, "inbox.index", I64, m), (self.aux, "inbox.aux", I64, m)))


@dataclass
class FollowerResult:
    """Device outputs of one follower step; responses are record-aligned."""
    resp_type: torch.Tensor   # [M] u8: pb MessageType | FRESP_REJECT, 0 = no message
    resp_term: torch.Tensor   # [M] u64 (int64 storage)
    stop_at: torch.Tensor     # [G] u32 (int32 storage), NO_STOP = none
    gflags: torch.Tensor      # [G] u8 FFLAG_*
    stats: torch.Tensor       # [len(FSTAT_NAMES)] u64, accumulated
    workspace: torch.Tensor
    inbox: Optional[FollowerInbox] = None

    def stats_dict(self) -> Dict[str, int]:
        return stats_dict(FSTAT_NAMES, self.stats)

    def responses(self) -> Iterator[dict]:
        """The messages to send, in batch order — after the HardState of every
        group with FFLAG_HARDSTATE is persisted.  context: the heartbeat's
        context id for a MsgHeartbeatResp (raft.go:1515), else 0."""
        ib = self.inbox
        m = ib.M
        if m == 0:
            return
        rt = _to_np(self.resp_type, np.uint8, m)
        term = _to_np(self.resp_term, np.uint64, m)
        frm = _to_np(ib.frm, np.uint64, m)
        aux = _to_np(ib.aux, np.uint64, m)
        for i in np.flatnonzero(rt).tolist():
            ty = int(rt[i]) & 0x7F
            yield {"i": i, "type": ty, "to": int(frm[i]), "term": int(term[i]),
                   "reject": bool(rt[i] & FRESP_REJECT),
                   "context": int(aux[i]) if ty == MSG_HEARTBEAT_RESP else 0}


def follower_workspace_bytes(G: int, M: int) -> int:
    n = int(_lib.fn("qb_follower_workspace_bytes")(G, M))
    if n == 0:
        raise _lib.QuorumBatchError(f"no follower-step workspace for G={G}, M={M} (M <= 2^32 - 2)")
    return n


def follower_step(groups: FollowerGroups, inbox: FollowerInbox, stream=None, *,
                  out: Optional[FollowerResult] = None) -> FollowerResult:
    """Step ``inbox`` into ``groups`` in place.  ``out``: a previous result
    whose buffers are reused (stats accumulate) when they are large enough;
    else fresh ones.  ``stream``: a torch stream or a raw hipStream_t; default
    the current stream."""
    G, st, t = groups.G, groups.state, groups.t
    if not 1 <= int(groups.election_timeout) <= 0xFFFFFFFF:
        raise _lib.QuorumBatchError(f"election_timeout must be 1..2^32-1, got "
                                    f"{groups.election_timeout}")
    inbox.check()
    M = inbox.M
    group_specs = tuple((t[k], k, I64, G) for k in _U64_FIELDS) + (
        (st.role, "state.role", U8, G), (st.election_elapsed, "state.election_elapsed", I32, G),
        (st.heartbeat_elapsed, "state.heartbeat_elapsed", I32, G))
    check_tensors(group_specs + ((inbox.group, "inbox.group", I32, M),))
    dev = groups.device
    need = follower_workspace_bytes(G, M)
    if out is None:
        out = FollowerResult(torch.zeros(max(M, 1), dtype=torch.uint8, device=dev),
                             torch.zeros(max(M, 1), dtype=torch.int64, device=dev),
                             torch.zeros(max(G, 1), dtype=torch.int32, device=dev),
                             torch.zeros(max(G, 1), dtype=torch.uint8, device=dev),
                             torch.zeros(len(FSTAT_NAMES), dtype=torch.int64, device=dev),
                             torch.empty((need + 7) // 8, dtype=torch.int64, device=dev))
    check_tensors(group_specs[:1] + (
        (out.resp_type, "resp_type", U8, M), (out.resp_term, "resp_term", I64, M),
        (out.stop_at, "stop_at", I32, G), (out.gflags, "gflags", U8, G),
        (out.stats, "stats", I64, len(FSTAT_NAMES)),
        (out.workspace, "workspace", I64, (need + 7) // 8)))
    stream = stream_handle(dev, stream)
    fg = FollowerGroupsC(G=G, election_timeout=int(groups.election_timeout),
                         check_quorum=1 if groups.check_quorum else 0,
                         pre_vote=1 if groups.pre_vote else 0, reserved=0,
                         role=st.role.data_ptr(), election_elapsed=st.election_elapsed.data_ptr(),
                         heartbeat_elapsed=st.heartbeat_elapsed.data_ptr(),
                         **{k: t[k].data_ptr() for k in _U64_FIELDS})
    ib = FollowerInboxC(M=M, group=inbox.group.data_ptr(), flags=inbox.flags.data_ptr(),
                        term=inbox.term.data_ptr(), index=inbox.index.data_ptr(),
                        aux=inbox.aux.data_ptr())
    setattr(ib, "from", inbox.frm.data_ptr())
    _lib.call("qb_dev_follower_step", C.byref(fg), C.byref(ib), out.resp_type.data_ptr(),
              out.resp_term.data_ptr(), out.stop_at.data_ptr(), out.gflags.data_ptr(),
              out.stats.data_ptr(), out.workspace.data_ptr(), out.workspace.numel() * 8, stream)
    out.inbox = inbox
    return out
