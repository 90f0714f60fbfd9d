"""The batched raft tick (include/quorum_batch.h ``qb_dev_leader_tick``).

raft.tick() for every group of a ``LeaderGroups`` table in one call:
tickElection / tickHeartbeat (raft.go:645-684), the MsgBeat broadcast and the
MsgCheckQuorum sweep of stepLeader (raft.go:994-1018).  The tick runs in the
HIP library over the table's own arrays (off, cfg, meta, committed, match,
pstate, rq_ctx) and the per-group ``TickState``; torch only holds device
memory.  What stays the host's per flag is in INTEGRATION.md.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch

from .. import _lib
from ._checks import I32, I64, U8, check_tensors
from ._dev import stats_dict, stream_handle
from ._dev import to_dev as _to_dev, to_np as _to_np
from .leader import MAX_READQ, LeaderGroups

MSG_HEARTBEAT = 8
ROLE_FOLLOWER, ROLE_CANDIDATE, ROLE_LEADER, ROLE_PRE_CANDIDATE = 0, 1, 2, 3
ROLE_PROMOTABLE = 0x80
TFLAG_HUP, TFLAG_BEAT, TFLAG_STEPPED_DOWN = 0x01, 0x02, 0x04
TFLAG_CHECK_QUORUM, TFLAG_TRANSFER_ABORTED = 0x08, 0x10
TSTAT_NAMES = ("leaders", "non_leaders", "beats", "heartbeats", "check_quorum", "stepped_down",
               "transfer_aborted", "hups")

_P = C.c_void_p


class TickGroupsC(C.Structure):
    """struct qb_tick_groups (include/quorum_batch.h)."""
    _fields_ = [("G", C.c_uint64), ("readq_cap", C.c_uint32), ("election_timeout", C.c_uint32),
                ("heartbeat_timeout", C.c_uint32), ("check_quorum", C.c_uint32)] + [
        (n, _P) for n in ("off", "cfg", "meta", "committed", "match", "pstate", "rq_ctx", "role",
                          "election_elapsed", "heartbeat_elapsed", "rand_timeout")]


@dataclass
class TickState:
    """The tick's own per-group state, device tensors of G entries: role u8
    (StateType | ROLE_PROMOTABLE), election_elapsed / heartbeat_elapsed /
    rand_timeout u32 (held as int32)."""
    role: torch.Tensor
    election_elapsed: torch.Tensor
    heartbeat_elapsed: torch.Tensor
    rand_timeout: torch.Tensor

    @classmethod
    def from_numpy(cls, role, election_elapsed, heartbeat_elapsed, rand_timeout, device="cuda"):
        dev = torch.device(device)
        return cls(_to_dev(role, np.uint8, dev), _to_dev(election_elapsed, np.uint32, dev),
                   _to_dev(heartbeat_elapsed, np.uint32, dev), _to_dev(rand_timeout, np.uint32, dev))

    def numpy(self, G: int) -> Dict[str, np.ndarray]:
        return {"role": _to_np(self.role, np.uint8, G),
                "election_elapsed": _to_np(self.election_elapsed, np.uint32, G),
                "heartbeat_elapsed": _to_np(self.heartbeat_elapsed, np.uint32, G),
                "rand_timeout": _to_np(self.rand_timeout, np.uint32, G)}


@dataclass
class TickResult:
    """Device outputs of one tick.  hb_commit [S] / hb_ctx [G] hold a value
    only where a heartbeat was sent (tflags & TFLAG_BEAT, every slot of the
    group but the leader's); the rest keeps what the buffers held."""
    tflags: torch.Tensor     # [G] u8
    hb_commit: torch.Tensor  # [S] u64 (int64 storage)
    hb_ctx: torch.Tensor     # [G] u64
    stats: torch.Tensor      # [8] u64, accumulated
    groups: LeaderGroups

    def stats_dict(self) -> Dict[str, int]:
        return stats_dict(TSTAT_NAMES, self.stats)

    def heartbeats(self, g: int) -> List[dict]:
        """Group g's MsgHeartbeats of this tick, in the order the reference
        emits them (ProgressTracker.Visit: ascending slots), as dicts with the
        leader step's message fields; empty unless the group beat."""
        lg = self.groups
        if not 0 <= g < lg.G:
            raise IndexError(g)
        if not int(self.tflags[g].item()) & TFLAG_BEAT:
            return []
        s0, s1 = (int(x) for x in _to_np(lg.t["off"][g:g + 2], np.uint32))
        s1 = min(s1, s0 + _lib.QB_MAX_SLOTS)
        lead = int(_to_np(lg.t["meta"][g:g + 1], np.uint32)[0]) & 0xFF
        commit = _to_np(self.hb_commit[s0:s1], np.uint64) if s1 > s0 else ()
        ctx = int(_to_np(self.hb_ctx[g:g + 1], np.uint64)[0])
        return [{"type": MSG_HEARTBEAT, "to": k, "index": 0, "log_term": 0,
                 "commit": int(commit[k]), "aux": ctx}
                for k in range(s1 - s0) if k != lead]


def leader_tick(groups: LeaderGroups, state: TickState, election_timeout: int,
                heartbeat_timeout: int, check_quorum: bool, stream=None, *,
                out: Optional[TickResult] = None) -> TickResult:
    """One raft.tick() over every group of ``groups``, in place (meta's
    transferee, pstate's RecentActive bits, ``state``).  ``out``: a previous
    result whose buffers are reused (stats accumulate); else fresh ones
    (hb_commit / hb_ctx zero-filled).  ``stream``: a torch stream or a raw
    hipStream_t; default the current stream."""
    G, S, dev = groups.G, groups.S, groups.device
    t = groups.t
    if not 0 <= groups.readq_cap <= MAX_READQ:
        raise _lib.QuorumBatchError(f"readq_cap must be 0..{MAX_READQ}, got {groups.readq_cap}")
    for what, v in (("election_timeout", election_timeout), ("heartbeat_timeout", heartbeat_timeout)):
        if not 1 <= int(v) <= 0xFFFFFFFF:
            raise _lib.QuorumBatchError(f"{what} must be 1..2^32-1, got {v}")
    if out is None:
        out = TickResult(torch.zeros(max(G, 1), dtype=torch.uint8, device=dev),
                         torch.zeros(max(S, 1), dtype=torch.int64, device=dev),
                         torch.zeros(max(G, 1), dtype=torch.int64, device=dev),
                         torch.zeros(len(TSTAT_NAMES), dtype=torch.int64, device=dev), groups)
    check_tensors(((t["off"], "off", I32, G + 1), (t["cfg"], "cfg", I32, G),
                   (t["meta"], "meta", I32, G), (t["committed"], "committed", I64, G),
                   (t["match"], "match", I64, S), (t["pstate"], "pstate", U8, S),
                   (t["rq_ctx"], "rq_ctx", I64, G * groups.readq_cap),
                   (state.role, "state.role", U8, G),
                   (state.election_elapsed, "state.election_elapsed", I32, G),
                   (state.heartbeat_elapsed, "state.heartbeat_elapsed", I32, G),
                   (state.rand_timeout, "state.rand_timeout", I32, G),
                   (out.tflags, "tflags", U8, G), (out.hb_commit, "hb_commit", I64, S),
                   (out.hb_ctx, "hb_ctx", I64, G), (out.stats, "stats", I64, len(TSTAT_NAMES))))
    stream = stream_handle(dev, stream)
    tg = TickGroupsC(G=G, readq_cap=groups.readq_cap, election_timeout=int(election_timeout),
                     heartbeat_timeout=int(heartbeat_timeout), check_quorum=1 if check_quorum else 0,
                     off=t["off"].data_ptr(), cfg=t["cfg"].data_ptr(), meta=t["meta"].data_ptr(),
                     committed=t["committed"].data_ptr(), match=t["match"].data_ptr(),
                     pstate=t["pstate"].data_ptr(),
                     rq_ctx=t["rq_ctx"].data_ptr() if groups.readq_cap else None,
                     role=state.role.data_ptr(),
                     election_elapsed=state.election_elapsed.data_ptr(),
                     heartbeat_elapsed=state.heartbeat_elapsed.data_ptr(),
                     rand_timeout=state.rand_timeout.data_ptr())
    _lib.call("qb_dev_leader_tick", C.byref(tg), out.tflags.data_ptr(), out.hb_commit.data_ptr(),
              out.hb_ctx.data_ptr(), out.stats.data_ptr(), stream)
    out.groups = groups
    return out
