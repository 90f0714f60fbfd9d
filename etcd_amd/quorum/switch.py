"""The batched switchToConfig (include/quorum_batch.h ``qb_dev_switch_config``).

raft.switchToConfig (raft.go:1651-1700) for every group of a ``LeaderGroups``
table in one call: the tail of applyConfChange behind ``ConfigTable.change``
and the tail of restore behind ``follower_snapshot``.  It renumbers every
slot-encoded word (the own slot, the transferee, the pending reads, the
votes), runs maybeCommit under the new quorum, bcastAppend or the immediate
probe of every member, and aborts a transfer to a removed or demoted member.
It runs in the HIP library over the new ``ConfigTable``'s arrays and the
table's per-group words; torch only holds device memory.  What stays the
host's per flag is in INTEGRATION.md.
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
from ._dev import to_np as _to_np
from .campaign import ElectionState
from .confchange import ConfigTable
from .leader import MAX_READQ, MAX_RUNS, LeaderGroups

SW_NONE, SW_SWITCH, SW_RESTORE = 0, 1, 2
MSG_APP, MSG_SNAP = 3, 7
SWFLAG_SWITCHED, SWFLAG_COMMITTED, SWFLAG_SENT, SWFLAG_TRANSFER_ABORTED = 0x01, 0x02, 0x04, 0x08
SWFLAG_SELF_REMOVED, SWFLAG_SELF_LEARNER, SWFLAG_VOTE_DROPPED, SWFLAG_HOST = 0x10, 0x20, 0x40, 0x80
SWSTAT_NAMES = ("switched", "restores", "commits", "bcast", "probed", "msg_app", "msg_snap",
                "transfer_aborted", "self_removed", "self_learner", "vote_dropped", "host",
                "bad_action")

_P = C.c_void_p
_POINTERS = ("old_off", "old_ids", "off", "ids", "cfg", "self_id", "role", "term", "first_index",
             "last_index", "last_term", "snap_index", "snap_term", "max_ents", "run_start",
             "run_term", "meta", "committed", "votes", "rq_meta", "match", "next",
             "pending_snapshot", "pstate", "infl_pos", "infl_buf")
_OUT_POINTERS = ("swflags", "slot_map", "msg_type", "msg_index", "msg_log_term", "msg_n")
# what the table takes over from the new config
_ADOPTED = ("off", "cfg", "match", "next", "pending_snapshot", "pstate", "infl_pos", "infl_buf")


class SwitchGroupsC(C.Structure):
    """struct qb_switch_groups (include/quorum_batch.h)."""
    _fields_ = [("G", C.c_uint64), ("inflight_cap", C.c_uint32), ("readq_cap", C.c_uint32)] + [
        (n, _P) for n in _POINTERS]


class SwitchOutC(C.Structure):
    """struct qb_switch_out."""
    _fields_ = [(n, _P) for n in _OUT_POINTERS]


@dataclass
class SwitchResult:
    """Device outputs of one switch call.  slot_map holds a value only in the
    old slots of groups with SWFLAG_SWITCHED, msg_type only in the new slots
    of groups with SWFLAG_SENT, msg_index / msg_log_term / msg_n only where
    msg_type is non-zero; the rest keeps what the buffers held."""
    swflags: torch.Tensor       # [G] u8 SWFLAG_*
    slot_map: torch.Tensor      # [S_old] u8: new slot, 0xFF = removed
    msg_type: torch.Tensor      # [S] u8: 0 / MSG_APP / MSG_SNAP
    msg_index: torch.Tensor     # [S] u64 (int64 storage)
    msg_log_term: torch.Tensor  # [S] u64
    msg_n: torch.Tensor         # [S] u64
    stats: torch.Tensor         # [len(SWSTAT_NAMES)] u64, accumulated
    groups: Optional[LeaderGroups] = None
    table: Optional[ConfigTable] = None   # the new config the messages' slots index

    def stats_dict(self) -> Dict[str, int]:
        return stats_dict(SWSTAT_NAMES, self.stats)

    def messages(self, g: int) -> List[Tuple[int, int, int, int, int, int]]:
        """Group g's messages of this call as (type, to, index, log_term,
        commit, n) over the new slots, ascending as Visit emits them; empty
        unless the group's swflags has SWFLAG_SENT."""
        lg = self.groups
        if not 0 <= g < lg.G:
            raise IndexError(g)
        if not int(self.swflags[g].item()) & SWFLAG_SENT:
            return []
        off = _to_np(self.table.t["off"][g:g + 2], np.uint32)
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


def switch_args(groups: LeaderGroups, election: ElectionState, old: ConfigTable,
                new: ConfigTable, action: torch.Tensor, out: Optional[SwitchResult] = None):
    """The checked argument blocks of one call: (qb_switch_groups,
    qb_switch_out, the SwitchResult whose buffers they name).  Every tensor's
    device, dtype, contiguity and length is checked here, before any pointer
    reaches the library."""
    G, dev, t = groups.G, groups.device, groups.t
    fg = election.follower
    st, ft = fg.state, fg.t
    if fg.G != G:
        raise _lib.QuorumBatchError(f"the election state holds {fg.G} groups, the table {G}")
    if old.G != G or new.G != G:
        raise _lib.QuorumBatchError(f"the configs hold {old.G} / {new.G} groups, the table {G}")
    K, Q = int(groups.inflight_cap), int(groups.readq_cap)
    if not 1 <= K <= 4096:
        raise _lib.QuorumBatchError(f"inflight_cap must be 1..4096, got {groups.inflight_cap}")
    if int(new.inflight_cap) != K:
        raise _lib.QuorumBatchError(f"the new config's rings hold {new.inflight_cap} entries, "
                                    f"the table's {K}")
    if not 0 <= Q <= MAX_READQ:
        raise _lib.QuorumBatchError(f"readq_cap must be 0..{MAX_READQ}, got {groups.readq_cap}")
    S0, S = int(old.S), int(new.S)
    if out is None:
        n, s = max(G, 1), max(S, 1)
        out = SwitchResult(torch.zeros(n, dtype=torch.uint8, device=dev),
                           torch.zeros(max(S0, 1), dtype=torch.uint8, device=dev),
                           torch.zeros(s, dtype=torch.uint8, device=dev),
                           torch.zeros(s, dtype=torch.int64, device=dev),
                           torch.zeros(s, dtype=torch.int64, device=dev),
                           torch.zeros(s, dtype=torch.int64, device=dev),
                           torch.zeros(len(SWSTAT_NAMES), dtype=torch.int64, device=dev))
    nt = new.t
    tensors = {"old_off": (old.t["off"], I32, G + 1), "old_ids": (old.t["ids"], I64, S0),
               "off": (nt["off"], I32, G + 1), "ids": (nt["ids"], I64, S), "cfg": (nt["cfg"], I32, G),
               "self_id": (election.self_id, I64, G), "role": (st.role, U8, G),
               "term": (ft["term"], I64, G), "first_index": (t["first_index"], I64, G),
               "last_index": (ft["last_index"], I64, G), "last_term": (ft["last_term"], I64, G),
               "snap_index": (t["snap_index"], I64, G), "snap_term": (t["snap_term"], I64, G),
               "max_ents": (t["max_ents"], I64, G),
               "run_start": (t["run_start"], I64, MAX_RUNS * G),
               "run_term": (t["run_term"], I64, MAX_RUNS * G), "meta": (t["meta"], I32, G),
               "committed": (ft["committed"], I64, G), "votes": (election.votes, I32, G),
               "rq_meta": (t["rq_meta"] if Q else None, I32, G * Q),
               "match": (nt["match"], I64, S), "next": (nt["next"], I64, S),
               "pending_snapshot": (nt["pending_snapshot"], I64, S), "pstate": (nt["pstate"], U8, S),
               "infl_pos": (nt["infl_pos"], I32, S), "infl_buf": (nt["infl_buf"], I64, S * K)}
    outs = {"swflags": (out.swflags, U8, G), "slot_map": (out.slot_map, U8, S0),
            "msg_type": (out.msg_type, U8, S), "msg_index": (out.msg_index, I64, S),
            "msg_log_term": (out.msg_log_term, I64, S), "msg_n": (out.msg_n, I64, S)}
    check_tensors(tuple((v[0], k, v[1], v[2]) for d in (tensors, outs) for k, v in d.items()) +
                  ((action, "action", U8, G), (out.stats, "stats", I64, len(SWSTAT_NAMES))))
    for k in ("term", "committed", "last_index"):
        if ft[k].data_ptr() != t[k].data_ptr():
            raise _lib.QuorumBatchError(f"the election state's {k} is not the table's tensor")
    ptr = lambda v: None if v is None else v.data_ptr()  # noqa: E731
    sg = SwitchGroupsC(G=G, inflight_cap=K, readq_cap=Q,
                       **{k: ptr(v[0]) for k, v in tensors.items()})
    so = SwitchOutC(**{k: ptr(v[0]) for k, v in outs.items()})
    return sg, so, out


def switch_config(groups: LeaderGroups, election: ElectionState, old: ConfigTable,
                  new: ConfigTable, action: torch.Tensor, *, adopt: bool = True, stream=None,
                  out: Optional[SwitchResult] = None) -> SwitchResult:
    """switchToConfig for every group, in place.  ``old`` is the ConfigTable
    ``change`` was called on, ``new`` the one it returned (its arrays are used
    as they are: nothing is repacked); ``action`` a device u8 tensor of G
    SW_* codes.  The group words are the table's and the election state's.
    ``out``: a previous result whose buffers are reused (stats accumulate);
    else fresh zero-filled ones.

    ``adopt`` (default): after the call the table runs on the new config —
    ``groups`` takes over ``new``'s off, cfg and Progress tensors (groups.S
    follows), so the next ``leader_propose`` / ``leader_tick`` / ``campaign``
    sees the renumbered slots.  The new table holds every group's new config
    (``change`` copies a group without an operation through), but the call
    renumbers meta, votes and rq_meta only where it acted and was not stopped:
    a group whose conf change was applied and whose action was SW_NONE, and a
    group that came back SWFLAG_HOST, still name OLD slots in those words.
    Before the next leader_* call on an adopted table the host repacks those
    groups' words itself (switchToConfig by ID for a SWFLAG_HOST group), or it
    passes ``adopt=False``, keeps ``groups`` on the old tensors and adopts
    when it has dealt with them."""
    sg, so, out = switch_args(groups, election, old, new, action, out)
    _lib.call("qb_dev_switch_config", C.byref(sg), action.data_ptr(), C.byref(so),
              out.stats.data_ptr(), stream_handle(groups.device, stream))
    if adopt:
        for k in _ADOPTED:
            groups.t[k] = new.t[k]
        groups.S = int(new.S)
    out.groups, out.table = groups, new
    return out
