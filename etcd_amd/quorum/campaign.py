"""The batched campaign (include/quorum_batch.h ``qb_dev_campaign``).

The state changes of an election for every group of a ``LeaderGroups`` table
in one call: Step(MsgHup) -> hup -> campaign -> becomePreCandidate /
becomeCandidate -> poll self -> vote requests (raft.go:760-845), and
becomeLeader (+ bcastAppend) or becomeFollower once the tally is in
(raft.go:1399-1414).  It runs in the HIP library over the table's own arrays
(off, cfg, meta, term, committed, last_index, match, next, pending_snapshot,
pstate, infl_pos), the follower step's (vote, lead, last_term), the tick's
``TickState`` and the per-group ``ElectionState``; torch only holds device
memory.  What stays the host's per flag is in INTEGRATION.md.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch

from .. import _lib
from ._checks import I16, I32, I64, U8, check_tensors
from ._dev import stats_dict, stream_handle
from ._dev import to_dev as _to_dev, to_np as _to_np
from .follower import FollowerGroups
from .leader import LeaderGroups
from .tick import TickState

CAMP_NONE, CAMP_HUP, CAMP_TRANSFER, CAMP_WON, CAMP_LOST = 0, 1, 2, 3, 4
CAMP_PENDING_CONF = 0x80
MSG_VOTE, MSG_PREVOTE = 5, 17
CREQ_TRANSFER = 0x80
CFLAG_REQUESTS, CFLAG_BECAME_LEADER, CFLAG_BCAST_APPEND = 0x01, 0x02, 0x04
CFLAG_RESET, CFLAG_HARDSTATE, CFLAG_IGNORED = 0x08, 0x10, 0x20
CSTAT_NAMES = ("pre_campaigns", "campaigns", "became_leader", "became_follower", "vote_requests",
               "ignored_leader", "ignored_unpromotable", "ignored_pending_conf", "ignored_role",
               "bad_action")

_P = C.c_void_p
_POINTERS = ("off", "cfg", "meta", "self_id", "term", "vote", "lead", "committed", "last_index",
             "last_term", "role", "election_elapsed", "heartbeat_elapsed", "votes", "match", "next",
             "pending_snapshot", "pstate", "infl_pos")


class CampaignGroupsC(C.Structure):
    """struct qb_campaign_groups (include/quorum_batch.h)."""
    _fields_ = [("G", C.c_uint64), ("pre_vote", C.c_uint32), ("reserved", C.c_uint32)] + [
        (n, _P) for n in _POINTERS]


@dataclass
class ElectionState:
    """What an election needs beyond the leader table: ``self_id`` (the node's
    raft ID per group, u64) and ``votes`` (the voted | granted << 16 word of
    ``record_votes``, u32), device tensors of G entries, and ``follower`` —
    the ``FollowerGroups`` of the same node, whose term / committed /
    last_index tensors ARE the table's (``for_table`` builds it so) and whose
    ``state`` is the tick's ``TickState``: the tick, the follower step, the
    leader step and the campaign all run over one set of buffers."""
    self_id: torch.Tensor
    votes: torch.Tensor
    follower: FollowerGroups

    @classmethod
    def for_table(cls, groups: LeaderGroups, state: TickState, self_id, vote, lead, last_term,
                  election_timeout: int, check_quorum: bool, pre_vote: bool,
                  votes=None) -> "ElectionState":
        """self_id / vote / lead / last_term (and votes, default 0): numpy
        columns of G entries, copied to the table's device."""
        G, dev = groups.G, groups.device
        cols = {"self_id": self_id, "vote": vote, "lead": lead, "last_term": last_term}
        if votes is not None:
            cols["votes"] = votes
        for k, a in cols.items():
            if len(a) != G:
                raise _lib.QuorumBatchError(f"{k} has {len(a)} entries, the table {G} groups")
        t = {"term": groups.t["term"], "committed": groups.t["committed"],
             "last_index": groups.t["last_index"], "vote": _to_dev(vote, np.uint64, dev),
             "lead": _to_dev(lead, np.uint64, dev), "last_term": _to_dev(last_term, np.uint64, dev)}
        fg = FollowerGroups(G, int(election_timeout), bool(check_quorum), bool(pre_vote), t, state)
        return cls(_to_dev(self_id, np.uint64, dev),
                   _to_dev(votes if votes is not None else np.zeros(G, np.uint32), np.uint32, dev),
                   fg)

    def numpy(self) -> Dict[str, np.ndarray]:
        G = self.follower.G
        out = self.follower.numpy()
        out["self_id"] = _to_np(self.self_id, np.uint64, G)
        out["votes"] = _to_np(self.votes, np.uint32, G)
        return out


@dataclass
class CampaignResult:
    """Device outputs of one campaign call.  req_term / req_mask hold a value
    only where req_type is non-zero; the rest keeps what the buffers held."""
    cflags: torch.Tensor    # [G] u8 CFLAG_*
    req_type: torch.Tensor  # [G] u8: MSG_VOTE / MSG_PREVOTE | CREQ_TRANSFER, 0 = none
    req_term: torch.Tensor  # [G] u64 (int64 storage)
    req_mask: torch.Tensor  # [G] u16 (int16 storage): recipient slots
    stats: torch.Tensor     # [len(CSTAT_NAMES)] u64, accumulated
    groups: Optional[LeaderGroups] = None
    election: Optional[ElectionState] = None

    def stats_dict(self) -> Dict[str, int]:
        return stats_dict(CSTAT_NAMES, self.stats)

    def requests(self, g: int) -> List[dict]:
        """Group g's vote requests of this call, in the order the reference
        emits them (raft.go:813-834: ascending IDs are ascending slots), as
        dicts: type (MSG_VOTE / MSG_PREVOTE), to (slot), term, index, log_term
        and transfer (the Context is "CampaignTransfer"); empty unless the
        group campaigned and did not win on its own vote."""
        lg, fg = self.groups, self.election.follower
        if not 0 <= g < lg.G:
            raise IndexError(g)
        rt = int(self.req_type[g].item())
        if not rt:
            return []
        term = int(_to_np(self.req_term[g:g + 1], np.uint64)[0])
        mask = int(_to_np(self.req_mask[g:g + 1], np.uint16)[0])
        index = int(_to_np(fg.t["last_index"][g:g + 1], np.uint64)[0])
        log_term = int(_to_np(fg.t["last_term"][g:g + 1], np.uint64)[0])
        return [{"type": rt & 0x7F, "to": s, "term": term, "index": index, "log_term": log_term,
                 "transfer": bool(rt & CREQ_TRANSFER)}
                for s in range(_lib.QB_MAX_SLOTS) if (mask >> s) & 1]


def campaign(groups: LeaderGroups, election: ElectionState, action: torch.Tensor, stream=None, *,
             out: Optional[CampaignResult] = None) -> CampaignResult:
    """Apply ``action`` ([G] u8: CAMP_* | CAMP_PENDING_CONF) to every group, in
    place.  ``out``: a previous result whose buffers are reused (stats
    accumulate); else fresh zero-filled ones.  ``stream``: a torch stream or a
    raw hipStream_t; default the current stream."""
    G, S, dev, t = groups.G, groups.S, groups.device, groups.t
    fg = election.follower
    st, ft = fg.state, fg.t
    if fg.G != G:
        raise _lib.QuorumBatchError(f"the election state holds {fg.G} groups, the table {G}")
    if out is None:
        n = max(G, 1)
        out = CampaignResult(torch.zeros(n, dtype=torch.uint8, device=dev),
                             torch.zeros(n, dtype=torch.uint8, device=dev),
                             torch.zeros(n, dtype=torch.int64, device=dev),
                             torch.zeros(n, dtype=torch.int16, device=dev),
                             torch.zeros(len(CSTAT_NAMES), dtype=torch.int64, device=dev))
    check_tensors(((t["off"], "off", I32, G + 1), (t["cfg"], "cfg", I32, G),
                   (t["meta"], "meta", I32, G), (election.self_id, "self_id", I64, G),
                   (ft["term"], "term", I64, G), (ft["vote"], "vote", I64, G),
                   (ft["lead"], "lead", I64, G), (ft["committed"], "committed", I64, G),
                   (ft["last_index"], "last_index", I64, G), (ft["last_term"], "last_term", I64, G),
                   (st.role, "state.role", U8, G),
                   (st.election_elapsed, "state.election_elapsed", I32, G),
                   (st.heartbeat_elapsed, "state.heartbeat_elapsed", I32, G),
                   (election.votes, "votes", I32, G), (t["match"], "match", I64, S),
                   (t["next"], "next", I64, S), (t["pending_snapshot"], "pending_snapshot", I64, S),
                   (t["pstate"], "pstate", U8, S), (t["infl_pos"], "infl_pos", I32, S),
                   (action, "action", U8, G), (out.cflags, "cflags", U8, G),
                   (out.req_type, "req_type", U8, G), (out.req_term, "req_term", I64, G),
                   (out.req_mask, "req_mask", I16, G),
                   (out.stats, "stats", I64, len(CSTAT_NAMES))))
    stream = stream_handle(dev, stream)
    cg = CampaignGroupsC(G=G, pre_vote=1 if fg.pre_vote else 0, reserved=0,
                         off=t["off"].data_ptr(), cfg=t["cfg"].data_ptr(),
                         meta=t["meta"].data_ptr(), self_id=election.self_id.data_ptr(),
                         term=ft["term"].data_ptr(), vote=ft["vote"].data_ptr(),
                         lead=ft["lead"].data_ptr(), committed=ft["committed"].data_ptr(),
                         last_index=ft["last_index"].data_ptr(),
                         last_term=ft["last_term"].data_ptr(), role=st.role.data_ptr(),
                         election_elapsed=st.election_elapsed.data_ptr(),
                         heartbeat_elapsed=st.heartbeat_elapsed.data_ptr(),
                         votes=election.votes.data_ptr(), match=t["match"].data_ptr(),
                         next=t["next"].data_ptr(),
                         pending_snapshot=t["pending_snapshot"].data_ptr(),
                         pstate=t["pstate"].data_ptr(), infl_pos=t["infl_pos"].data_ptr())
    _lib.call("qb_dev_campaign", C.byref(cg), action.data_ptr(), out.cflags.data_ptr(),
              out.req_type.data_ptr(), out.req_term.data_ptr(), out.req_mask.data_ptr(),
              out.stats.data_ptr(), stream)
    out.groups, out.election = groups, election
    return out
