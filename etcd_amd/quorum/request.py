"""The batched requests (include/quorum_batch.h ``qb_dev_leader_requests``).

Step(MsgReadIndex) and Step(MsgTransferLeader) (raft.go:1078-1097, 1339-1370,
1445-1464, 1827-1843; read_only.go:56-76) for every group of a ``LeaderGroups``
table in one call: up to ``max_reads`` read requests and at most one transfer
request per group.  It runs in the HIP library over the table's own arrays
(the read queue included), the follower step's (lead, last_term) and the
tick's role bytes and election timer; torch only holds device memory.  What
stays the host's per status and flag is in INTEGRATION.md.
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

MAX_READS = 16
NO_SLOT = 0xFF
MSG_APP, MSG_SNAP, MSG_TIMEOUT_NOW = 3, 7, 14
RD_READ_STATE, RD_RESP, RD_BCAST, RD_BCAST_DUP, RD_POSTPONED = 1, 2, 3, 4, 5
RD_FORWARD, RD_DROPPED, RD_IGNORED, RD_QUEUE_FULL, RD_HOST, RD_BAD = 6, 7, 8, 9, 10, 11
QFLAG_HEARTBEATS, QFLAG_POSTPONED, QFLAG_TRANSFER_STARTED = 0x01, 0x02, 0x04
QFLAG_TRANSFER_ABORTED, QFLAG_FORWARD, QFLAG_HOST, QFLAG_BAD = 0x08, 0x10, 0x20, 0x40
QSTAT_NAMES = ("read_states", "read_resps", "bcast", "bcast_dup", "postponed", "rd_forward",
               "rd_dropped", "rd_ignored", "queue_full", "rd_host", "bad_ctx", "bad_count",
               "bcast_groups", "xf_started", "xf_timeout_now", "xf_msg_app", "xf_msg_snap",
               "xf_aborted", "xf_ign_term", "xf_ign_no_progress", "xf_ign_learner", "xf_ign_same",
               "xf_ign_self", "xf_ign_role", "xf_forward", "xf_dropped", "xf_host")

_P = C.c_void_p
_POINTERS = ("off", "cfg", "meta", "role", "term", "lead", "committed", "first_index",
             "last_index", "last_term", "snap_index", "snap_term", "max_ents", "run_start",
             "run_term", "election_elapsed", "match", "next", "pending_snapshot", "pstate",
             "infl_pos", "infl_buf", "rq_ctx", "rq_index", "rq_meta")
_IN_POINTERS = ("n_reads", "rd_ctx", "rd_from", "xf_from", "xf_term")
_OUT_POINTERS = ("rd_status", "rd_index", "hb_commit", "xf_type", "xf_index", "xf_log_term",
                 "xf_n", "qflags")


class RequestGroupsC(C.Structure):
    """struct qb_request_groups (include/quorum_batch.h)."""
    _fields_ = [("G", C.c_uint64), ("inflight_cap", C.c_uint32), ("readq_cap", C.c_uint32),
                ("read_only", C.c_uint32), ("max_reads", C.c_uint32)] + [(n, _P) for n in _POINTERS]


class RequestInC(C.Structure):
    """struct qb_request_in."""
    _fields_ = [(n, _P) for n in _IN_POINTERS]


class RequestOutC(C.Structure):
    """struct qb_request_out."""
    _fields_ = [(n, _P) for n in _OUT_POINTERS]


@dataclass
class RequestInbox:
    """The requests of one call (struct qb_request_in), device tensors:
    ``n_reads`` u8 [G]; ``rd_ctx`` u64 and ``rd_from`` u8 [max_reads * G],
    k-major (request k of group g at k * G + g; rd_from NO_SLOT = local);
    ``xf_from`` u8 [G] (NO_SLOT = no transfer request); ``xf_term`` u64 [G]
    or None (every transfer request is local)."""
    max_reads: int
    n_reads: torch.Tensor
    rd_ctx: torch.Tensor
    rd_from: torch.Tensor
    xf_from: torch.Tensor
    xf_term: Optional[torch.Tensor] = None

    @classmethod
    def from_numpy(cls, max_reads, n_reads, rd_ctx, rd_from, xf_from=None, xf_term=None,
                   device="cuda"):
        dev = torch.device(device)
        G = len(n_reads)
        xf_from = np.full(G, NO_SLOT, np.uint8) if xf_from is None else xf_from
        for k, a, n in (("rd_ctx", rd_ctx, max_reads * G), ("rd_from", rd_from, max_reads * G),
                        ("xf_from", xf_from, G)) + ((("xf_term", xf_term, G),)
                                                    if xf_term is not None else ()):
            if len(a) != n:
                raise _lib.QuorumBatchError(f"{k} has {len(a)} entries, want {n}")
        return cls(int(max_reads), _to_dev(n_reads, np.uint8, dev), _to_dev(rd_ctx, np.uint64, dev),
                   _to_dev(rd_from, np.uint8, dev), _to_dev(xf_from, np.uint8, dev),
                   None if xf_term is None else _to_dev(xf_term, np.uint64, dev))


@dataclass
class RequestResult:
    """Device outputs of one requests call.  rd_status holds a value only for
    k < n_reads[g], rd_index only where the status answers, hb_commit only in
    the peer slots of groups with QFLAG_HEARTBEATS, xf_index / xf_log_term /
    xf_n only where xf_type is MSG_APP / MSG_SNAP; the rest keeps what the
    buffers held."""
    rd_status: torch.Tensor    # [max_reads * G] u8 RD_*
    rd_index: torch.Tensor     # [max_reads * G] u64 (int64 storage)
    hb_commit: torch.Tensor    # [S] u64
    xf_type: torch.Tensor      # [G] u8: 0 / MSG_TIMEOUT_NOW / MSG_APP / MSG_SNAP
    xf_index: torch.Tensor     # [G] u64
    xf_log_term: torch.Tensor  # [G] u64
    xf_n: torch.Tensor         # [G] u64
    qflags: torch.Tensor       # [G] u8 QFLAG_*
    stats: torch.Tensor        # [len(QSTAT_NAMES)] u64, accumulated
    groups: Optional[LeaderGroups] = None
    inbox: Optional[RequestInbox] = None

    def stats_dict(self) -> Dict[str, int]:
        return stats_dict(QSTAT_NAMES, self.stats)

    def reads(self, g: int) -> List[Tuple[int, int, int, Optional[int]]]:
        """Group g's read requests of this call as (status, ctx, from slot,
        read index or None), in k order."""
        lg, ib = self.groups, self.inbox
        if not 0 <= g < lg.G:
            raise IndexError(g)
        n = min(int(ib.n_reads[g].item()), ib.max_reads)
        at = [k * lg.G + g for k in range(n)]
        st = self.rd_status[at].cpu().numpy() if n else []
        ix = _to_np(self.rd_index[at], np.uint64) if n else []
        cx = _to_np(ib.rd_ctx[at], np.uint64) if n else []
        fr = ib.rd_from[at].cpu().numpy() if n else []
        return [(int(st[k]), int(cx[k]), int(fr[k]),
                 int(ix[k]) if st[k] in (RD_READ_STATE, RD_RESP) else None) for k in range(n)]

    def heartbeats(self, g: int) -> List[Tuple[int, int]]:
        """(to slot, commit) of one broadcast of group g, ascending slots;
        empty unless qflags has QFLAG_HEARTBEATS.  The host sends them once per
        RD_BCAST / RD_BCAST_DUP request, with that request's context."""
        lg = self.groups
        if not 0 <= g < lg.G:
            raise IndexError(g)
        if not int(self.qflags[g].item()) & QFLAG_HEARTBEATS:
            return []
        off = _to_np(lg.t["off"][g:g + 2], np.uint32)
        lo, hi = int(off[0]), int(off[1])
        hi = min(hi, lo + _lib.QB_MAX_SLOTS)
        own = int(_to_np(lg.t["meta"][g:g + 1], np.uint32)[0]) & 0xFF
        hb = _to_np(self.hb_commit[lo:hi], np.uint64) if hi > lo else []
        return [(k, int(hb[k])) for k in range(max(hi - lo, 0)) if k != own]

    def transfer(self, g: int) -> Optional[Tuple[int, int, int, int, int, int]]:
        """The message group g's transfer request produced, as (type, to,
        index, log_term, commit, n) — a MSG_TIMEOUT_NOW carries only its
        recipient — or None."""
        lg = self.groups
        if not 0 <= g < lg.G:
            raise IndexError(g)
        t = int(self.xf_type[g].item())
        if not t:
            return None
        to = int(self.inbox.xf_from[g].item())
        if t == MSG_TIMEOUT_NOW:
            return (t, to, 0, 0, 0, 0)
        commit = int(_to_np(lg.t["committed"][g:g + 1], np.uint64)[0]) if t == MSG_APP else 0
        return (t, to, int(_to_np(self.xf_index[g:g + 1], np.uint64)[0]),
                int(_to_np(self.xf_log_term[g:g + 1], np.uint64)[0]), commit,
                int(_to_np(self.xf_n[g:g + 1], np.uint64)[0]))


def new_result(G: int, S: int, max_reads: int, device) -> RequestResult:
    """Fresh zero-filled output buffers."""
    n, s, r = max(G, 1), max(S, 1), max(G * max_reads, 1)
    z = lambda k, dt: torch.zeros(k, dtype=dt, device=device)  # noqa: E731
    return RequestResult(z(r, torch.uint8), z(r, torch.int64), z(s, torch.int64), z(n, torch.uint8),
                         z(n, torch.int64), z(n, torch.int64), z(n, torch.int64), z(n, torch.uint8),
                         z(len(QSTAT_NAMES), torch.int64))


def request_structs(groups: LeaderGroups, election: ElectionState, inbox: RequestInbox,
                    out: RequestResult):
    """The three C structs of a call over checked tensors."""
    G, S, t = groups.G, groups.S, groups.t
    fg = election.follower
    st, ft = fg.state, fg.t
    R = int(inbox.max_reads)
    if fg.G != G:
        raise _lib.QuorumBatchError(f"the election state holds {fg.G} groups, the table {G}")
    if not 1 <= int(groups.inflight_cap) <= 4096:
        raise _lib.QuorumBatchError(f"inflight_cap must be 1..4096, got {groups.inflight_cap}")
    if not 1 <= R <= MAX_READS:
        raise _lib.QuorumBatchError(f"max_reads must be 1..{MAX_READS}, got {R}")
    if not 0 <= int(groups.readq_cap) <= 16:
        raise _lib.QuorumBatchError(f"readq_cap must be 0..16, got {groups.readq_cap}")
    if int(groups.read_only) not in (0, 1):
        raise _lib.QuorumBatchError(f"read_only must be 0 or 1, got {groups.read_only}")
    K, Q = int(groups.inflight_cap), int(groups.readq_cap)
    tensors = {"off": (t["off"], I32, G + 1), "cfg": (t["cfg"], I32, G),
               "meta": (t["meta"], I32, G), "role": (st.role, U8, G), "term": (ft["term"], I64, G),
               "lead": (ft["lead"], I64, G), "committed": (ft["committed"], I64, G),
               "first_index": (t["first_index"], I64, G), "last_index": (ft["last_index"], I64, G),
               "last_term": (ft["last_term"], I64, G), "snap_index": (t["snap_index"], I64, G),
               "snap_term": (t["snap_term"], I64, G), "max_ents": (t["max_ents"], I64, G),
               "run_start": (t["run_start"], I64, MAX_RUNS * G),
               "run_term": (t["run_term"], I64, MAX_RUNS * G),
               "election_elapsed": (st.election_elapsed, I32, G),
               "match": (t["match"], I64, S), "next": (t["next"], I64, S),
               "pending_snapshot": (t["pending_snapshot"], I64, S), "pstate": (t["pstate"], U8, S),
               "infl_pos": (t["infl_pos"], I32, S), "infl_buf": (t["infl_buf"], I64, S * K),
               "rq_ctx": (t["rq_ctx"], I64, G * Q), "rq_index": (t["rq_index"], I64, G * Q),
               "rq_meta": (t["rq_meta"], I32, G * Q)}
    ins = {"n_reads": (inbox.n_reads, U8, G), "rd_ctx": (inbox.rd_ctx, I64, R * G),
           "rd_from": (inbox.rd_from, U8, R * G), "xf_from": (inbox.xf_from, U8, G),
           "xf_term": (inbox.xf_term, I64, G)}
    outs = {"rd_status": (out.rd_status, U8, R * G), "rd_index": (out.rd_index, I64, R * G),
            "hb_commit": (out.hb_commit, I64, S), "xf_type": (out.xf_type, U8, G),
            "xf_index": (out.xf_index, I64, G), "xf_log_term": (out.xf_log_term, I64, G),
            "xf_n": (out.xf_n, I64, G), "qflags": (out.qflags, U8, G)}
    check_tensors(tuple((v[0], k, v[1], v[2]) for d in (tensors, ins, outs) for k, v in d.items()) +
                  ((out.stats, "stats", I64, len(QSTAT_NAMES)),))
    # the table's term / committed / last_index are the election state's
    # (ElectionState.for_table builds it so): one set of buffers
    for k in ("term", "committed", "last_index"):
        if ft[k].data_ptr() != t[k].data_ptr():
            raise _lib.QuorumBatchError(f"the election state's {k} is not the table's tensor")
    ptr = lambda d: {k: (v[0].data_ptr() if v[0] is not None else None)  # noqa: E731
                     for k, v in d.items()}
    rg = RequestGroupsC(G=G, inflight_cap=K, readq_cap=Q, read_only=int(groups.read_only),
                        max_reads=R, **ptr(tensors))
    return rg, RequestInC(**ptr(ins)), RequestOutC(**ptr(outs))


def leader_requests(groups: LeaderGroups, election: ElectionState, inbox: RequestInbox, *,
                    stream=None, out: Optional[RequestResult] = None) -> RequestResult:
    """Apply the read and transfer requests of ``inbox`` to every group, in
    place: within a group the reads in k order, then the transfer.  The read
    queue, ``readq_cap`` and ``read_only`` are the table's.  ``out``: a
    previous result whose buffers are reused (stats accumulate); else fresh
    zero-filled ones.  ``stream``: a torch stream or a raw hipStream_t; default
    the current stream."""
    if out is None:
        out = new_result(groups.G, groups.S, int(inbox.max_reads), groups.device)
    rg, rin, rout = request_structs(groups, election, inbox, out)
    _lib.call("qb_dev_leader_requests", C.byref(rg), C.byref(rin), C.byref(rout),
              out.stats.data_ptr(), stream_handle(groups.device, stream))
    out.groups, out.inbox = groups, inbox
    return out
