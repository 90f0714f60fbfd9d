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


# ---- the log step: the follower step plus MsgApp (qb_dev_follower_log_step) ----

FIN_APP = 5
FFLAG_LOG_CONFLICT, FFLAG_LOG_RUNS, FFLAG_APPENDED = 0x20, 0x40, 0x80
MAX_RUNS = 8  # QB_LEADER_MAX_RUNS
FLSTAT_NAMES = FSTAT_NAMES + ("app_accepted", "app_rejected", "app_below_commit",
                              "entries_appended", "app_truncated")


class FollowerLogC(C.Structure):
    """struct qb_follower_log."""
    _fields_ = [(n, _P) for n in ("meta", "first_index", "last_index", "last_term", "run_start",
                                  "run_term")]


class FollowerAppInboxC(C.Structure):
    """struct qb_follower_app_inbox."""
    _fields_ = [(n, _P) for n in ("commit", "ent_off", "ent_term", "ent_len")] + [("E", C.c_uint64)]


class FollowerAppOutC(C.Structure):
    """struct qb_follower_app_out."""
    _fields_ = [(n, _P) for n in ("resp_index", "resp_hint", "resp_log_term", "app_from")]


def check_run_table(meta, first_index, run_start, run_term, last_index, last_term,
                    committed) -> None:
    """The invariant qb_dev_follower_log_step relies on, over host arrays
    (run tables [MAX_RUNS, G]): 1..8 runs, run 0 at first_index - 1, starts
    ascending up to last_index, adjacent runs of different terms, the last
    run's term == last_term, first_index - 1 <= committed."""
    G = len(first_index)
    nr = (np.asarray(meta, np.uint32) >> 16) & 0xF
    first = np.asarray(first_index, np.uint64)
    rs = np.asarray(run_start, np.uint64).reshape(MAX_RUNS, G)
    rt = np.asarray(run_term, np.uint64).reshape(MAX_RUNS, G)

    def refuse(bad, what):
        if bad.any():
            g = int(np.flatnonzero(bad)[0])
            raise _lib.QuorumBatchError(f"follower log of group {g}: {what}")

    refuse((nr < 1) | (nr > MAX_RUNS), "the run count in meta bits 16-19 must be 1..8")
    refuse(first < 1, "first_index must be >= 1")
    refuse(rs[0] != first - np.uint64(1), "run 0 must start at first_index - 1")
    refuse(np.asarray(committed, np.uint64) < first - np.uint64(1),
           "committed is below first_index - 1")
    gi = np.arange(G)
    for r in range(1, MAX_RUNS):
        live = nr > r
        refuse(live & (rs[r] <= rs[r - 1]), f"run {r} does not start behind run {r - 1}")
        refuse(live & (rt[r] == rt[r - 1]), f"run {r} has the term of run {r - 1}")
    refuse(rs[nr - 1, gi] > np.asarray(last_index, np.uint64), "a run starts behind last_index")
    refuse(rt[nr - 1, gi] != np.asarray(last_term, np.uint64),
           "the last run's term is not last_term")


@dataclass
class FollowerLog:
    """The term index of G logs (struct qb_follower_log): ``meta`` (the run
    count in bits 16-19; the leader step's word), ``first_index`` and the run
    tables, run-major [MAX_RUNS * G].  last_index / last_term are the
    ``FollowerGroups``' own tensors."""
    G: int
    meta: torch.Tensor         # [G] u32 (int32 storage)
    first_index: torch.Tensor  # [G] u64 (int64 storage)
    run_start: torch.Tensor    # [MAX_RUNS * G]
    run_term: torch.Tensor     # [MAX_RUNS * G]

    @classmethod
    def from_numpy(cls, meta, first_index, run_start, run_term, groups: Dict[str, np.ndarray],
                   device="cuda") -> "FollowerLog":
        """``groups``: the arrays the FollowerGroups are built from (last_index,
        last_term and committed are checked against the table here)."""
        dev = torch.device(device)
        G = len(first_index)
        for what, a, n in (("meta", meta, G), ("run_start", run_start, MAX_RUNS * G),
                           ("run_term", run_term, MAX_RUNS * G)):
            if np.asarray(a).size != n:
                raise _lib.QuorumBatchError(f"log {what} has {np.asarray(a).size} entries, not {n}")
        for k in ("last_index", "last_term", "committed"):
            if k not in groups or len(groups[k]) != G:
                raise _lib.QuorumBatchError(f"log check needs {k} of {G} groups")
        check_run_table(meta, first_index, run_start, run_term, groups["last_index"],
                        groups["last_term"], groups["committed"])
        return cls(G, _to_dev(meta, np.uint32, dev), _to_dev(first_index, np.uint64, dev),
                   _to_dev(np.asarray(run_start).reshape(-1), np.uint64, dev),
                   _to_dev(np.asarray(run_term).reshape(-1), np.uint64, dev))

    def numpy(self) -> Dict[str, np.ndarray]:
        G = self.G
        return {"meta": _to_np(self.meta, np.uint32, G),
                "first_index": _to_np(self.first_index, np.uint64, G),
                "run_start": _to_np(self.run_start, np.uint64, MAX_RUNS * G).reshape(MAX_RUNS, G),
                "run_term": _to_np(self.run_term, np.uint64, MAX_RUNS * G).reshape(MAX_RUNS, G)}

    def validate(self, groups: FollowerGroups) -> None:
        """check_run_table over the device state (copies it to the host)."""
        a, g = self.numpy(), groups.numpy()
        check_run_table(a["meta"], a["first_index"], a["run_start"], a["run_term"],
                        g["last_index"], g["last_term"], g["committed"])


@dataclass
class FollowerAppInbox:
    """The MsgApp columns beside a ``FollowerInbox`` of the same M: Commit and
    each record's entries run-length encoded by term (``ent_off`` [M + 1]
    into ``ent_term`` / ``ent_len`` [E]).  For a FIN_APP record the inbox's
    index is Message.Index and aux Message.LogTerm."""
    commit: torch.Tensor
    ent_off: torch.Tensor
    ent_term: torch.Tensor
    ent_len: torch.Tensor
    E: int

    @classmethod
    def from_numpy(cls, commit, ent_off, ent_term, ent_len, device="cuda") -> "FollowerAppInbox":
        dev = torch.device(device)
        if len(ent_off) != len(commit) + 1:
            raise _lib.QuorumBatchError(f"ent_off has {len(ent_off)} entries, not M + 1 = "
                                        f"{len(commit) + 1}")
        if len(ent_term) != len(ent_len):
            raise _lib.QuorumBatchError(f"ent_term has {len(ent_term)} entries, ent_len "
                                        f"{len(ent_len)}")
        return cls(_to_dev(commit, np.uint64, dev), _to_dev(ent_off, np.uint32, dev),
                   _to_dev(ent_term, np.uint64, dev), _to_dev(ent_len, np.uint32, dev),
                   len(ent_term))

    def check(self, M: int) -> None:
        if not 0 <= int(self.E) < 1 << 64:
            raise _lib.QuorumBatchError(f"E must be a uint64, got {self.E}")
        check_tensors(((self.commit, "app.commit", I64, M), (self.ent_off, "app.ent_off", I32, M + 1),
                       (self.ent_term, "app.ent_term", I64, self.E),
                       (self.ent_len, "app.ent_len", I32, self.E)))


@dataclass
class FollowerLogResult(FollowerResult):
    """``FollowerResult`` (stats: FLSTAT_NAMES) plus the MsgApp columns."""
    resp_index: Optional[torch.Tensor] = None     # [M] u64
    resp_hint: Optional[torch.Tensor] = None      # [M] u64, rejected MsgAppResp only
    resp_log_term: Optional[torch.Tensor] = None  # [M] u64, same
    app_from: Optional[torch.Tensor] = None       # [M] u64, 0 = the host's log takes nothing

    def stats_dict(self) -> Dict[str, int]:
        return stats_dict(FLSTAT_NAMES, self.stats)

    def responses(self) -> Iterator[dict]:
        """As ``FollowerResult.responses``; a MsgAppResp also carries index,
        and with reject the hint and its log_term.  They may be sent once the
        HardState (FFLAG_HARDSTATE) and the entries (FFLAG_APPENDED) of their
        group are persisted."""
        m = self.inbox.M
        if m == 0:
            return
        idx = _to_np(self.resp_index, np.uint64, m)
        hint = _to_np(self.resp_hint, np.uint64, m)
        lterm = _to_np(self.resp_log_term, np.uint64, m)
        for r in super().responses():
            if r["type"] == MSG_APP_RESP:
                i = r["i"]
                r["index"] = int(idx[i])
                r["hint"] = int(hint[i]) if r["reject"] else 0
                r["log_term"] = int(lterm[i]) if r["reject"] else 0
            yield r

    def appends(self) -> Iterator[dict]:
        """The records whose entries the host's log takes, in batch order:
        truncate behind ``from - 1`` and append the message's entries from
        index ``from`` on."""
        m = self.inbox.M
        if m == 0:
            return
        af = _to_np(self.app_from, np.uint64, m)
        for i in np.flatnonzero(af).tolist():
            yield {"i": i, "from": int(af[i])}


def follower_log_workspace_bytes(G: int, M: int) -> int:
    # (the grouping, and so the workspace, is the follower step's)
    n = int(_lib.fn("qb_follower_workspace_bytes")(G, M))
    if n == 0:
        raise _lib.QuorumBatchError(f"no follower-log-step workspace for G={G}, M={M} "
                                    f"(M <= 2^32 - 2)")
    return n


def follower_log_step(groups: FollowerGroups, log: FollowerLog, inbox: FollowerInbox,
                      app: FollowerAppInbox, stream=None, *,
                      out: Optional[FollowerLogResult] = None) -> FollowerLogResult:
    """``follower_step`` with FIN_APP records: steps ``inbox`` / ``app`` into
    ``groups`` and ``log`` in place.  ``out`` / ``stream`` as there."""
    G, st, t = groups.G, groups.state, groups.t
    if not 1 <= int(groups.election_timeout) <= 0xFFFFFFFF:
        raise _lib.QuorumBatchError(f"election_timeout must be 1..2^32-1, got "
                                    f"{groups.election_timeout}")
    if log.G != G:
        raise _lib.QuorumBatchError(f"the log has {log.G} groups, the groups {G}")
    inbox.check()
    M = inbox.M
    app.check(M)
    group_specs = tuple((t[k], k, I64, G) for k in _U64_FIELDS) + (
        (st.role, "state.role", U8, G), (st.election_elapsed, "state.election_elapsed", I32, G),
        (st.heartbeat_elapsed, "state.heartbeat_elapsed", I32, G),
        (log.meta, "log.meta", I32, G), (log.first_index, "log.first_index", I64, G),
        (log.run_start, "log.run_start", I64, MAX_RUNS * G),
        (log.run_term, "log.run_term", I64, MAX_RUNS * G))
    check_tensors(group_specs + ((inbox.group, "inbox.group", I32, M),
                                 (app.commit, "app.commit", I64, M)))
    dev = groups.device
    need = follower_log_workspace_bytes(G, M)
    if out is None:
        def col():
            return torch.zeros(max(M, 1), dtype=torch.int64, device=dev)
        out = FollowerLogResult(torch.zeros(max(M, 1), dtype=torch.uint8, device=dev), col(),
                                torch.zeros(max(G, 1), dtype=torch.int32, device=dev),
                                torch.zeros(max(G, 1), dtype=torch.uint8, device=dev),
                                torch.zeros(len(FLSTAT_NAMES), dtype=torch.int64, device=dev),
                                torch.empty((need + 7) // 8, dtype=torch.int64, device=dev),
                                None, col(), col(), col(), col())
    for what in ("resp_index", "resp_hint", "resp_log_term", "app_from"):
        if getattr(out, what, None) is None:   # (a FollowerResult of follower_step lacks them)
            raise _lib.QuorumBatchError(f"{what} is missing from the result to reuse: pass a "
                                        f"FollowerLogResult of follower_log_step")
    check_tensors(group_specs[:1] + (
        (out.resp_type, "resp_type", U8, M), (out.resp_term, "resp_term", I64, M),
        (out.resp_index, "resp_index", I64, M), (out.resp_hint, "resp_hint", I64, M),
        (out.resp_log_term, "resp_log_term", I64, M), (out.app_from, "app_from", I64, M),
        (out.stop_at, "stop_at", I32, G), (out.gflags, "gflags", U8, G),
        (out.stats, "stats", I64, len(FLSTAT_NAMES)),
        (out.workspace, "workspace", I64, (need + 7) // 8)))
    stream = stream_handle(dev, stream)
    fg = FollowerGroupsC(G=G, election_timeout=int(groups.election_timeout),
                         check_quorum=1 if groups.check_quorum else 0,
                         pre_vote=1 if groups.pre_vote else 0, reserved=0,
                         role=st.role.data_ptr(), election_elapsed=st.election_elapsed.data_ptr(),
                         heartbeat_elapsed=st.heartbeat_elapsed.data_ptr(),
                         **{k: t[k].data_ptr() for k in _U64_FIELDS})
    lg = FollowerLogC(meta=log.meta.data_ptr(), first_index=log.first_index.data_ptr(),
                      last_index=t["last_index"].data_ptr(), last_term=t["last_term"].data_ptr(),
                      run_start=log.run_start.data_ptr(), run_term=log.run_term.data_ptr())
    ib = FollowerInboxC(M=M, group=inbox.group.data_ptr(), flags=inbox.flags.data_ptr(),
                        term=inbox.term.data_ptr(), index=inbox.index.data_ptr(),
                        aux=inbox.aux.data_ptr())
    setattr(ib, "from", inbox.frm.data_ptr())
    ap = FollowerAppInboxC(commit=app.commit.data_ptr(), ent_off=app.ent_off.data_ptr(),
                           ent_term=app.ent_term.data_ptr(), ent_len=app.ent_len.data_ptr(),
                           E=int(app.E))
    ao = FollowerAppOutC(resp_index=out.resp_index.data_ptr(), resp_hint=out.resp_hint.data_ptr(),
                         resp_log_term=out.resp_log_term.data_ptr(),
                         app_from=out.app_from.data_ptr())
    _lib.call("qb_dev_follower_log_step", C.byref(fg), C.byref(lg), C.byref(ib), C.byref(ap),
              out.resp_type.data_ptr(), out.resp_term.data_ptr(), C.byref(ao),
              out.stop_at.data_ptr(), out.gflags.data_ptr(), out.stats.data_ptr(),
              out.workspace.data_ptr(), out.workspace.numel() * 8, stream)
    out.inbox = inbox
    return out


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
