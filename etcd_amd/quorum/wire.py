"""Wire ingest (include/quorum_batch.h ``qb_dev_ingest_messages``): raw
protobuf raftpb.Message bytes (raft/raftpb/raft.proto:68-86) decoded on the
device into leader-inbox records for ``LeaderGroups.step``.  Validation is
the generated gogoproto Message.Unmarshal (raftpb/raft.pb.go:1739-2061)."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from .. import _lib
from ._checks import check_tensors as _check_tensors
from ._dev import grow_workspace, stream_handle
from .leader import LeaderInbox

WIRE_OK, WIRE_UNMARSHAL, WIRE_TYPE, WIRE_CTX = 0, 1, 2, 3
WIRE_ENTRIES, WIRE_NO_SPACE = 4, 5  # ingest_follower only
WIRE_FOLLOWER_STAT_NAMES = ("ok", "unmarshal", "type", "ctx", "entries", "no_space")
REC_NO_PROGRESS = 0x40


def pack_messages(msgs, groups, device="cuda"):
    """Host helper: a list of encoded messages and their envelope groups ->
    (bytes u8, msg_off int64 [M+1], msg_group int32) device tensors."""
    off = np.zeros(len(msgs) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    buf = np.frombuffer(b"".join(msgs), np.uint8) if msgs else np.zeros(0, np.uint8)
    dev = torch.device(device)
    b = torch.from_numpy(buf.copy() if buf.size else np.zeros(1, np.uint8)).to(dev)
    return (b, int(off[-1]), torch.from_numpy(off.view(np.int64).copy()).to(dev),
            torch.from_numpy(np.asarray(groups, np.uint32).view(np.int32).copy()).to(dev))


def group_rows(off: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """The 64-byte group-row table of a CSR slot-ID config
    (qb_dev_wire_group_rows): build once per config, pass to ``ingest(rows=)``."""
    G = off.numel() - 1
    rows = torch.empty(max(G, 1) * 8, dtype=torch.int64, device=off.device)
    _lib.call("qb_dev_wire_group_rows", G, off.data_ptr(), ids.data_ptr(), rows.data_ptr(),
              stream_handle(off.device))
    return rows


def _check_batch(buf, nbytes, msg_off, msg_group):
    """The message batch: nbytes >= 0 bytes of buf, M + 1 offsets, M groups."""
    if not isinstance(nbytes, int) or nbytes < 0:
        raise _lib.QuorumBatchError(f"nbytes must be a non-negative int, got {nbytes!r}")
    M = msg_group.numel() if isinstance(msg_group, torch.Tensor) else 0
    _check_tensors(((buf, "buf", (torch.uint8,), nbytes),
                    (msg_off, "msg_off", (torch.int64,), M + 1),
                    (msg_group, "msg_group", (torch.int32,), 0)))


def ingest(buf: torch.Tensor, nbytes: int, msg_off: torch.Tensor, msg_group: torch.Tensor,
           off: torch.Tensor, ids: torch.Tensor, stats: torch.Tensor = None,
           rows: torch.Tensor = None):
    """Decode M = len(msg_group) messages.  ``off`` [G+1] int32 and ``ids``
    [off[G]] int64 are the groups' CSR slot IDs (ascending per group); with
    ``rows`` (``group_rows(off, ids)``) each message gathers one 64-byte row
    instead (qb_dev_ingest_messages_rows).
    Returns (LeaderInbox, status u8 tensor, msg_type u8 tensor)."""
    _check_batch(buf, nbytes, msg_off, msg_group)
    _check_tensors(((off, "off", (torch.int32,), 1), (ids, "ids", (torch.int64,), 0),
                    (stats, "stats", (torch.int64,), 4)))
    dev = buf.device
    M = msg_group.numel()
    G = off.numel() - 1
    _check_tensors(((rows, "rows", (torch.int64,), 8 * G), (buf, "buf", (torch.uint8,), 0),
                    (off, "off", (torch.int32,), 0)))
    n = max(M, 1)
    rg = torch.empty(n, dtype=torch.int32, device=dev)
    rf = torch.empty(n, dtype=torch.uint8, device=dev)
    ri, rt, rh, rl = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(4))
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    mtype = torch.empty(n, dtype=torch.uint8, device=dev)
    if rows is None:
        _lib.call("qb_dev_ingest_messages", M, buf.data_ptr(), nbytes, msg_off.data_ptr(),
                  msg_group.data_ptr(), G, off.data_ptr(), ids.data_ptr(), rg.data_ptr(),
                  rf.data_ptr(), ri.data_ptr(), rt.data_ptr(), rh.data_ptr(), rl.data_ptr(),
                  status.data_ptr(), mtype.data_ptr(),
                  None if stats is None else stats.data_ptr(),
                  stream_handle(dev))
    else:
        _lib.call("qb_dev_ingest_messages_rows", M, buf.data_ptr(), nbytes, msg_off.data_ptr(),
                  msg_group.data_ptr(), G, rows.data_ptr(), ids.data_ptr(), rg.data_ptr(),
                  rf.data_ptr(), ri.data_ptr(), rt.data_ptr(), rh.data_ptr(), rl.data_ptr(),
                  status.data_ptr(), mtype.data_ptr(),
                  None if stats is None else stats.data_ptr(),
                  stream_handle(dev))
    ib = LeaderInbox(rg, rf, ri, rt, rh, rl)
    ib._m = M
    return ib, status[:M], mtype[:M]


def ingest_tracker_step(tracker, buf: torch.Tensor, nbytes: int, msg_off: torch.Tensor,
                        msg_group: torch.Tensor, rows: torch.Tensor = None,
                        off: torch.Tensor = None, ids: torch.Tensor = None,
                        advanced_out: torch.Tensor = None, wire_stats: torch.Tensor = None,
                        reset_stats: bool = True, rearm: bool = True) -> torch.Tensor:
    """The composed tick in one call: M encoded responses decoded and stepped
    into ``tracker``, the commit advanced — ``ingest`` followed by
    ``tracker.step`` on its records, without the record columns between them
    (a message that is not a MsgAppResp steps nothing).  A
    ``batch.FixedTracker`` (qb_dev_ingest_fixed_tracker_step: ``rows``
    (``group_rows``) or ``off`` + ``ids`` give the groups' slot IDs) or a
    ``batch.CsrTracker`` (qb_dev_ingest_csr_tracker_step: ``ids`` over the
    tracker's own ``off``, ``rows`` optional).  ``reset_stats`` / ``rearm``
    as the trackers' ``step``; ``wire_stats`` (int64 [4], nullable)
    accumulates the QB_WIRE_* counts.  Returns the per-message status (u8 [M])."""
    from .batch import CsrTracker
    _check_batch(buf, nbytes, msg_off, msg_group)
    G = tracker.G
    _check_tensors(((buf, "buf", (torch.uint8,), 0), (tracker.committed, "tracker", (torch.int64,), G),
                    (rows, "rows", (torch.int64,), 8 * G),
                    (off, "off", (torch.int32,), G + 1),
                    (ids, "ids", (torch.int64,), 0),
                    (advanced_out, "advanced_out", (torch.uint8, torch.bool), G),
                    (wire_stats, "wire_stats", (torch.int64,), 4)))
    csr = isinstance(tracker, CsrTracker)
    if csr and ids is None:
        raise _lib.QuorumBatchError("ids (the groups' slot IDs over the tracker's off) are required")
    if not csr and rows is None and (off is None or ids is None):
        raise _lib.QuorumBatchError("rows, or off and ids, are required")
    dev = buf.device
    M = msg_group.numel()
    if reset_stats:
        tracker.stats.zero_()
    if rearm:
        tracker.stepdown_at.fill_(-1)
    lib = _lib.load()
    need = (lib.qb_wire_csr_tracker_workspace_bytes(tracker.G, tracker.max_slots, M) if csr
            else lib.qb_wire_fixed_tracker_workspace_bytes(tracker.n, tracker.G, M))
    if need == 0:
        raise _lib.QuorumBatchError(f"batch of {M} messages too large for one call")
    ws = tracker._wire_ws = grow_workspace(getattr(tracker, "_wire_ws", None), need, dev)
    status = torch.empty(max(M, 1), dtype=torch.uint8, device=dev)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    stream = stream_handle(dev)
    state = (p(tracker.term), p(tracker.term_start), p(tracker.match), p(tracker.next),
             p(tracker.active), p(tracker.committed), p(tracker.stepdown_at), p(advanced_out),
             status.data_ptr(), p(wire_stats), p(tracker.stats), ws.data_ptr(), ws.numel(), stream)
    if csr:
        _lib.call("qb_dev_ingest_csr_tracker_step", tracker.G, tracker.max_slots, p(tracker.off),
                  p(tracker.cfg), M, buf.data_ptr(), nbytes, msg_off.data_ptr(),
                  msg_group.data_ptr(), p(rows), p(ids), *state)
    else:
        _lib.call("qb_dev_ingest_fixed_tracker_step", tracker.n, tracker.G, M, buf.data_ptr(),
                  nbytes, msg_off.data_ptr(), msg_group.data_ptr(), p(rows), p(off), p(ids), *state)
    return status[:M]


class FollowerWireOutC(C.Structure):
    """struct qb_follower_wire_out (include/quorum_batch.h)."""
    _fields_ = ([(n, C.c_void_p) for n in ("group", "flags", "from", "term", "index", "aux", "commit",
                                           "status", "msg_type", "ent_pos", "ent_bytes", "ent_n",
                                           "ent_off", "ent_term", "ent_len")] +
                [("ent_cap", C.c_uint64), ("ent_total", C.c_void_p), ("stats", C.c_void_p)])


class FollowerIngest(NamedTuple):
    """What ``ingest_follower`` returns: the two inboxes the follower steps
    take as they are, and the per-message columns beside them."""
    inbox: "FollowerInbox"
    app: "FollowerAppInbox"
    status: torch.Tensor     # uint8 [M] WIRE_*
    msg_type: torch.Tensor   # uint8 [M] the low byte of Message.Type
    ent_pos: torch.Tensor    # int64 [M] the entries' byte range inside buf
    ent_bytes: torch.Tensor  # int32 [M]
    ent_n: torch.Tensor      # int32 [M] the entry count
    ent_total: torch.Tensor  # int64 [1] the runs the batch needs, whatever ent_cap


_follower_ws = {}


def new_follower_out(M: int, ent_cap: int, device) -> FollowerIngest:
    """Fresh output tensors of ``ingest_follower`` for M messages and
    ``ent_cap`` term runs (never empty, so every pointer is valid)."""
    from .follower import FollowerAppInbox, FollowerInbox
    n = max(M, 1)
    e = lambda k, dt: torch.empty(k, dtype=dt, device=device)  # noqa: E731
    ib = FollowerInbox(e(n, torch.int32), e(n, torch.uint8), e(n, torch.int64), e(n, torch.int64),
                       e(n, torch.int64), e(n, torch.int64))
    ib._m = M
    app = FollowerAppInbox(e(n, torch.int64), e(M + 1, torch.int32), e(max(ent_cap, 1), torch.int64),
                           e(max(ent_cap, 1), torch.int32), ent_cap)
    return FollowerIngest(ib, app, e(n, torch.uint8), e(n, torch.uint8), e(n, torch.int64),
                          e(n, torch.int32), e(n, torch.int32), e(1, torch.int64))


def ingest_follower(buf: torch.Tensor, nbytes: int, msg_off: torch.Tensor, msg_group: torch.Tensor,
                    G: int, *, ent_cap: Optional[int] = None, stats: torch.Tensor = None,
                    out: Optional[FollowerIngest] = None, stream=None) -> FollowerIngest:
    """Decode M = len(msg_group) messages to non-leaders into the follower
    steps' inbox (qb_dev_ingest_follower): MsgHeartbeat, MsgVote / MsgPreVote,
    MsgTimeoutNow and MsgApp become records, every other type a FIN_HOST
    record.  ``ent_cap`` is the room for the MsgApp entries' term runs
    (default ``nbytes // 2``, which no batch exceeds: an entry takes two bytes;
    a large batch should pass a tighter one and retry with ``ent_total`` where
    a status is WIRE_NO_SPACE).  ``stats`` (int64 [6], nullable) accumulates
    the WIRE_* counts.  ``G`` is the step's group count; a group >= G is
    passed through and stays the step's bad group.  ``out`` (a
    ``FollowerIngest`` of the caller's tensors, ``out.app.E`` its ent_cap) is
    written in place of fresh tensors and returned as it is."""
    from .follower import MAX_RECORDS
    _check_batch(buf, nbytes, msg_off, msg_group)
    _check_tensors(((buf, "buf", (torch.uint8,), 0), (stats, "stats", (torch.int64,),
                                                     len(WIRE_FOLLOWER_STAT_NAMES))))
    if not isinstance(G, int) or G < 0:
        raise _lib.QuorumBatchError(f"G must be a non-negative int, got {G!r}")
    M = msg_group.numel()
    if M > MAX_RECORDS or nbytes >= 1 << 32:
        raise _lib.QuorumBatchError(f"batch of {M} messages / {nbytes} bytes too large for one call "
                                    "(M <= 2^32 - 2, nbytes < 2^32)")
    dev = buf.device
    if out is None:
        cap = nbytes // 2 if ent_cap is None else ent_cap
        if not isinstance(cap, int) or cap < 0:
            raise _lib.QuorumBatchError(f"ent_cap must be a non-negative int, got {ent_cap!r}")
        o = new_follower_out(M, cap, dev)
    else:
        if ent_cap is not None and ent_cap != out.app.E:
            raise _lib.QuorumBatchError(f"ent_cap {ent_cap} is not out.app.E = {out.app.E}")
        o = out
        if o.inbox.M != M:
            raise _lib.QuorumBatchError(f"out.inbox holds {o.inbox.M} records, the batch {M}")
    ib, app, cap = o.inbox, o.app, o.app.E
    ib.check()
    app.check(M)
    _check_tensors(((buf, "buf", (torch.uint8,), 0), (ib.group, "out.inbox", (torch.int32,), M),
                    (app.commit, "out.app", (torch.int64,), M),
                    (o.status, "status", (torch.uint8,), M), (o.msg_type, "msg_type", (torch.uint8,), M),
                    (o.ent_pos, "ent_pos", (torch.int64,), M),
                    (o.ent_bytes, "ent_bytes", (torch.int32,), M),
                    (o.ent_n, "ent_n", (torch.int32,), M),
                    (o.ent_total, "ent_total", (torch.int64,), 1)))
    for k in ("status", "msg_type", "ent_pos", "ent_bytes", "ent_n", "ent_total"):
        if getattr(o, k) is None:
            raise _lib.QuorumBatchError(f"ingest_follower out: {k} is missing")
    need = int(_lib.fn("qb_wire_follower_scratch_bytes")(M))
    key = (dev, stream_handle(dev, stream))  # one workspace per stream: calls on two may overlap
    ws = _follower_ws[key] = grow_workspace(_follower_ws.get(key), need, dev)
    c = FollowerWireOutC(ib.group.data_ptr(), ib.flags.data_ptr(), ib.frm.data_ptr(),
                         ib.term.data_ptr(), ib.index.data_ptr(), ib.aux.data_ptr(),
                         app.commit.data_ptr(), o.status.data_ptr(), o.msg_type.data_ptr(),
                         o.ent_pos.data_ptr(), o.ent_bytes.data_ptr(), o.ent_n.data_ptr(),
                         app.ent_off.data_ptr(), app.ent_term.data_ptr(), app.ent_len.data_ptr(), cap,
                         o.ent_total.data_ptr(), None if stats is None else stats.data_ptr())
    _lib.call("qb_dev_ingest_follower", M, buf.data_ptr(), nbytes, msg_off.data_ptr(),
              msg_group.data_ptr(), G, C.byref(c), ws.data_ptr(), ws.numel(), key[1])
    if out is not None:
        return out
    return o._replace(status=o.status[:M], msg_type=o.msg_type[:M], ent_pos=o.ent_pos[:M],
                      ent_bytes=o.ent_bytes[:M], ent_n=o.ent_n[:M])


# ------------------------------------------------------ request ingest ---

WIRE_TERM, WIRE_CONF_CHANGE, WIRE_GROUP, WIRE_DEFERRED = 6, 7, 8, 9  # ingest_requests only
RQ_NONE, RQ_PROP, RQ_READ, RQ_TRANSFER, RQ_READ_RESP = range(5)
RWFLAG_TAKEN, RWFLAG_DEFERRED = 1, 2
NO_CONF_CHANGE = 0xFFFFFFFF  # cc_at of a MsgProp without one
SLOT_LOCAL, SLOT_NONE = 0xFF, 0xFE
WIRE_REQUEST_STAT_NAMES = ("ok", "unmarshal", "type", "ctx", "entries", "no_space", "term",
                           "conf_change", "group", "deferred", "taken_props", "taken_reads",
                           "taken_transfers", "read_resps", "entries_taken")

# (field, dtype) of struct qb_request_wire_out, in order: the message-aligned
# columns [M], then the dense ones
_RW_MSG = (("kind", torch.uint8), ("status", torch.uint8), ("group", torch.int32),
           ("from", torch.int64), ("term", torch.int64), ("msg_type", torch.uint8),
           ("slot", torch.uint8), ("ctx", torch.int64), ("index", torch.int64),
           ("ent_n", torch.int32), ("payload", torch.int64), ("ent_pos", torch.int64),
           ("ent_bytes", torch.int32), ("cc_at", torch.int32), ("cc_payload", torch.int64),
           ("cc_leave", torch.uint8), ("rd_k", torch.uint8), ("ent_base", torch.int32))
_RW_DENSE = (("n_reads", torch.uint8, 0), ("rd_ctx", torch.int64, 1), ("rd_from", torch.uint8, 1),
             ("xf_from", torch.uint8, 0), ("xf_term", torch.int64, 0), ("action", torch.uint8, 0),
             ("n_ents", torch.int32, 0), ("g_payload", torch.int64, 0), ("g_cc_at", torch.int32, 0),
             ("g_cc_payload", torch.int64, 0), ("gflags", torch.uint8, 0))


class RequestWireOutC(C.Structure):
    """struct qb_request_wire_out (include/quorum_batch.h)."""
    _fields_ = [(n, C.c_void_p) for n, _ in _RW_MSG] + [(n, C.c_void_p) for n, _, _ in _RW_DENSE] + \
        [("stats", C.c_void_p)]


class RequestIngest(NamedTuple):
    """What ``ingest_requests`` returns: the message-aligned columns ([M];
    ``frm`` is the struct's ``from``), the inboxes the two dense calls take as
    they are — ``request_in`` first, ``propose_in`` second — and ``gflags``."""
    kind: torch.Tensor        # uint8 RQ_*
    status: torch.Tensor      # uint8 WIRE_*
    group: torch.Tensor       # int32
    frm: torch.Tensor         # int64
    term: torch.Tensor        # int64
    msg_type: torch.Tensor    # uint8 the low byte of Message.Type
    slot: torch.Tensor        # uint8 READ / TRANSFER: From's slot, SLOT_LOCAL, SLOT_NONE
    ctx: torch.Tensor         # int64 READ / READ_RESP
    index: torch.Tensor       # int64 READ_RESP
    ent_n: torch.Tensor       # int32 PROP
    payload: torch.Tensor     # int64 PROP
    ent_pos: torch.Tensor     # int64 PROP: the entries' byte range inside buf
    ent_bytes: torch.Tensor   # int32 PROP
    cc_at: torch.Tensor       # int32 PROP: NO_CONF_CHANGE (-1 as stored) = none
    cc_payload: torch.Tensor  # int64 PROP
    cc_leave: torch.Tensor    # uint8 PROP
    rd_k: torch.Tensor        # uint8 a taken READ's row
    ent_base: torch.Tensor    # int32 a taken PROP's first entry within n_ents[g]
    request_in: "RequestInbox"
    propose_in: "ProposeInbox"
    gflags: torch.Tensor      # uint8 [G] RWFLAG_*


_request_ws = {}


def new_request_out(M: int, G: int, max_reads: int, device) -> RequestIngest:
    """Fresh output tensors of ``ingest_requests`` (never empty, so every
    pointer is valid)."""
    from .propose import ProposeInbox
    from .request import RequestInbox
    n, g = max(M, 1), max(G, 1)
    e = lambda k, dt: torch.empty(k, dtype=dt, device=device)  # noqa: E731
    msg = [e(n, dt) for _, dt in _RW_MSG]
    d = {name: e(g * (max_reads if per_read else 1), dt) for name, dt, per_read in _RW_DENSE}
    rin = RequestInbox(max_reads, d["n_reads"], d["rd_ctx"], d["rd_from"], d["xf_from"], d["xf_term"])
    pin = ProposeInbox(d["action"], d["n_ents"], d["g_payload"], d["g_cc_at"], d["g_cc_payload"])
    return RequestIngest(*msg, rin, pin, d["gflags"])


def ingest_requests(buf: torch.Tensor, nbytes: int, msg_off: torch.Tensor, msg_group: torch.Tensor,
                    off: torch.Tensor, ids: torch.Tensor, *, max_reads: int = 1, concat: bool = False,
                    stats: torch.Tensor = None, out: Optional[RequestIngest] = None,
                    stream=None) -> RequestIngest:
    """Decode M = len(msg_group) request messages at the leaders of G =
    len(off) - 1 groups (qb_dev_ingest_requests): MsgProp, MsgReadIndex and
    MsgTransferLeader become the dense inputs of ``leader_requests``
    (``.request_in``, run first) and ``leader_propose`` (``.propose_in``, run
    second); MsgReadIndexResp is decoded for the host.  ``off`` / ``ids`` are
    the groups' CSR slot IDs as for ``ingest``.  ``max_reads`` reads per group
    and call are taken; ``concat`` concatenates a group's proposals into one
    (False: one MsgProp per group and call).  A message behind what the call
    took has status WIRE_DEFERRED and is submitted again.  ``stats`` (int64
    [15], nullable) accumulates WIRE_REQUEST_STAT_NAMES.  ``out`` (a
    ``RequestIngest`` of the caller's tensors) is written in place of fresh
    tensors and returned as it is."""
    from .request import MAX_READS
    _check_batch(buf, nbytes, msg_off, msg_group)
    _check_tensors(((buf, "buf", (torch.uint8,), 0), (off, "off", (torch.int32,), 1),
                    (ids, "ids", (torch.int64,), 0),
                    (stats, "stats", (torch.int64,), len(WIRE_REQUEST_STAT_NAMES))))
    if not isinstance(max_reads, int) or not 1 <= max_reads <= MAX_READS:
        raise _lib.QuorumBatchError(f"max_reads must be 1..{MAX_READS}, got {max_reads!r}")
    M, G = msg_group.numel(), off.numel() - 1
    if M > 0xFFFFFFFE or nbytes >= 1 << 32:
        raise _lib.QuorumBatchError(f"batch of {M} messages / {nbytes} bytes too large for one call "
                                    "(M <= 2^32 - 2, nbytes < 2^32)")
    dev = buf.device
    o = new_request_out(M, G, max_reads, dev) if out is None else out
    rin, pin = o.request_in, o.propose_in
    if rin.max_reads != max_reads:
        raise _lib.QuorumBatchError(f"out.request_in has max_reads {rin.max_reads}, the call {max_reads}")
    dense = {"n_reads": rin.n_reads, "rd_ctx": rin.rd_ctx, "rd_from": rin.rd_from,
             "xf_from": rin.xf_from, "xf_term": rin.xf_term, "action": pin.action,
             "n_ents": pin.n_ents, "g_payload": pin.payload, "g_cc_at": pin.cc_at,
             "g_cc_payload": pin.cc_payload, "gflags": o.gflags}
    cols = [(getattr(o, "frm" if name == "from" else name), name, dt, M) for name, dt in _RW_MSG] + \
        [(dense[name], name, dt, G * (max_reads if per_read else 1)) for name, dt, per_read in _RW_DENSE]
    for t, name, _, _ in cols:
        if t is None:
            raise _lib.QuorumBatchError(f"ingest_requests out: {name} is missing")
    _check_tensors(((buf, "buf", (torch.uint8,), 0),) + tuple((t, name, (dt,), n) for t, name, dt, n in cols))
    need = int(_lib.fn("qb_wire_requests_scratch_bytes")(G, M))
    key = (dev, stream_handle(dev, stream))  # one workspace per stream: calls on two may overlap
    ws = _request_ws[key] = grow_workspace(_request_ws.get(key), need, dev)
    c = RequestWireOutC(*[t.data_ptr() for t, _, _, _ in cols], None if stats is None else stats.data_ptr())
    _lib.call("qb_dev_ingest_requests", M, buf.data_ptr(), nbytes, msg_off.data_ptr(),
              msg_group.data_ptr(), G, off.data_ptr(), ids.data_ptr(), max_reads, 1 if concat else 0,
              C.byref(c), ws.data_ptr(), ws.numel(), key[1])
    if out is not None:
        return out
    fields = ["frm" if name == "from" else name for name, _ in _RW_MSG]
    return o._replace(**{k: getattr(o, k)[:M] for k in fields})


# ------------------------------------------------------- workload synth ---

def _vfix(v: np.ndarray, n: int) -> np.ndarray:
    """Varints of exactly n bytes (v must need exactly n bytes)."""
    v = v.astype(np.uint64)
    out = np.empty((v.size, n), np.uint8)
    for k in range(n):
        b = ((v >> np.uint64(7 * k)) & np.uint64(0x7F)).astype(np.uint8)
        out[:, k] = b | (0x80 if k < n - 1 else 0)
    return out


_EMPTY_SNAPSHOT = bytes([0x12, 0x08, 0x0A, 0x02, 0x28, 0x00, 0x10, 0x00, 0x18, 0x00])
# Snapshot{Metadata{ConfState{AutoLeave:false}, Index:0, Term:0}} as gogoproto
# writes it (non-nullable fields always present).


def synth_response_stream(M: int, G: int, seed: int = 0x5EED0008, hb_frac: float = 0.1):
    """Host bytes of M gogoproto-encoded responses to G 5-voter leaders (the
    wire-ingest bench workload): MsgAppResp (10% rejected) and, with
    probability hb_frac, MsgHeartbeatResp carrying an 8-byte read context.
    Node IDs, terms and indexes are sized so every message of a kind has the
    same layout (vectorised construction).  Returns (bytes ndarray u8,
    msg_off u64 [M+1], msg_group u32 [M], off u32 [G+1], ids u64 [5G])."""
    rng = np.random.default_rng(seed)
    grp = rng.integers(0, G, M).astype(np.uint32)
    slot = rng.integers(1, 5, M).astype(np.uint64)
    g64 = grp.astype(np.uint64)
    frm = np.uint64(16384) + slot * np.uint64(200000) + (g64 % np.uint64(100000))
    to = np.uint64(16384) + (g64 % np.uint64(100000))
    term = np.full(M, 20000, np.uint64)
    index = np.uint64(1 << 35) + g64 * np.uint64(64) + rng.integers(0, 64, M).astype(np.uint64)
    reject = rng.random(M) < 0.1
    hb = rng.random(M) < hb_frac
    ctx = (np.uint64(1) << np.uint64(56)) + rng.integers(1, 1 << 40, M).astype(np.uint64)

    def col(byte):
        return np.full((M, 1), byte, np.uint8)
    app = np.concatenate([
        col(0x08), col(4), col(0x10), _vfix(to, 3), col(0x18), _vfix(frm, 3), col(0x20),
        _vfix(term, 3), col(0x28), col(0), col(0x30), _vfix(index, 6), col(0x40), col(0),
        col(0x4A), col(len(_EMPTY_SNAPSHOT)),
        np.tile(np.frombuffer(_EMPTY_SNAPSHOT, np.uint8), (M, 1)),
        col(0x50), reject.astype(np.uint8)[:, None], col(0x58), col(0)], axis=1)
    ctxb = ((ctx[:, None] >> (np.arange(7, -1, -1, dtype=np.uint64) * np.uint64(8)))
            & np.uint64(0xFF)).astype(np.uint8)
    hbm = np.concatenate([
        col(0x08), col(9), col(0x10), _vfix(to, 3), col(0x18), _vfix(frm, 3), col(0x20),
        _vfix(term, 3), col(0x28), col(0), col(0x30), col(0), col(0x40), col(0),
        col(0x4A), col(len(_EMPTY_SNAPSHOT)),
        np.tile(np.frombuffer(_EMPTY_SNAPSHOT, np.uint8), (M, 1)),
        col(0x50), col(0), col(0x58), col(0), col(0x62), col(8), ctxb], axis=1)
    la, lh = app.shape[1], hbm.shape[1]
    lens = np.where(hb, lh, la).astype(np.uint64)
    moff = np.zeros(M + 1, np.uint64)
    np.cumsum(lens, out=moff[1:])
    buf = np.empty(int(moff[-1]), np.uint8)
    for sel, t, L_ in ((~hb, app, la), (hb, hbm, lh)):
        pos = moff[:-1][sel].astype(np.int64)
        buf[(pos[:, None] + np.arange(L_)).reshape(-1)] = t[sel].reshape(-1)
    off = (np.arange(G + 1, dtype=np.uint32) * 5).astype(np.uint32)
    gg = np.repeat(np.arange(G, dtype=np.uint64), 5)
    ss = np.tile(np.arange(5, dtype=np.uint64), G)
    ids = np.uint64(16384) + ss * np.uint64(200000) + (gg % np.uint64(100000))
    return buf, moff, grp, off, ids


def _dev_varint(v: torch.Tensor, n: int) -> list:
    """Varint bytes (exactly n) of an int64 device tensor, one u8 column each."""
    cols = []
    for k in range(n):
        b = (v >> (7 * k)) & 0x7F
        if k < n - 1:
            b = b | 0x80
        cols.append(b.to(torch.uint8))
    return cols


def encode_appresp(to: torch.Tensor, frm: torch.Tensor, term: torch.Tensor,
                   index: torch.Tensor, reject: torch.Tensor):
    """Device-side gogoproto encoding of M MsgAppResp messages with one fixed
    layout (raft.pb.go Message.Marshal field order: Type, To, From, Term,
    LogTerm 0, Index, Commit 0, the empty non-nullable Snapshot, Reject,
    RejectHint 0) — the composed wire -> tracker workload's generator.  Node
    IDs and terms must need 3-byte varints ([2^14, 2^21)), indexes 6-byte
    ones ([2^35, 2^42)).  Returns (bytes u8, nbytes, msg_off int64 [M+1])."""
    lo, hi = 1 << 14, 1 << 21
    for t, what, a, b in ((to, "to", lo, hi), (frm, "frm", lo, hi), (term, "term", lo, hi),
                          (index, "index", 1 << 35, 1 << 42)):
        if t.numel() and (int(t.min()) < a or int(t.max()) >= b):
            raise ValueError(f"encode_appresp: {what} outside [{a}, {b})")
    M = to.numel()
    dev = to.device

    def col(byte):
        return torch.full((M,), byte, dtype=torch.uint8, device=dev)
    cols = [col(0x08), col(4), col(0x10), *_dev_varint(to, 3), col(0x18), *_dev_varint(frm, 3),
            col(0x20), *_dev_varint(term, 3), col(0x28), col(0), col(0x30),
            *_dev_varint(index, 6), col(0x40), col(0), col(0x4A), col(len(_EMPTY_SNAPSHOT))]
    cols += [col(b) for b in _EMPTY_SNAPSHOT]
    cols += [col(0x50), reject.to(torch.uint8), col(0x58), col(0)]
    L = len(cols)
    buf = torch.stack(cols, dim=1).reshape(-1)
    moff = torch.arange(M + 1, dtype=torch.int64, device=dev) * L
    return buf, M * L, moff
