"""Batched raftpb.Message Marshal of the outboxes (include/quorum_batch.h
``qb_dev_encode_messages``, ``qb_dev_encode_msg_out``, ``qb_dev_encode_slots``).

The sending side of ``wire.ingest``: the messages the step calls leave as
records and slot-aligned columns become gogoproto bytes on the device, bit for
bit Message.Marshal (raftpb/raft.pb.go:903-972, 1235-1263), with raft.send's
From / Term (raft.go:386-419) in the two group front ends.  Entry payloads and
snapshots stay the host's: INTEGRATION.md, "Sending: what the host does per
status".  The encoder runs in the HIP library; torch only holds device memory.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import torch

from .. import _lib
from ._checks import I32, I64, U8, check_tensors
from ._dev import grow_workspace, stats_dict, stream_handle

ENC_OK, ENC_ENTRIES, ENC_HOST, ENC_NONE, ENC_NO_SPACE = 0, 1, 2, 3, 4
ENC_MAX_BYTES = 111
ENC_STAT_NAMES = ("ok", "entries", "host", "none", "no_space")
MSG_APP, MSG_SNAP, MSG_HEARTBEAT, MSG_TIMEOUT_NOW, MSG_READ_INDEX_RESP = 3, 7, 8, 14, 16
MSG_READ_INDEX, READ_STATE = 15, 255
MSG_OUT_BYTES = 40  # sizeof(qb_msg_out)

_P = C.c_void_p
_COLS = ("type", "to", "from", "term", "log_term", "index", "commit", "reject_hint", "reject",
         "context", "n_entries")
_U8_COLS = ("type", "reject")
_SLOT_COLS = ("type", "index", "log_term", "commit", "n_entries")  # [S]
_SLOT_GCOLS = ("commit_g", "ctx_g")                                # [G]


class EncodeOutC(C.Structure):
    """struct qb_encode_out (include/quorum_batch.h)."""
    _fields_ = [("bytes", _P), ("cap", C.c_uint64), ("msg_off", _P), ("status", _P),
                ("ent_at", _P), ("nbytes", _P), ("stats", _P)]


class EncodeColsC(C.Structure):
    """struct qb_encode_cols."""
    _fields_ = [(n, _P) for n in _COLS]


class EncodeGroupsC(C.Structure):
    """struct qb_encode_groups."""
    _fields_ = [("G", C.c_uint64)] + [(n, _P) for n in ("off", "ids", "self_id", "term")]


class EncodeSlotColsC(C.Structure):
    """struct qb_encode_slot_cols."""
    _fields_ = [("S", C.c_uint64), ("gflags", _P), ("gmask", C.c_uint32), ("type_all", C.c_uint32),
                ("type", _P), ("index", _P), ("log_term", _P), ("commit", _P), ("n_entries", _P),
                ("commit_g", _P), ("ctx_g", _P)]


def max_bytes(M: int) -> int:
    """The bytes M messages need at most (ENC_MAX_BYTES each)."""
    return int(M) * ENC_MAX_BYTES


@dataclass
class EncodeGroups:
    """struct qb_encode_groups: the CSR every call already has (``off`` [G+1]
    int32, ``ids`` [S] int64: slot -> raft ID) plus the sender (``self_id`` and
    ``term``, [G] int64)."""
    off: torch.Tensor
    ids: torch.Tensor
    self_id: torch.Tensor
    term: torch.Tensor
    S: int  # off[G], the caller's
    _ws: Optional[torch.Tensor] = field(default=None, repr=False)

    @property
    def G(self) -> int:
        return max(int(self.off.numel()) - 1, 0) if isinstance(self.off, torch.Tensor) else 0

    def struct(self) -> EncodeGroupsC:
        G = self.G
        if self.S < 0:
            raise _lib.QuorumBatchError(f"S must be non-negative, got {self.S}")
        check_tensors(((self.off, "off", I32, G + 1), (self.ids, "ids", I64, self.S),
                       (self.self_id, "self_id", I64, G), (self.term, "term", I64, G)))
        for k in ("off", "ids", "self_id", "term"):
            if getattr(self, k) is None:
                raise _lib.QuorumBatchError(f"encode groups: {k} is missing")
        return EncodeGroupsC(G=G, off=self.off.data_ptr(), ids=self.ids.data_ptr(),
                             self_id=self.self_id.data_ptr(), term=self.term.data_ptr())


@dataclass
class EncodeOut:
    """struct qb_encode_out as device tensors: ``bytes`` uint8 [cap] (any
    alignment: a slice of a larger buffer works), ``msg_off`` int64 [M+1],
    ``status`` uint8 [M], ``ent_at`` int32 [M] (optional), ``nbytes`` int64
    [1], ``stats`` int64 [5] (optional, accumulated)."""
    bytes: torch.Tensor
    cap: int
    msg_off: torch.Tensor
    status: torch.Tensor
    ent_at: Optional[torch.Tensor]
    nbytes: torch.Tensor
    stats: Optional[torch.Tensor] = None

    def stats_dict(self) -> Dict[str, int]:
        return stats_dict(ENC_STAT_NAMES, self.stats)

    def result(self, M: int) -> Tuple[torch.Tensor, ...]:
        return (self.bytes, self.msg_off[:M + 1], self.status[:M],
                None if self.ent_at is None else self.ent_at[:M], self.nbytes)


def new_out(M: int, device, cap: Optional[int] = None) -> EncodeOut:
    """Fresh output buffers for M messages (``cap`` bytes, default
    ``max_bytes(M)``: every batch fits)."""
    cap = max_bytes(M) if cap is None else int(cap)
    z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device=device)  # noqa: E731
    return EncodeOut(torch.empty(max(cap, 1), dtype=torch.uint8, device=device), cap,
                     z(M + 1, torch.int64), z(M, torch.uint8), z(M, torch.int32),
                     z(1, torch.int64), z(len(ENC_STAT_NAMES), torch.int64))


def _out_struct(out: EncodeOut, M: int) -> EncodeOutC:
    if not isinstance(out.cap, int) or out.cap < 0:
        raise _lib.QuorumBatchError(f"cap must be a non-negative int, got {out.cap!r}")
    check_tensors(((out.bytes, "bytes", U8, out.cap), (out.msg_off, "msg_off", I64, M + 1),
                   (out.status, "status", U8, M), (out.ent_at, "ent_at", I32, M),
                   (out.nbytes, "nbytes", I64, 1), (out.stats, "stats", I64, len(ENC_STAT_NAMES))))
    for k in ("bytes", "msg_off", "status", "nbytes"):
        if getattr(out, k) is None:
            raise _lib.QuorumBatchError(f"encode out: {k} is missing")
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    return EncodeOutC(bytes=out.bytes.data_ptr(), cap=out.cap, msg_off=out.msg_off.data_ptr(),
                      status=out.status.data_ptr(), ent_at=p(out.ent_at),
                      nbytes=out.nbytes.data_ptr(), stats=p(out.stats))


def _workspace(holder, M: int, device) -> torch.Tensor:
    need = int(_lib.fn("qb_encode_scratch_bytes")(M))
    if need == 0 and M:
        raise _lib.QuorumBatchError(f"batch of {M} messages too large for one call "
                                    f"(M * {ENC_MAX_BYTES} must stay below 2^32)")
    ws = grow_workspace(getattr(holder, "_ws", None), need, device)
    if holder is not None:
        holder._ws = ws
    return ws


def encode_columns(cols: Dict[str, Optional[torch.Tensor]], *, M: Optional[int] = None,
                   out: Optional[EncodeOut] = None, cap: Optional[int] = None, stream=None):
    """The general form: ``cols`` maps the names of struct qb_encode_cols
    (``type`` uint8, required; ``to`` ``from`` ``term`` ``log_term`` ``index``
    ``commit`` ``reject_hint`` ``context`` ``n_entries`` int64; ``reject``
    uint8) to device tensors of M entries; a missing column reads as 0.  Term is
    taken as given.  Returns (bytes, msg_off, status, ent_at, nbytes tensor)."""
    unknown = set(cols) - set(_COLS)
    if unknown:
        raise _lib.QuorumBatchError(f"encode_columns: unknown column(s) {sorted(unknown)}")
    typ = cols.get("type")
    if typ is None:
        raise _lib.QuorumBatchError("encode_columns: the type column is required")
    check_tensors(((typ, "type", U8, 0),))
    M = int(typ.numel() if M is None else M)
    if M < 0:
        raise _lib.QuorumBatchError(f"M must be non-negative, got {M}")
    check_tensors(tuple((cols.get(k), k, U8 if k in _U8_COLS else I64, M) for k in _COLS))
    dev = typ.device
    if out is None:
        out = new_out(M, dev, cap)
    elif cap is not None:
        out.cap = int(cap)
    check_tensors(((typ, "type", U8, M), (out.bytes, "bytes", U8, 0)))
    oc = _out_struct(out, M)
    ws = _workspace(out, M, dev)
    cc = EncodeColsC(**{k: (None if cols.get(k) is None else cols[k].data_ptr()) for k in _COLS})
    _lib.call("qb_dev_encode_messages", M, C.byref(cc), C.byref(oc), ws.data_ptr(), ws.numel(),
              stream_handle(dev, stream))
    return out.result(M)


def encode_msg_out(groups: EncodeGroups, msgs: torch.Tensor, msg_cap: Optional[int] = None,
                   msg_total: Optional[torch.Tensor] = None, *, out: Optional[EncodeOut] = None,
                   cap: Optional[int] = None, stream=None):
    """``LeaderGroups.step(fetch=False)``'s dense list (``msgs``: uint8, 40
    bytes a record; ``msg_total``: its device count, int64 [1], never copied
    back; None encodes all ``msg_cap``), or an outbox's ``slots`` / ``chunks``
    as flat arrays.  M = ``msg_cap`` (default: the records ``msgs`` holds).
    Returns (bytes, msg_off, status, ent_at, nbytes tensor)."""
    eg = groups.struct()
    check_tensors(((msgs, "msgs", U8, 0),))
    if msgs is None:
        raise _lib.QuorumBatchError("encode_msg_out: msgs is missing")
    M = int(msgs.numel() // MSG_OUT_BYTES if msg_cap is None else msg_cap)
    if M < 0:
        raise _lib.QuorumBatchError(f"msg_cap must be non-negative, got {M}")
    dev = msgs.device
    if out is None:
        out = new_out(M, dev, cap)
    elif cap is not None:
        out.cap = int(cap)
    check_tensors(((msgs, "msgs", U8, M * MSG_OUT_BYTES), (msg_total, "msg_total", I64, 1),
                   (groups.off, "off", I32, 0), (out.bytes, "bytes", U8, 0)))
    oc = _out_struct(out, M)
    ws = _workspace(groups, M, dev)
    _lib.call("qb_dev_encode_msg_out", C.byref(eg), msgs.data_ptr(), M,
              None if msg_total is None else msg_total.data_ptr(), C.byref(oc), ws.data_ptr(),
              ws.numel(), stream_handle(dev, stream))
    return out.result(M)


def encode_slots(groups: EncodeGroups, *, gflags: Optional[torch.Tensor] = None, gmask: int = 0xFF,
                 type_all: int = MSG_HEARTBEAT, cols: Optional[Dict[str, torch.Tensor]] = None,
                 out: Optional[EncodeOut] = None, cap: Optional[int] = None, stream=None):
    """Slot-aligned messages: message s belongs to slot s, M = ``groups.S``.
    A group takes part where ``gflags`` is None or ``gflags[g] & gmask``;
    ``cols`` maps ``type`` (uint8 [S]; None: ``type_all`` everywhere), ``index``
    ``log_term`` ``commit`` ``n_entries`` (int64 [S]) and ``commit_g`` ``ctx_g``
    (int64 [G]) to device tensors.  The tick's broadcast is
    ``encode_slots(g, gflags=tflags, gmask=TFLAG_BEAT, cols={"commit":
    hb_commit, "ctx_g": hb_ctx})``.
    Returns (bytes, msg_off, status, ent_at, nbytes tensor)."""
    cols = dict(cols or {})
    unknown = set(cols) - set(_SLOT_COLS) - set(_SLOT_GCOLS)
    if unknown:
        raise _lib.QuorumBatchError(f"encode_slots: unknown column(s) {sorted(unknown)}")
    eg = groups.struct()
    G, S = groups.G, int(groups.S)
    if not 0 <= int(gmask) <= 0xFF or not 0 <= int(type_all) <= 0xFF:
        raise _lib.QuorumBatchError("encode_slots: gmask and type_all are bytes")
    check_tensors(((groups.off, "off", I32, 0), (gflags, "gflags", U8, G),
                   (cols.get("type"), "type", U8, S)) +
                  tuple((cols.get(k), k, I64, S) for k in _SLOT_COLS[1:]) +
                  tuple((cols.get(k), k, I64, G) for k in _SLOT_GCOLS))
    dev = groups.off.device
    if out is None:
        out = new_out(S, dev, cap)
    elif cap is not None:
        out.cap = int(cap)
    check_tensors(((groups.off, "off", I32, 0), (out.bytes, "bytes", U8, 0)))
    oc = _out_struct(out, S)
    ws = _workspace(groups, S, dev)
    p = lambda k: None if cols.get(k) is None else cols[k].data_ptr()  # noqa: E731
    sc = EncodeSlotColsC(S=S, gflags=None if gflags is None else gflags.data_ptr(),
                         gmask=int(gmask), type_all=int(type_all),
                         **{k: p(k) for k in _SLOT_COLS + _SLOT_GCOLS})
    _lib.call("qb_dev_encode_slots", C.byref(eg), C.byref(sc), C.byref(oc), ws.data_ptr(),
              ws.numel(), stream_handle(dev, stream))
    return out.result(S)
