"""CPU restatement of the batched Message.Marshal (include/quorum_batch.h
``qb_dev_encode_*``) — TEST INFRASTRUCTURE ONLY.

Follows the reference statement by statement: raft.send (raft.go:386-419),
sendHeartbeat (495-511), maybeSendAppend's MsgApp (471-475), sendTimeoutNow
(1722-1724), responseToReadIndexReq (1745-1750), Message.Size
(raftpb/raft.pb.go:1235-1263) and MarshalToSizedBuffer (903-972).  The bytes
come from oracle/raftpb_ref.marshal_message / marshal_entry (pinned to
Google's protobuf runtime in tests/test_wire_oracle.py and
tests/test_encode_ref.py).

A message is a dict {type, to, frm, term, log_term, index, commit, reject,
reject_hint, ctx (the 8-byte big-endian id as an int, 0 = nil), n_entries};
every front end yields (status, message or None) per position and ``finish``
lays them out as the device does.
"""
from __future__ import annotations

import numpy as np

from oracle import raftpb_ref as W

OK, ENTRIES, HOST, NONE, NO_SPACE = 0, 1, 2, 3, 4
MAX_BYTES = 111
MSG_APP, MSG_SNAP, MSG_HEARTBEAT, MSG_TIMEOUT_NOW = 3, 7, 8, 14
MSG_READ_INDEX, MSG_READ_INDEX_RESP, READ_STATE = 15, 16, 255
MSG_PROP, MSG_VOTE, MSG_VOTE_RESP, MSG_PRE_VOTE, MSG_PRE_VOTE_RESP = 2, 5, 6, 17, 18
MAX_SLOTS = 16
BOUNDARY = (0, 1, 127, 128, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, (1 << 64) - 1)


def message(type=0, to=0, frm=0, term=0, log_term=0, index=0, commit=0, reject=0, reject_hint=0,
            ctx=0, n_entries=0) -> dict:
    return dict(type=int(type), to=int(to), frm=int(frm), term=int(term), log_term=int(log_term),
                index=int(index), commit=int(commit), reject=int(reject),
                reject_hint=int(reject_hint), ctx=int(ctx), n_entries=int(n_entries))


# ------------------------------------------------------------ the bytes ---

def sov(x: int) -> int:
    """sovRaft (raft.pb.go:1354-1356)."""
    return ((x | 1).bit_length() + 6) // 7


def context_of(m: dict):
    """(entries, context) of a message as the project carries request ids: the
    two read types hold it as one Entry{Data: id} (responseToReadIndexReq hands
    req.Entries back, raft.go:1749; the request is forwarded whole,
    raft.go:1445-1470), everything else as Context; 0 is nil."""
    if m["ctx"] == 0:
        return (), None
    data = m["ctx"].to_bytes(8, "big")
    if m["type"] in (MSG_READ_INDEX, MSG_READ_INDEX_RESP):
        return (W.marshal_entry(data=data),), None
    return (), data


def size(m: dict) -> int:
    """Message.Size (raft.pb.go:1235-1263) without the host's entries."""
    entries, context = context_of(m)
    n = 0
    n += 1 + sov(m["type"])
    n += 1 + sov(m["to"])
    n += 1 + sov(m["frm"])
    n += 1 + sov(m["term"])
    n += 1 + sov(m["log_term"])
    n += 1 + sov(m["index"])
    for e in entries:
        l = len(e)
        n += 1 + l + sov(l)
    n += 1 + sov(m["commit"])
    l = len(W.EMPTY_SNAPSHOT)
    n += 1 + l + sov(l)
    n += 2
    n += 1 + sov(m["reject_hint"])
    if context is not None:
        l = len(context)
        n += 1 + l + sov(l)
    return n


def marshal(m: dict, entries=None) -> bytes:
    """Message.Marshal (raft.pb.go:888-972).  ``entries``: the host's encoded
    entries of a MsgApp (the device never sees them)."""
    own, context = context_of(m)
    return W.marshal_message(m["type"], m["to"], m["frm"], m["term"], m["log_term"], m["index"],
                             own if entries is None else entries, m["commit"], W.EMPTY_SNAPSHOT,
                             bool(m["reject"]), m["reject_hint"], context)


def ent_at(m: dict) -> int:
    """The offset just behind the Index field: where field 7 goes."""
    return 6 + sum(sov(m[k]) for k in ("type", "to", "frm", "term", "log_term", "index"))


def splice(b: bytes, at: int, entries) -> bytes:
    """What the host does with a QB_ENC_ENTRIES message: its encoded entries
    go in at ent_at, each as field 7 (raft.pb.go:939-951)."""
    mid = b"".join(b"\x3a" + W.varint(len(e)) + e for e in entries)
    return b[:at] + mid + b[at:]


# -------------------------------------------------------------- raft.send ---

def send(r_id: int, r_term: int, m: dict) -> dict:
    """raft.send (raft.go:386-419) on a copy of m."""
    m = dict(m)
    if m["frm"] == 0:
        m["frm"] = r_id
    if m["type"] in (MSG_VOTE, MSG_VOTE_RESP, MSG_PRE_VOTE, MSG_PRE_VOTE_RESP):
        if m["term"] == 0:
            raise ValueError(f"term should be set when sending {m['type']}")
    else:
        if m["term"] != 0:
            raise ValueError(f"term should not be set when sending {m['type']}")
        if m["type"] not in (MSG_PROP, MSG_READ_INDEX):
            m["term"] = r_term
    return m


def form(r_id, r_term, mtype, to, index, log_term, commit, n, ctx):
    """What the group front ends form of a type and its operands: (status,
    message)."""
    if mtype == MSG_APP:  # maybeSendAppend, raft.go:471-475
        m = message(type=MSG_APP, to=to, index=index, log_term=log_term, commit=commit,
                    n_entries=n)
    elif mtype == MSG_HEARTBEAT:  # sendHeartbeat, raft.go:503-508
        m = message(type=MSG_HEARTBEAT, to=to, commit=commit, ctx=ctx)
    elif mtype == MSG_TIMEOUT_NOW:  # raft.go:1723
        m = message(type=MSG_TIMEOUT_NOW, to=to)
    elif mtype == MSG_READ_INDEX_RESP:  # responseToReadIndexReq, raft.go:1745-1750
        m = message(type=MSG_READ_INDEX_RESP, to=to, index=index, ctx=ctx)
    else:
        return HOST, None
    m = send(r_id, r_term, m)
    return (ENTRIES if m["n_entries"] else OK), m


# ------------------------------------------------------------- front ends ---

def _col(cols, k, i):
    c = cols.get(k)
    return 0 if c is None else int(c[i])


def columns(cols: dict, M: int):
    """qb_dev_encode_messages: every field explicit, a missing column is 0."""
    out = []
    for i in range(M):
        t = int(cols["type"][i])
        if t == 0:
            out.append((NONE, None))
        elif t == MSG_SNAP:
            out.append((HOST, None))
        else:
            m = message(type=t, to=_col(cols, "to", i), frm=_col(cols, "from", i),
                        term=_col(cols, "term", i), log_term=_col(cols, "log_term", i),
                        index=_col(cols, "index", i), commit=_col(cols, "commit", i),
                        reject=1 if _col(cols, "reject", i) else 0,
                        reject_hint=_col(cols, "reject_hint", i), ctx=_col(cols, "context", i),
                        n_entries=_col(cols, "n_entries", i))
            read = t in (MSG_READ_INDEX, MSG_READ_INDEX_RESP)
            out.append((ENTRIES if m["n_entries"] and not read else OK, m))
    return out


def _slots_of(off, g):
    s0, s1 = int(off[g]), int(off[g + 1])
    return s0, (min(s1 - s0, MAX_SLOTS) if s1 > s0 else 0)


def msg_out(G, off, ids, self_id, term, msgs, msg_cap: int, msg_total=None):
    """qb_dev_encode_msg_out over MSG_DTYPE records."""
    out = []
    for i in range(msg_cap):
        if msg_total is not None and i >= msg_total:
            out.append((NONE, None))
            continue
        r = msgs[i]
        t, to, g = int(r["type"]), int(r["to"]), int(r["group"])
        if t in (0, READ_STATE) or to == 0xFF or g >= G:
            out.append((NONE, None))
            continue
        s0, n = _slots_of(off, g)
        if to >= n:
            out.append((NONE, None))
            continue
        out.append(form(int(self_id[g]), int(term[g]), t, int(ids[s0 + to]), int(r["index"]),
                        int(r["log_term"]), int(r["commit"]), int(r["aux"]), int(r["aux"])))
    return out


def slots(G, off, ids, self_id, term, S: int, gflags=None, gmask=0xFF, type_all=MSG_HEARTBEAT,
          cols=None):
    """qb_dev_encode_slots: message s belongs to slot s."""
    cols = cols or {}
    out = [(NONE, None)] * S
    for g in range(G):
        s0, n = _slots_of(off, g)
        if gflags is not None and not (int(gflags[g]) & gmask):
            continue
        for s in range(s0, min(s0 + n, S)):
            t = int(cols["type"][s]) if cols.get("type") is not None else type_all
            if t in (0, READ_STATE):
                continue
            to = int(ids[s])
            if to == int(self_id[g]):
                continue
            commit = (int(cols["commit"][s]) if cols.get("commit") is not None
                      else _col(cols, "commit_g", g))
            out[s] = form(int(self_id[g]), int(term[g]), t, to, _col(cols, "index", s),
                          _col(cols, "log_term", s), commit, _col(cols, "n_entries", s),
                          _col(cols, "ctx_g", g))
    return out


# ----------------------------------------------------------------- layout ---

def finish(recs, cap=None):
    """(status, message) per position -> dict(bytes, msg_off [M+1] u64, status
    u8, ent_at (int, -1 = not written), nbytes, stats [5]) as the device lays
    them out: a message whose end lies past cap gets NO_SPACE and no bytes."""
    M = len(recs)
    off = np.zeros(M + 1, np.uint64)
    status = np.zeros(M, np.uint8)
    at = np.full(M, -1, np.int64)
    parts, pos = [], 0
    written = 0
    for i, (st, m) in enumerate(recs):
        off[i] = pos
        if st <= ENTRIES:
            b = marshal(m)
            assert len(b) == size(m) <= MAX_BYTES
            pos += len(b)
            if cap is not None and pos > cap:
                st = NO_SPACE
            else:
                parts.append(b)
                written = pos
                at[i] = ent_at(m)
        status[i] = st
    off[M] = pos
    stats = np.bincount(status, minlength=5).astype(np.uint64)
    return dict(bytes=np.frombuffer(b"".join(parts), np.uint8), written=written, msg_off=off,
                status=status, ent_at=at, nbytes=pos, stats=stats)
