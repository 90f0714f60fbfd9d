"""CPU restatement of qb_dev_ingest_follower (include/quorum_batch.h) — TEST
INFRASTRUCTURE ONLY: raw raftpb.Message bytes -> the follower steps' inbox,
statement by statement over oracle/raftpb_ref.unmarshal (Message.Unmarshal,
raft.pb.go:1739-2061, which returns every Entry's fields).  The entries' byte
range is found by walking the message's top-level fields with the oracle's
own ``_varint`` / ``_len_field`` / ``skip_raft``.

Classification is raft.Step's for what a non-leader receives
(raft.go:847-984): MsgHeartbeat, MsgVote / MsgPreVote, MsgTimeoutNow and
MsgApp become records, every other type a FIN_HOST record.
"""
from __future__ import annotations

import numpy as np

from oracle import raftpb_ref as W

OK, UNMARSHAL, TYPE, CTX, ENTRIES, NO_SPACE = range(6)
STATUS_COUNT = 6
FIN_HEARTBEAT, FIN_VOTE, FIN_PREVOTE, FIN_TIMEOUT_NOW, FIN_HOST, FIN_APP = range(6)
FORCE = 0x80
MSG_APP, MSG_VOTE, MSG_HEARTBEAT, MSG_TIMEOUT_NOW, MSG_PREVOTE = 3, 5, 8, 14, 17
CAMPAIGN_TRANSFER = b"CampaignTransfer"  # raft.go:854 campaignTransfer
NO_GROUP = 0xFFFFFFFF
M64 = W.M64

COLUMNS = (("group", np.uint32), ("flags", np.uint8), ("frm", np.uint64), ("term", np.uint64),
           ("index", np.uint64), ("aux", np.uint64), ("commit", np.uint64), ("status", np.uint8),
           ("msg_type", np.uint8), ("ent_pos", np.uint64), ("ent_bytes", np.uint32),
           ("ent_n", np.uint32))


def entry_ranges(b: bytes, i: int = 0, l: int = None):
    """[(pre, post)] of the field-7 fields of a message that unmarshals, key
    and length included, in order (the top-level walk of Message.Unmarshal)."""
    if l is None:
        l = len(b)
    out = []
    schema = W.SCHEMAS["Message"]
    while i < l:
        pre = i
        wire, i = W._varint(b, i, l)
        fnum = W._int32(wire >> 3)
        kind = schema.get(fnum)
        if kind is None:
            i = W.skip_raft(b, pre, l)
        elif kind == "v":
            _, i = W._varint(b, i, l)
        else:
            _, i = W._len_field(b, i, l)
            if fnum == 7:
                out.append((pre, i))
    return out


def _record(status, group=NO_GROUP, flags=0, frm=0, term=0, index=0, aux=0, commit=0, msg_type=0,
            ent_pos=0, ent_bytes=0, ent_n=0, runs=()):
    return dict(status=status, group=group, flags=flags, frm=frm, term=term, index=index, aux=aux,
                commit=commit, msg_type=msg_type, ent_pos=ent_pos, ent_bytes=ent_bytes,
                ent_n=ent_n, runs=list(runs))


def term_runs(terms):
    """[(term, length)] with adjacent runs differing."""
    runs = []
    for t in terms:
        if runs and runs[-1][0] == t:
            runs[-1][1] += 1
        else:
            runs.append([t, 1])
    return [(t, n) for t, n in runs]


def decode(b: bytes, group: int) -> dict:
    """One message -> its record (ent_pos relative to the message's start;
    ``runs`` = the term runs a FIN_APP record carries)."""
    try:
        f = W.unmarshal("Message", b)
    except W.WireError:
        return _record(UNMARSHAL)
    t = f.get(1, 0) & 0xFFFFFFFF  # MessageType is an int32
    frm, term = f.get(3, 0), f.get(4, 0)
    host = dict(group=group, flags=FIN_HOST, frm=frm, term=term, msg_type=t & 0xFF)
    ctx = f.get(12) or b""  # nil and empty are one
    if t == MSG_HEARTBEAT:
        if len(ctx) == 0 or (len(ctx) == 8 and any(ctx)):
            return _record(OK, **dict(host, flags=FIN_HEARTBEAT, index=f.get(8, 0),
                                      aux=int.from_bytes(ctx, "big") if ctx else 0))
        return _record(CTX, **host)
    if t in (MSG_VOTE, MSG_PREVOTE):
        kind = FIN_VOTE if t == MSG_VOTE else FIN_PREVOTE
        force = FORCE if ctx == CAMPAIGN_TRANSFER else 0
        return _record(OK, **dict(host, flags=kind | force, index=f.get(6, 0), aux=f.get(5, 0)))
    if t == MSG_TIMEOUT_NOW:
        return _record(OK, **dict(host, flags=FIN_TIMEOUT_NOW))
    if t == MSG_APP:
        ents = f.get(7, [])
        rng = entry_ranges(b)
        assert len(rng) == len(ents)
        app = dict(host, index=f.get(6, 0), aux=f.get(5, 0), commit=f.get(8, 0), ent_n=len(ents))
        contiguous = all(rng[k][1] == rng[k + 1][0] for k in range(len(rng) - 1))
        consecutive = all(e.get(3, 0) == (app["index"] + 1 + k) & M64 for k, e in enumerate(ents))
        if not (contiguous and consecutive):
            return _record(ENTRIES, **app)
        pos, nb = (rng[0][0], rng[-1][1] - rng[0][0]) if rng else (0, 0)
        return _record(OK, **dict(app, flags=FIN_APP, ent_pos=pos, ent_bytes=nb,
                                  runs=term_runs(e.get(2, 0) for e in ents)))
    return _record(TYPE, **host)


def ingest(buf: bytes, nbytes: int, msg_off, msg_group, ent_cap: int = None) -> dict:
    """The batch: every column of qb_follower_wire_out as numpy arrays, plus
    ``ent_off`` [M+1], ``runs`` (per message: the (term, length) list written
    at ent_off[i], empty where none is), ``ent_total`` and ``stats`` [6]."""
    M = len(msg_group)
    recs = []
    for i in range(M):
        p0, p1 = int(msg_off[i]), int(msg_off[i + 1])
        if not (p0 <= p1 <= nbytes):
            recs.append(_record(UNMARSHAL))
            continue
        r = decode(bytes(buf[p0:p1]), int(msg_group[i]))
        if r["ent_bytes"]:
            r["ent_pos"] += p0
        recs.append(r)
    ent_off = np.zeros(M + 1, np.uint32)
    ent_off[1:] = np.cumsum([len(r["runs"]) for r in recs], dtype=np.uint64)
    total = int(ent_off[M])
    cap = total if ent_cap is None else ent_cap
    for i, r in enumerate(recs):
        if r["runs"] and int(ent_off[i + 1]) > cap:
            r.update(status=NO_SPACE, flags=FIN_HOST, runs=[])
    out = {k: np.array([r[k] for r in recs], dt) for k, dt in COLUMNS}
    out["ent_off"] = ent_off
    out["runs"] = [r["runs"] for r in recs]
    out["ent_total"] = total
    out["stats"] = np.bincount(out["status"], minlength=STATUS_COUNT).astype(np.uint64)
    return out
