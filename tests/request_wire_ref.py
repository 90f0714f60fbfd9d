"""CPU restatement of qb_dev_ingest_requests (include/quorum_batch.h) — TEST
INFRASTRUCTURE ONLY: raw raftpb.Message bytes -> the dense inputs of
qb_dev_leader_requests and qb_dev_leader_propose, statement by statement over
oracle/raftpb_ref.unmarshal (Message.Unmarshal, raft.pb.go:1739-2061).  The
three conf-change kinds (ConfChange / ConfChangeSingle / ConfChangeV2.Unmarshal,
raft.pb.go:2543-2908) are decoded by the same ``unmarshal`` over the schemas
below, which tests/golden/request_wire_cases.json pins to the reference's own
descriptor.

Pass 1 classifies each message (stepLeader's MsgProp, raft.go:1019-1077;
MsgReadIndex, raft.go:1078-1097; MsgTransferLeader, raft.go:1339-1372; the
follower's MsgReadIndexResp, raft.go:1465-1470); pass 2 walks each group's
requests in batch order and takes or defers them.
"""
from __future__ import annotations

import numpy as np

from oracle import raftpb_ref as W
from tests.follower_wire_ref import entry_ranges

OK, UNMARSHAL, TYPE, CTX, ENTRIES, NO_SPACE, TERM, CONF_CHANGE, GROUP, DEFERRED = range(10)
RQ_NONE, RQ_PROP, RQ_READ, RQ_TRANSFER, RQ_READ_RESP = range(5)
STAT_TAKEN_PROPS, STAT_TAKEN_READS, STAT_TAKEN_TRANSFERS, STAT_READ_RESPS, STAT_ENTRIES_TAKEN = range(10, 15)
STAT_COUNT = 15
MSG_PROP, MSG_TRANSFER, MSG_READ_INDEX, MSG_READ_INDEX_RESP = 2, 13, 15, 16
ENTRY_CONF_CHANGE, ENTRY_CONF_CHANGE_V2 = 1, 2
PROP_NONE, PROP_ENTRIES, PROP_CONF_CHANGE, PROP_CC_LEAVE_JOINT = 0, 1, 0x40, 0x80
FLAG_TAKEN, FLAG_DEFERRED = 1, 2
NO_GROUP = NO_CC = 0xFFFFFFFF
SLOT_LOCAL, SLOT_NONE = 0xFF, 0xFE
MAX_SLOTS = 16
MAX_ENTS = (1 << 32) - 1

CC_SCHEMAS = {
    "ConfChange": {1: "v", 2: "v", 3: "v", 4: "b"},
    "ConfChangeSingle": {1: "v", 2: "v"},
    "ConfChangeV2": {1: "v", 2: ("m", "ConfChangeSingle"), 3: "b"},
}
SCHEMAS = dict(W.SCHEMAS, **CC_SCHEMAS)

COLUMNS = (("kind", np.uint8), ("status", np.uint8), ("group", np.uint32), ("frm", np.uint64),
           ("term", np.uint64), ("msg_type", np.uint8), ("slot", np.uint8), ("ctx", np.uint64),
           ("index", np.uint64), ("ent_n", np.uint32), ("payload", np.uint64), ("ent_pos", np.uint64),
           ("ent_bytes", np.uint32), ("cc_at", np.uint32), ("cc_payload", np.uint64),
           ("cc_leave", np.uint8), ("rd_k", np.uint8), ("ent_base", np.uint32))
DENSE = (("n_reads", np.uint8), ("xf_from", np.uint8), ("xf_term", np.uint64), ("action", np.uint8),
         ("n_ents", np.uint32), ("g_payload", np.uint64), ("g_cc_at", np.uint32),
         ("g_cc_payload", np.uint64), ("gflags", np.uint8))


def _record(status, **kw):
    r = {k: 0 for k, _ in COLUMNS}
    r.update(dict(status=status, group=NO_GROUP), **kw)
    return r


def wants_leave_joint(etype: int, data: bytes):
    """(unmarshals, wantsLeaveJoint) of a conf-change entry's Data
    (raft.go:1034-1053): a V1 always converts to one change (AsV2,
    confchange.go:63-73)."""
    try:
        cc = W.unmarshal("ConfChange" if etype == ENTRY_CONF_CHANGE else "ConfChangeV2", data,
                         schemas=SCHEMAS)
    except W.WireError:
        return False, False
    return True, etype == ENTRY_CONF_CHANGE_V2 and len(cc.get(2, [])) == 0


def slot_of(frm: int, ids) -> int:
    for s, vid in enumerate(list(ids)[:MAX_SLOTS]):
        if int(vid) == frm:
            return s
    return SLOT_NONE


def _read_ctx(ents):
    """The request id of a read or its response: the only entry's Data, 8
    bytes not all zero, big-endian; None for any other shape."""
    if len(ents) != 1:
        return None
    data = ents[0].get(4) or b""
    if len(data) != 8 or not any(data):
        return None
    return int.from_bytes(data, "big")


def decode(b: bytes, group: int, G: int, ids) -> dict:
    """One message -> its pass-1 columns (ent_pos relative to the message's
    start).  ``ids``: the slot IDs of ``group`` (empty where group >= G)."""
    try:
        f = W.unmarshal("Message", b)
    except W.WireError:
        return _record(UNMARSHAL)
    t = f.get(1, 0) & 0xFFFFFFFF  # MessageType is an int32
    frm, term = f.get(3, 0), f.get(4, 0)
    r = _record(OK, group=group, frm=frm, term=term, msg_type=t & 0xFF)
    ents = f.get(7, [])
    if t == MSG_PROP:
        rng = entry_ranges(b)
        assert len(rng) == len(ents)
        whole = len(ents) > 0 and all(rng[k][1] == rng[k + 1][0] for k in range(len(rng) - 1))
        ccs, bad = [], False
        for k, e in enumerate(ents):
            et = W._int32(e.get(1, 0))  # EntryType is an int32
            if et in (ENTRY_CONF_CHANGE, ENTRY_CONF_CHANGE_V2):
                data = e.get(4) or b""
                good, leave = wants_leave_joint(et, data)
                bad |= not good or len(ccs) > 0
                ccs.append((k, len(data), leave))
        r.update(kind=RQ_PROP, ent_n=len(ents), payload=sum(len(e.get(4) or b"") for e in ents),
                 ent_pos=rng[0][0] if whole else 0, ent_bytes=rng[-1][1] - rng[0][0] if whole else 0,
                 cc_at=NO_CC)
        if ccs and not bad:
            r.update(cc_at=ccs[0][0], cc_payload=ccs[0][1], cc_leave=int(ccs[0][2]))
        if term != 0:
            r["status"] = TERM
        elif not whole:
            r["status"] = ENTRIES
        elif bad:
            r["status"] = CONF_CHANGE
    elif t == MSG_READ_INDEX:
        ctx = _read_ctx(ents)
        r.update(kind=RQ_READ, ctx=ctx or 0,
                 slot=SLOT_LOCAL if frm == 0 else (slot_of(frm, ids) if group < G else SLOT_NONE))
        if term != 0:
            r["status"] = TERM
        elif ctx is None:
            r["status"] = CTX
    elif t == MSG_TRANSFER:
        r.update(kind=RQ_TRANSFER, slot=slot_of(frm, ids) if group < G and frm != 0 else SLOT_NONE)
    elif t == MSG_READ_INDEX_RESP:
        ctx = _read_ctx(ents)
        r.update(kind=RQ_READ_RESP, index=f.get(6, 0), ctx=ctx or 0)
        if ctx is None:
            r["status"] = CTX
    else:
        r["status"] = TYPE
    if r["status"] == OK and r["kind"] != RQ_READ_RESP and group >= G:
        r["status"] = GROUP
    return r


def combine(recs, G: int, max_reads: int, concat: bool, defer_behind_prop: bool = True) -> dict:
    """Pass 2 over the pass-1 records (modified in place: status, rd_k,
    ent_base): the dense columns as numpy arrays and ``rd`` = {(k, g): (ctx,
    from)} for the rows written.  ``defer_behind_prop`` False drops the rule
    "a read or transfer behind a taken proposal is deferred" (only
    tests/test_request_wire_ref.py sets it, to show the rule is needed)."""
    d = {k: np.zeros(G, dt) for k, dt in DENSE}
    d["xf_from"][:] = SLOT_LOCAL
    rd = {}
    runs = {}
    for i, r in enumerate(recs):
        if r["status"] == OK and RQ_PROP <= r["kind"] <= RQ_TRANSFER:
            runs.setdefault(r["group"], []).append(i)
    for g, run in runs.items():
        nr = n_ents = 0
        prop = cc = xfer = deferred = took = False
        for i in run:
            r = recs[i]
            if not deferred:
                if r["kind"] == RQ_READ:
                    deferred = (prop and defer_behind_prop) or nr >= max_reads
                elif r["kind"] == RQ_TRANSFER:
                    deferred = (prop and defer_behind_prop) or xfer
                else:
                    deferred = prop and (not concat or (r["cc_at"] != NO_CC and cc) or
                                         n_ents + r["ent_n"] > MAX_ENTS)
            if deferred:
                r["status"] = DEFERRED
                continue
            took = True
            if r["kind"] == RQ_READ:
                rd[(nr, g)] = (r["ctx"], r["slot"])
                r["rd_k"] = nr
                nr += 1
            elif r["kind"] == RQ_TRANSFER:
                xfer = True
                d["xf_from"][g], d["xf_term"][g] = r["slot"], r["term"]
            else:
                if r["cc_at"] != NO_CC:
                    cc = True
                    d["g_cc_at"][g] = n_ents + r["cc_at"]
                    d["g_cc_payload"][g] = r["cc_payload"]
                    d["action"][g] |= PROP_CONF_CHANGE | (PROP_CC_LEAVE_JOINT if r["cc_leave"] else 0)
                prop = True
                d["action"][g] |= PROP_ENTRIES
                r["ent_base"] = n_ents
                n_ents += r["ent_n"]
                d["g_payload"][g] += np.uint64(r["payload"])
        d["n_reads"][g], d["n_ents"][g] = nr, n_ents
        d["gflags"][g] = (FLAG_TAKEN if took else 0) | (FLAG_DEFERRED if deferred else 0)
    d["rd"] = rd
    return d


def ingest(buf: bytes, nbytes: int, msg_off, msg_group, off, ids, max_reads: int = 1,
           concat: bool = False) -> dict:
    """The batch: every message column and dense column of qb_request_wire_out
    as numpy arrays, ``rd`` (the rows of rd_ctx / rd_from written) and
    ``stats`` [15]."""
    M, G = len(msg_group), len(off) - 1
    recs = []
    for i in range(M):
        p0, p1 = int(msg_off[i]), int(msg_off[i + 1])
        if not (p0 <= p1 <= nbytes):
            recs.append(_record(UNMARSHAL))
            continue
        g = int(msg_group[i])
        gids = ids[int(off[g]):int(off[g + 1])] if g < G else ()
        r = decode(bytes(buf[p0:p1]), g, G, gids)
        if r["ent_bytes"]:
            r["ent_pos"] += p0
        recs.append(r)
    pass1 = [r["status"] for r in recs]
    out = combine(recs, G, max_reads, concat)
    out.update({k: np.array([r[k] for r in recs], dt) for k, dt in COLUMNS})
    stats = np.zeros(STAT_COUNT, np.uint64)
    stats[:10] = np.bincount(out["status"], minlength=10)
    for r, st1 in zip(recs, pass1):
        if r["status"] == OK:
            stats[{RQ_PROP: STAT_TAKEN_PROPS, RQ_READ: STAT_TAKEN_READS,
                   RQ_TRANSFER: STAT_TAKEN_TRANSFERS, RQ_READ_RESP: STAT_READ_RESPS}[r["kind"]]] += 1
            if r["kind"] == RQ_PROP:
                stats[STAT_ENTRIES_TAKEN] += r["ent_n"]
    out["stats"] = stats
    return out
