"""The restatement of the follower's wire ingest (tests/follower_wire_ref.py)
pinned against Google's protobuf runtime on the reference's own schema
(tests/golden/raftpb_schema.json): seeded messages of the five device kinds
and of the host kinds are encoded by that runtime, decoded by the restatement
and compared field for field."""
import random

import numpy as np
import pytest

from oracle import raftpb_ref as W
from tests import follower_wire_ref as FW
from tests.test_encode_ref import _pool

BOUNDARY = (0, 1, 127, 128, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63, (1 << 64) - 1)
DEVICE_TYPES = (3, 5, 8, 14, 17)
HOST_TYPES = (0, 1, 2, 4, 6, 7, 9, 10, 11, 12, 13, 15, 16, 18, 19, 127, 128, 255, 256 + 8, 1 << 31)
CONTEXTS = {"nil": None, "empty": b"", "eight": (0x0102030405060708).to_bytes(8, "big"),
            "eight zeros": bytes(8), "transfer": FW.CAMPAIGN_TRANSFER,
            "near miss": b"CampaignTransfes", "seven": b"1234567", "long": b"x" * 40}


def google(P, m, ents=(), snapshot="gogo"):
    """Google's runtime on the message ``m`` (a dict) with entries (term,
    index, data) — every scalar set explicitly, as gogoproto writes
    non-nullable fields."""
    g = P["Message"]()
    g.type, g.to, g.term, g.logTerm, g.index = m["type"], m["to"], m["term"], m["log_term"], m["index"]
    setattr(g, "from", m["frm"])
    g.commit, g.reject, g.rejectHint = m["commit"], bool(m["reject"]), m["reject_hint"]
    for term, index, data in ents:
        e = g.entries.add()
        e.Type, e.Term, e.Index = 0, term, index
        if data is not None:
            e.Data = data
    if snapshot == "gogo":      # Metadata and ConfState non-nullable: 12 bytes with the key
        g.snapshot.metadata.conf_state.auto_leave = False
        g.snapshot.metadata.index = 0
        g.snapshot.metadata.term = 0
    elif snapshot == "brief":   # an empty Metadata: 4a 02 12 00
        g.snapshot.metadata.SetInParent()
    if m["context"] is not None:
        g.context = m["context"]
    return g.SerializeToString()


def message(r, t, context=None):
    b = lambda: r.choice(BOUNDARY)  # noqa: E731
    return dict(type=t, to=b(), frm=b(), term=b(), log_term=b(), index=b(), commit=b(),
                reject=r.random() < 0.3, reject_hint=b(), context=context)


def entries_from(r, index, n, terms=None):
    return [(r.choice(BOUNDARY) if terms is None else terms[k], (index + 1 + k) & FW.M64,
             r.choice((None, b"", b"d", bytes(r.getrandbits(8) for _ in range(r.randint(2, 40))))))
            for k in range(n)]


def test_both_snapshot_spellings_come_from_the_runtime():
    P = _pool()
    m = message(random.Random(1), 8)
    full, brief = google(P, m), google(P, m, snapshot="brief")
    assert bytes.fromhex("4a0a12080a022800100018 00".replace(" ", "")) in full
    assert bytes.fromhex("4a021200") in brief and len(full) == len(brief) + 8
    assert FW.decode(full, 3) == FW.decode(brief, 3)


def test_seeded_messages_field_for_field():
    P = _pool()
    r = random.Random(0xF0110)
    seen = {}
    for it in range(3000):
        t = r.choice(DEVICE_TYPES * 3 + HOST_TYPES)
        cname = r.choice(list(CONTEXTS))
        m = message(r, t, CONTEXTS[cname])
        n = r.choice((0, 0, 1, 2, 5)) if t in (3, 2, 15) else 0
        ents = entries_from(r, m["index"], n)
        b = google(P, m, ents, snapshot=r.choice(("gogo", "brief")))
        group = r.choice((0, 7, 299, 300, 0xFFFFFFFE))
        rec = FW.decode(b, group)
        assert rec["group"] == group and rec["frm"] == m["frm"] and rec["term"] == m["term"]
        assert rec["msg_type"] == m["type"] & 0xFF
        ctx = m["context"] or b""
        if m["type"] == 8:
            ok = len(ctx) == 0 or (len(ctx) == 8 and any(ctx))
            assert rec["status"] == (FW.OK if ok else FW.CTX)
            if ok:
                assert (rec["flags"], rec["index"], rec["aux"], rec["commit"]) == (
                    FW.FIN_HEARTBEAT, m["commit"], int.from_bytes(ctx, "big") if ctx else 0, 0)
        elif m["type"] in (5, 17):
            kind = FW.FIN_VOTE if m["type"] == 5 else FW.FIN_PREVOTE
            force = FW.FORCE if cname == "transfer" else 0
            assert (rec["status"], rec["flags"], rec["index"], rec["aux"]) == (
                FW.OK, kind | force, m["index"], m["log_term"])
        elif m["type"] == 14:
            assert (rec["status"], rec["flags"], rec["index"], rec["aux"]) == (
                FW.OK, FW.FIN_TIMEOUT_NOW, 0, 0)
        elif m["type"] == 3:
            assert (rec["status"], rec["flags"]) == (FW.OK, FW.FIN_APP)
            assert (rec["index"], rec["aux"], rec["commit"], rec["ent_n"]) == (
                m["index"], m["log_term"], m["commit"], n)
            assert rec["runs"] == FW.term_runs(e[0] for e in ents)
            if n:
                # the range is the entries as the runtime wrote them, one 3a-keyed field each
                body = b[rec["ent_pos"]:rec["ent_pos"] + rec["ent_bytes"]]
                enc = [W.marshal_entry(t_, i_, 0, d_) for t_, i_, d_ in ents]
                assert body == b"".join(b"\x3a" + W.varint(len(e)) + e for e in enc)
            else:
                assert (rec["ent_pos"], rec["ent_bytes"]) == (0, 0)
        else:
            assert (rec["status"], rec["flags"]) == (FW.TYPE, FW.FIN_HOST)
            assert (rec["index"], rec["aux"], rec["commit"], rec["ent_n"], rec["runs"]) == (0, 0, 0, 0, [])
        if rec["status"] != FW.OK:
            assert rec["flags"] == FW.FIN_HOST
        seen.setdefault((m["type"], rec["status"]), 0)
        seen[(m["type"], rec["status"])] += 1
    for t in DEVICE_TYPES:
        assert seen[(t, FW.OK)] >= 100, (t, seen)
    assert seen[(8, FW.CTX)] >= 50
    assert {t for t, st in seen if st == FW.TYPE} >= {0, 1, 2, 4, 7, 9, 15, 18, 19, 255, 264}


@pytest.mark.parametrize("field", ("frm", "term", "index", "log_term", "commit"))
def test_boundary_values_of_every_field(field):
    P = _pool()
    r = random.Random(7)
    for v in BOUNDARY:
        for t in DEVICE_TYPES:
            m = dict(message(r, t), **{field: v})
            rec = FW.decode(google(P, m, entries_from(r, m["index"], 2) if t == 3 else ()), 1)
            assert rec["status"] == FW.OK
            got = {"frm": rec["frm"], "term": rec["term"],
                   "index": rec["index"] if t in (3, 5, 17) else m["index"],
                   "log_term": rec["aux"] if t in (3, 5, 17) else m["log_term"],
                   "commit": rec["commit"] if t == 3 else rec["index"] if t == 8 else m["commit"]}
            assert got[field] == v, (field, v, t)


def test_contexts():
    P = _pool()
    r = random.Random(9)
    want_hb = {"nil": (FW.OK, 0), "empty": (FW.OK, 0), "eight": (FW.OK, 0x0102030405060708),
               "eight zeros": (FW.CTX, 0), "transfer": (FW.CTX, 0), "near miss": (FW.CTX, 0),
               "seven": (FW.CTX, 0), "long": (FW.CTX, 0)}
    for name, ctx in CONTEXTS.items():
        rec = FW.decode(google(P, message(r, 8, ctx)), 2)
        assert (rec["status"], rec["aux"]) == want_hb[name], name
        assert rec["flags"] == (FW.FIN_HEARTBEAT if rec["status"] == FW.OK else FW.FIN_HOST)
        for t, kind in ((5, FW.FIN_VOTE), (17, FW.FIN_PREVOTE)):
            rec = FW.decode(google(P, message(r, t, ctx)), 2)
            assert rec["status"] == FW.OK
            assert rec["flags"] == kind | (FW.FORCE if name == "transfer" else 0), name
        rec = FW.decode(google(P, message(r, 14, ctx)), 2)
        assert (rec["status"], rec["flags"]) == (FW.OK, FW.FIN_TIMEOUT_NOW)


def test_entries_the_device_does_not_take():
    P = _pool()
    r = random.Random(11)
    m = dict(message(r, 3), index=10)
    good = [(5, 11, b"a"), (5, 12, None), (6, 13, b"")]
    rec = FW.decode(google(P, m, good), 0)
    assert rec["status"] == FW.OK and rec["runs"] == [(5, 2), (6, 1)]
    for bad in ([(5, 11, None), (5, 13, None)], [(5, 11, None), (5, 11, None)],
                [(5, 12, None)], [(5, 12, None), (5, 11, None)]):
        rec = FW.decode(google(P, m, bad), 0)
        assert (rec["status"], rec["flags"], rec["runs"], rec["ent_n"]) == (
            FW.ENTRIES, FW.FIN_HOST, [], len(bad))
        assert (rec["ent_pos"], rec["ent_bytes"]) == (0, 0)
        assert (rec["index"], rec["aux"], rec["commit"]) == (10, m["log_term"], m["commit"])
    # a Commit field between two entries: every index right, the range not one
    ents = [W.marshal_entry(5, 11 + k, 0, None) for k in range(2)]
    f7 = [b"\x3a" + W.varint(len(e)) + e for e in ents]
    b = b"\x08\x03\x30\x0a" + f7[0] + b"\x40\x09" + f7[1]
    rec = FW.decode(b, 0)
    assert (rec["status"], rec["commit"], rec["ent_n"]) == (FW.ENTRIES, 9, 2)
    assert FW.decode(b"\x08\x03\x30\x0a" + f7[0] + f7[1] + b"\x40\x09", 0)["status"] == FW.OK
    # Index behind the entries still counts: Unmarshal is a fold over the fields
    assert FW.decode(b"\x08\x03" + f7[0] + f7[1] + b"\x30\x0a", 0)["runs"] == [(5, 2)]
    # wrap: Index = 2^64 - 2 with three entries
    m = dict(message(r, 3), index=(1 << 64) - 2)
    rec = FW.decode(google(P, m, [(1, (1 << 64) - 1, None), (1, 0, None), (2, 1, None)]), 0)
    assert rec["status"] == FW.OK and rec["runs"] == [(1, 2), (2, 1)]


def test_batch_layout_and_ent_cap():
    P = _pool()
    r = random.Random(13)
    msgs, grp = [], []
    for i in range(40):
        t = (3, 8, 3, 5)[i % 4]
        m = dict(message(r, t), index=100)
        ents = [(1 + (k // 2), 101 + k, b"p") for k in range(i % 5)] if t == 3 else ()
        msgs.append(google(P, m, ents))
        grp.append(i)
    off = np.zeros(41, np.uint64)
    off[1:] = np.cumsum([len(b) for b in msgs])
    buf = b"".join(msgs)
    full = FW.ingest(buf, len(buf), off, grp)
    counts = np.diff(full["ent_off"].astype(np.int64))
    assert full["ent_total"] == counts.sum() == sum(len(x) for x in full["runs"]) > 20
    assert int(full["stats"][FW.OK]) == 40
    for i in np.nonzero(full["ent_bytes"])[0]:
        p = int(full["ent_pos"][i])
        assert off[i] < p and p + int(full["ent_bytes"][i]) <= off[i + 1] and buf[p] == 0x3A
    j = int(np.nonzero(counts == 2)[0][3])
    for cap, first in ((0, int(np.nonzero(counts)[0][0])), (int(full["ent_off"][j]) + 1, j),
                       (int(full["ent_off"][j + 1]), int(j + 1 + np.nonzero(counts[j + 1:])[0][0])),
                       (full["ent_total"], None)):
        got = FW.ingest(buf, len(buf), off, grp, cap)
        ns = np.nonzero(got["status"] == FW.NO_SPACE)[0]
        assert np.array_equal(got["ent_off"], full["ent_off"]) and got["ent_total"] == full["ent_total"]
        if first is None:
            assert len(ns) == 0
        else:
            assert ns[0] == first and np.array_equal(ns, first + np.nonzero(counts[first:])[0])
            assert (got["flags"][ns] == FW.FIN_HOST).all() and all(got["runs"][i] == [] for i in ns)
            assert np.array_equal(got["ent_pos"], full["ent_pos"])
        assert int(got["stats"].sum()) == 40 and int(got["stats"][FW.NO_SPACE]) == len(ns)
    # a slice that is not inside the buffer
    bad = off.copy()
    bad[5] = bad[6] + 1
    got = FW.ingest(buf, len(buf), bad, grp)
    assert got["status"][5] == FW.UNMARSHAL and got["group"][5] == FW.NO_GROUP
    got = FW.ingest(buf, len(buf) - 1, off, grp)
    assert got["status"][39] == FW.UNMARSHAL and (got["status"][:39] == FW.OK).all()


def test_the_gpu_tests_generator_reaches_every_path():
    """tests/follower_wire_pack.py's mixture, seen by the restatement alone:
    every prefix the GPU tests use keeps each device kind, the whole batch
    every status and every MsgApp case."""
    from tests import follower_wire_pack as P
    msgs, grp = P.base_batch()
    buf, off = P.pack(msgs)
    for M in (63, 64, 65, 255, 256, 257, 300, 600, 1000):
        P.assert_mixture(FW.ingest(buf, int(off[M]), off[:M + 1], grp[:M]), M)
    want = FW.ingest(buf, len(buf), off, grp)
    assert any(len(x) == 9 for x in want["runs"]) and [(9, 200)] in want["runs"]
    assert want["ent_bytes"].max() > 3000 and want["ent_total"] > 256
    r = random.Random(1)
    for name, b in P.corruptions(r).items():
        assert FW.decode(b, 0)["status"] == FW.UNMARSHAL, name
