"""The restatement of the batched Message.Marshal (tests/encode_ref.py)
against Google's protobuf runtime on the reference's own schema
(tests/golden/raftpb_schema.json), the wire decoder, the host's splice and
raft.send's rules."""
import json
import os
import random

import numpy as np
import pytest

from oracle import raftpb_ref as W
from tests import encode_ref as E

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "quorum_batch.h")
TYPE_ENUM, TYPE_UINT64 = 14, 4


def _pool():
    """Message classes of Google's runtime over the descriptor fixture (the
    enum fields as uint64: the same varint)."""
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    with open(os.path.join(HERE, "golden", "raftpb_schema.json")) as f:
        schema = json.load(f)["messages"]
    fd = descriptor_pb2.FileDescriptorProto(name="raftpb_encode_test.proto", package="raftpb",
                                            syntax="proto2")
    kinds = ("ConfState", "SnapshotMetadata", "Snapshot", "Entry", "Message")
    for kind in kinds:
        m = fd.message_type.add(name=kind)
        for num, fdesc in sorted(schema[kind].items(), key=lambda kv: int(kv[0])):
            typ = TYPE_UINT64 if fdesc["type"] == TYPE_ENUM else fdesc["type"]
            f_ = m.field.add(name=fdesc["name"], number=int(num), type=typ, label=fdesc["label"])
            if fdesc["type"] == W.TYPE_MESSAGE:
                f_.type_name = fdesc["type_name"]
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    return {k: message_factory.GetMessageClass(pool.FindMessageTypeByName("raftpb." + k))
            for k in kinds}


def _google(P, m, entries=()):
    g = P["Message"]()
    g.type, g.to, g.term, g.logTerm, g.index = m["type"], m["to"], m["term"], m["log_term"], m["index"]
    setattr(g, "from", m["frm"])
    g.commit, g.reject, g.rejectHint = m["commit"], bool(m["reject"]), m["reject_hint"]
    own, context = E.context_of(m)
    for data in ([m["ctx"].to_bytes(8, "big")] if own else []):
        e = g.entries.add()
        e.Type, e.Term, e.Index, e.Data = 0, 0, 0, data
    for term, index, data in entries:
        e = g.entries.add()
        e.Type, e.Term, e.Index, e.Data = 0, term, index, data
    # gogoproto's non-nullable embedded messages and scalars are always written
    g.snapshot.metadata.conf_state.auto_leave = False
    g.snapshot.metadata.index = 0
    g.snapshot.metadata.term = 0
    if context is not None:
        g.context = context
    return g.SerializeToString()


def _fuzz_message(r):
    b = lambda: r.choice(E.BOUNDARY)  # noqa: E731
    return E.message(type=r.choice([1, 3, 4, 5, 6, 8, 9, 14, 15, 16, 17, 18, 127, 128, 255]),
                     to=b(), frm=b(), term=b(), log_term=b(), index=b(), commit=b(),
                     reject=r.random() < 0.5, reject_hint=b(),
                     ctx=r.choice([0, 0, 1, 1 << 56, (1 << 64) - 1, r.getrandbits(64) | 1]))


def test_fuzz_against_google_protobuf():
    P = _pool()
    r = random.Random(0xE7C0DE)
    compared = 0
    seen = set()
    for _ in range(800):
        m = _fuzz_message(r)
        b = E.marshal(m)
        assert b == _google(P, m)
        assert len(b) == E.size(m)
        seen.add((m["type"] in (15, 16), m["ctx"] != 0))
        compared += 1
    assert compared >= 500
    assert seen == {(False, False), (False, True), (True, False), (True, True)}


def test_empty_snapshot_is_the_nested_marshal():
    """Field 9 of every message: Snapshot.Marshal of the zero value through
    SnapshotMetadata and ConfState (raft.pb.go:863-886, 824-846, 1021-1063),
    against Google's runtime."""
    P = _pool()
    s = P["Snapshot"]()
    s.metadata.conf_state.auto_leave = False
    s.metadata.index = 0
    s.metadata.term = 0
    assert s.SerializeToString() == W.EMPTY_SNAPSHOT
    b = E.marshal(E.message(type=8))
    assert bytes([0x4a, len(W.EMPTY_SNAPSHOT)]) + W.EMPTY_SNAPSHOT in b
    assert len(W.EMPTY_SNAPSHOT) + 2 == 12


def test_round_trip_through_unmarshal():
    r = random.Random(5)
    for _ in range(500):
        m = _fuzz_message(r)
        ok, f = W.decode_message(E.marshal(m))
        assert ok
        assert [f[k] for k in (1, 2, 3, 4, 5, 6, 8, 10, 11)] == [
            m["type"], m["to"], m["frm"], m["term"], m["log_term"], m["index"], m["commit"],
            m["reject"], m["reject_hint"]]
        assert f[9] == [{2: [{1: [{5: 0}], 2: 0, 3: 0}]}]
        data = m["ctx"].to_bytes(8, "big")
        if m["ctx"] == 0:
            assert 7 not in f and 12 not in f
        elif m["type"] in (15, 16):
            assert f[7] == [{1: 0, 2: 0, 3: 0, 4: data}] and 12 not in f
        else:
            assert f[12] == data and 7 not in f


def test_splice_of_host_entries():
    P = _pool()
    r = random.Random(6)
    for _ in range(200):
        m = _fuzz_message(r)
        m.update(type=3, ctx=0, n_entries=r.randint(1, 3))
        ents = [(r.choice(E.BOUNDARY), r.choice(E.BOUNDARY),
                 bytes(r.getrandbits(8) for _ in range(r.randint(0, 9))))
                for _ in range(m["n_entries"])]
        enc = [W.marshal_entry(t, i, 0, d) for t, i, d in ents]
        lay = E.finish([(E.ENTRIES, m)])
        assert lay["status"][0] == E.ENTRIES
        whole = E.splice(lay["bytes"].tobytes(), int(lay["ent_at"][0]), enc)
        assert whole == E.marshal(m, entries=enc) == _google(P, m, ents)


def _header_define(name):
    import re
    text = open(HEADER).read()
    return int(re.search(rf"#define {name} (\d+)", text).group(1))


def test_max_bytes_is_the_all_maximum_message():
    top = (1 << 64) - 1
    longest = 0
    for t in (255, 15, 16, 3):
        m = E.message(type=t, to=top, frm=top, term=top, log_term=top, index=top, commit=top,
                      reject=1, reject_hint=top, ctx=top)
        longest = max(longest, len(E.marshal(m)))
    assert longest == len(E.marshal(E.message(type=16, to=top, frm=top, term=top, log_term=top,
                                              index=top, commit=top, reject=1, reject_hint=top,
                                              ctx=top)))
    assert longest == E.MAX_BYTES == _header_define("QB_ENC_MAX_BYTES")
    from etcd_amd.quorum import encode
    assert encode.ENC_MAX_BYTES == longest and encode.max_bytes(3) == 3 * longest


def test_status_values_match_header():
    from etcd_amd.quorum import encode
    for k, name in enumerate(("OK", "ENTRIES", "HOST", "NONE", "NO_SPACE")):
        assert _header_define(f"QB_ENC_{name}") == k == getattr(E, name) == getattr(encode, f"ENC_{name}")


def _groups():
    off = np.array([0, 3, 3, 8, 9], np.uint32)          # group 1 empty
    ids = np.array([1, 2, 3, 10, 11, 12, 13, 14, 7], np.uint64)
    self_id = np.array([2, 5, 12, 99], np.uint64)       # group 3: own slot absent
    term = np.array([5, 6, 1 << 40, 8], np.uint64)
    return 4, off, ids, self_id, term


def test_send_rules_of_the_list_front_end():
    from etcd_amd.quorum.leader import MSG_DTYPE
    G, off, ids, self_id, term = _groups()
    recs = np.zeros(12, MSG_DTYPE)
    rows = [(3, 0, 0, 7, 4, 9, 2), (8, 2, 1, 0, 0, 3, 77), (14, 2, 4, 0, 0, 0, 0),
            (16, 0, 2, 21, 0, 0, 0xABCD), (7, 0, 1, 5, 5, 0, 0), (255, 0, 0xFF, 1, 0, 0, 9),
            (3, 4, 0, 0, 0, 0, 0), (3, 1, 0, 0, 0, 0, 0), (3, 0, 3, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 0),
            (5, 0, 1, 0, 0, 0, 0), (3, 3, 0, 1, 1, 1, 0)]
    for i, (t, g, to, idx, lt, com, aux) in enumerate(rows):
        recs[i] = (idx, lt, com, aux, g, to, t, 0)
    out = E.msg_out(G, off, ids, self_id, term, recs, 12, msg_total=11)
    st = [s for s, _ in out]
    assert st == [E.ENTRIES, E.OK, E.OK, E.OK, E.HOST, E.NONE, E.NONE, E.NONE, E.NONE, E.NONE,
                  E.HOST, E.NONE]
    app, hb, tn, rir = (out[i][1] for i in range(4))
    for m, g, to in ((app, 0, 1), (hb, 2, 11), (tn, 2, 14), (rir, 0, 3)):
        assert (m["frm"], m["term"], m["to"]) == (int(self_id[g]), int(term[g]), to)
    assert (app["index"], app["log_term"], app["commit"], app["n_entries"], app["ctx"]) == (7, 4, 9, 2, 0)
    assert (hb["commit"], hb["ctx"], hb["index"]) == (3, 77, 0)
    assert (rir["index"], rir["ctx"]) == (21, 0xABCD)
    f = W.decode_message(E.marshal(rir))[1]
    assert f[7] == [{1: 0, 2: 0, 3: 0, 4: (0xABCD).to_bytes(8, "big")}] and 12 not in f
    assert (tn["index"], tn["commit"], tn["ctx"]) == (0, 0, 0)


def test_send_rules_of_the_slot_front_end():
    G, off, ids, self_id, term = _groups()
    S = 9
    hb_commit = np.arange(100, 109, dtype=np.uint64)
    hb_ctx = np.array([0, 0, 0xFEED, 4], np.uint64)
    gflags = np.array([2, 2, 2, 0], np.uint8)
    out = E.slots(G, off, ids, self_id, term, S, gflags, 2, E.MSG_HEARTBEAT,
                  {"commit": hb_commit, "ctx_g": hb_ctx})
    st = [s for s, _ in out]
    assert st == [E.OK, E.NONE, E.OK, E.OK, E.OK, E.NONE, E.OK, E.OK, E.NONE]
    for s, (code, m) in enumerate(out):
        if code != E.OK:
            continue
        g = 0 if s < 3 else 2
        assert (m["type"], m["to"], m["frm"], m["term"]) == (8, int(ids[s]), int(self_id[g]), int(term[g]))
        assert (m["commit"], m["ctx"]) == (int(hb_commit[s]), int(hb_ctx[g]))
    # without gflags group 3 takes part, and its own slot is absent: slot 8 gets a message
    out = E.slots(G, off, ids, self_id, term, S, None, 0xFF, E.MSG_HEARTBEAT, {"commit_g": term})
    assert out[8][0] == E.OK and out[8][1]["commit"] == 8 and out[8][1]["frm"] == 99
    # bcastAppend's columns: per-slot types, a MsgSnap is the host's
    mt = np.array([3, 0, 3, 7, 3, 0, 3, 14, 5], np.uint8)
    out = E.slots(G, off, ids, self_id, term, S, None, 0xFF, 0,
                  {"type": mt, "index": hb_commit, "log_term": hb_commit, "commit_g": term,
                   "n_entries": np.array([0, 0, 2, 0, 0, 0, 1, 0, 0], np.uint64)})
    assert [s for s, _ in out] == [E.OK, E.NONE, E.ENTRIES, E.HOST, E.OK, E.NONE, E.ENTRIES,
                                   E.OK, E.HOST]
    assert out[2][1]["commit"] == 5 and out[6][1]["commit"] == 1 << 40
    assert out[7][1]["index"] == 0  # MsgTimeoutNow carries nothing


def test_send_refuses_what_raft_send_panics_on():
    with pytest.raises(ValueError):
        E.send(1, 2, E.message(type=5))
    with pytest.raises(ValueError):
        E.send(1, 2, E.message(type=8, term=3))
    assert E.send(1, 2, E.message(type=15))["term"] == 0
    assert E.send(1, 2, E.message(type=2))["term"] == 0
    assert E.send(1, 2, E.message(type=5, term=9))["term"] == 9


def test_finish_clips_at_cap():
    recs = E.columns({"type": np.array([8, 0, 8, 7, 8], np.uint8),
                      "to": np.array([1, 2, 300, 4, 5], np.uint64)}, 5)
    full = E.finish(recs)
    L = [int(x) for x in np.diff(full["msg_off"].astype(np.int64))]
    assert L[1] == 0 and L[3] == 0 and L[2] == L[0] + 1
    for cap, want in ((0, [4, 3, 4, 2, 4]), (L[0], [0, 3, 4, 2, 4]), (L[0] + 3, [0, 3, 4, 2, 4]),
                      (L[0] + L[2], [0, 3, 0, 2, 4]), (full["nbytes"], [0, 3, 0, 2, 0])):
        lay = E.finish(recs, cap)
        assert lay["status"].tolist() == want
        assert (lay["msg_off"] == full["msg_off"]).all() and lay["nbytes"] == full["nbytes"]
        assert lay["bytes"].tobytes() == full["bytes"].tobytes()[:lay["written"]]
