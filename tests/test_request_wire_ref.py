"""tests/request_wire_ref.py against the reference's own data and against
stepping the messages one by one: the conf-change schema pinned to the
reference's descriptor, the conf changes the reference's tests propose with
the wantsLeaveJoint Go yields, every deferral rule, and the rule that orders
the two dense calls (qb_dev_leader_requests first, qb_dev_leader_propose
second) checked on a one-voter group with tests/request_ref.py and
tests/propose_ref.py."""
import copy
import json
import os

import numpy as np
import pytest

from oracle import raftpb_ref as W
from tests import propose_ref as PR, request_pack, request_ref as QR, request_wire_pack as P, \
    request_wire_ref as RW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "request_wire_cases.json"), encoding="utf-8") as f:
        return json.load(f)


def test_conf_change_schemas_are_the_reference_descriptors(golden):
    fields = {k: {int(n): v for n, v in m.items()} for k, m in golden["schema"].items()}
    assert W.schema_from_descriptor(fields, kinds=tuple(RW.CC_SCHEMAS)) == RW.CC_SCHEMAS
    assert [fields["ConfChange"][n]["name"] for n in (1, 2, 3, 4)] == ["id", "type", "node_id", "context"]
    assert [fields["ConfChangeV2"][n]["name"] for n in (1, 2, 3)] == ["transition", "changes", "context"]
    assert fields["ConfChangeV2"][2]["label"] == W.LABEL_REPEATED


def _data(case):
    if case["data_nil"]:
        return None
    ctx = lambda c: None if c is None else c.encode()  # noqa: E731
    if "v1" in case:
        v = case["v1"]
        return P.marshal_cc(v["id"], v["type"], v["node_id"], ctx(v["context"]))
    if "v2" in case:
        v = case["v2"]
        return P.marshal_cc_v2(v["transition"], [tuple(c) for c in v["changes"]], ctx(v["context"]))
    return case["data"].encode()


def test_golden_conf_changes(golden):
    """Each of the reference's proposals as the second entry of a MsgProp, as
    TestRawNodeProposeAndConfChange proposes them behind "somedata"."""
    assert len(golden["cases"]) == 13
    for case in golden["cases"]:
        data = _data(case)
        m = P.prop([P.ent(b"somedata"), P.ent(data, case["entry_type"])], frm=2)
        r = RW.decode(m, 0, 1, [1, 2, 3])
        assert r["status"] == RW.OK and r["ent_n"] == 2, case["source"]
        assert r["payload"] == 8 + len(data or b""), case["source"]
        if case["wants_leave_joint"] is None:
            assert r["cc_at"] == RW.NO_CC and r["cc_leave"] == 0, case["source"]
        else:
            assert (r["cc_at"], r["cc_payload"]) == (1, len(data or b"")), case["source"]
            assert r["cc_leave"] == int(case["wants_leave_joint"]), case["source"]
    leaves = [c["source"] for c in golden["cases"] if c["wants_leave_joint"]]
    assert len(leaves) == 2 and all("leaving" in s for s in leaves)


def test_every_special_case_and_corruption():
    for name, (b, st) in P.special_cases().items():
        assert RW.decode(b, 0, 1, [3, 5])["status"] == st, name
    for name, b in P.corruptions().items():
        r = RW.decode(b, 0, 1, [3, 5])
        assert r["status"] == RW.UNMARSHAL and r["group"] == RW.NO_GROUP and r["frm"] == 0, name


OFF, IDS = np.array([0, 3, 4], np.uint32), np.array([11, 22, 33, 7], np.uint64)
CC = P.ent(P.marshal_cc_v2(0, [(0, 9)]), RW.ENTRY_CONF_CHANGE_V2)
LEAVE = P.ent(P.marshal_cc_v2(), RW.ENTRY_CONF_CHANGE_V2)


def _ingest(msgs, grp=None, max_reads=2, concat=False):
    buf, off = P.pack(msgs)
    return RW.ingest(buf, len(buf), off, [0] * len(msgs) if grp is None else grp, OFF, IDS, max_reads,
                     concat)


@pytest.mark.parametrize("what,msgs,concat,status", (
    ("the read past max_reads", [P.read(1), P.read(2, 22), P.read(3)], False, [0, 0, 9]),
    ("a read behind a taken proposal", [P.prop([P.ent()]), P.read(1)], False, [0, 9]),
    ("a second transfer", [P.transfer(11), P.read(5), P.transfer(22)], False, [0, 0, 9]),
    ("a transfer behind a taken proposal", [P.prop([P.ent()]), P.transfer(11)], True, [0, 9]),
    ("a second proposal without concat", [P.prop([P.ent()]), P.prop([P.ent()])], False, [0, 9]),
    ("a second proposal with concat", [P.prop([P.ent()]), P.prop([P.ent()])], True, [0, 0]),
    ("a second conf change with concat", [P.prop([CC]), P.prop([P.ent()]), P.prop([LEAVE])], True,
     [0, 0, 9]),
    ("everything behind a deferred one", [P.read(1), P.read(2), P.read(3), P.transfer(11), P.prop([P.ent()])],
     True, [0, 0, 9, 9, 9]),
    ("another group is not held back", [P.prop([P.ent()]), P.read(1), P.read(2)], False, [0, 9, 0]),
))
def test_deferral_rules(what, msgs, concat, status):
    grp = [0, 0, 1] if what.startswith("another") else None
    w = _ingest(msgs, grp, concat=concat)
    assert w["status"].tolist() == status, what
    assert w["gflags"][0] == RW.FLAG_TAKEN | (RW.FLAG_DEFERRED if 9 in status else 0)
    n_def = status.count(9)
    assert w["stats"][RW.DEFERRED] == n_def and w["stats"][RW.OK] == len(status) - n_def


def test_entry_count_past_32_bits_defers():
    recs = [dict(RW._record(RW.OK, group=0, kind=RW.RQ_PROP, ent_n=n, cc_at=RW.NO_CC, payload=1))
            for n in ((1 << 31), (1 << 31) - 1, 1, 5)]
    for r in recs:
        r["group"] = 0
    d = RW.combine(recs, 1, 1, True)
    assert [r["status"] for r in recs] == [RW.OK, RW.OK, RW.DEFERRED, RW.DEFERRED]
    assert int(d["n_ents"][0]) == RW.MAX_ENTS and recs[1]["ent_base"] == 1 << 31


def test_concatenation_sums_and_places_the_conf_change():
    w = _ingest([P.prop([P.ent(b"ab"), P.ent(b"c")]), P.prop([P.ent(b"defg"), LEAVE, P.ent(b"")]),
                 P.prop([P.ent(b"h")])], concat=True)
    leave = len(P.marshal_cc_v2())
    assert w["ent_base"].tolist() == [0, 2, 5] and int(w["n_ents"][0]) == 6
    assert int(w["g_payload"][0]) == 3 + 4 + leave + 1
    assert int(w["g_cc_at"][0]) == 3 and int(w["g_cc_payload"][0]) == leave
    assert int(w["action"][0]) == RW.PROP_ENTRIES | RW.PROP_CONF_CHANGE | RW.PROP_CC_LEAVE_JOINT
    assert int(w["action"][1]) == RW.PROP_NONE and int(w["xf_from"][1]) == RW.SLOT_LOCAL
    assert w["stats"][RW.STAT_TAKEN_PROPS] == 3 and w["stats"][RW.STAT_ENTRIES_TAKEN] == 6


def test_reads_and_transfer_fill_the_request_columns():
    w = _ingest([P.read(5, 33), P.transfer(22, term=9), P.read(6), P.read_resp(8, 77, frm=11, term=4)])
    assert w["rd"] == {(0, 0): (5, 2), (1, 0): (6, RW.SLOT_LOCAL)} and w["rd_k"].tolist() == [0, 0, 1, 0]
    assert (int(w["xf_from"][0]), int(w["xf_term"][0]), int(w["n_reads"][0])) == (1, 9, 2)
    assert (int(w["index"][3]), int(w["ctx"][3]), int(w["term"][3]), int(w["frm"][3])) == (77, 8, 4, 11)
    assert w["stats"][RW.STAT_READ_RESPS] == 1 and w["stats"][RW.OK] == 4


# ------------------------------------------- requests first, proposal second ---

def _one_voter():
    """A one-voter leader at term 5 whose log [1, 2] is committed."""
    return request_pack.make_node(1, 1, 0, 0, terms=[0, 5, 5], term=5, committed=2)


def _step_dense(n, recs, d, rd, out):
    """qb_dev_leader_requests, then qb_dev_leader_propose, on group 0's dense
    columns; ``out`` collects (ctx, read index) and the commit."""
    reads = [rd[(k, 0)] for k in range(int(d["n_reads"][0]))]
    res = QR.step(n, reads, int(d["xf_from"][0]), int(d["xf_term"][0]),
                  QR.Config(max_reads=4), QR.new_stats())
    out += [(ctx, idx) for (ctx, _), (st, idx) in zip(reads, res.reads) if st == QR.RD_READ_STATE]
    PR.step(n.prop, int(d["action"][0]), int(d["n_ents"][0]), int(d["g_payload"][0]),
            int(d["g_cc_at"][0]), int(d["g_cc_payload"][0]), PR.Config(), PR.new_stats())
    n.sync()


def _by_the_dense_calls(msgs, defer_behind_prop):
    """The batch ingested and stepped, then the deferred rest resubmitted,
    until nothing is left: (node, ReadStates)."""
    n, states = _one_voter(), []
    while msgs:
        recs = [RW.decode(m, 0, 1, [1]) for m in msgs]
        assert all(r["status"] == RW.OK for r in recs)
        d = RW.combine(recs, 1, 4, False, defer_behind_prop=defer_behind_prop)
        _step_dense(n, recs, d, d["rd"], states)
        rest = [m for m, r in zip(msgs, recs) if r["status"] == RW.DEFERRED]
        assert len(rest) < len(msgs)
        msgs = rest
    return n, states


def _one_by_one(msgs):
    """Step(m) for each message in arrival order, through the same restatements."""
    n, states = _one_voter(), []
    for m in msgs:
        r = RW.decode(m, 0, 1, [1])
        if r["kind"] == RW.RQ_READ:
            res = QR.step(n, [(r["ctx"], r["slot"])], QR.NO_SLOT, 0, QR.Config(max_reads=4), QR.new_stats())
            states += [(r["ctx"], idx) for st, idx in res.reads if st == QR.RD_READ_STATE]
        else:
            PR.step(n.prop, RW.PROP_ENTRIES, r["ent_n"], r["payload"], 0, 0, PR.Config(), PR.new_stats())
            n.sync()
    return n, states


def _state(n):
    g = n.group
    return (g.log.committed, g.log.last, list(n.prop.terms), n.prop.uncommitted_size, g.term)


def test_requests_then_proposal_equals_stepping_in_arrival_order():
    msgs = [P.read(101), P.prop([P.ent(b"w")]), P.read(102)]
    want_n, want_states = _one_by_one(msgs)
    assert want_states == [(101, 2), (102, 3)] and want_n.group.log.committed == 3
    n, states = _by_the_dense_calls(msgs, defer_behind_prop=True)
    assert states == want_states and _state(n) == _state(want_n)
    # without "a read behind a taken proposal is deferred" the second read is
    # answered ahead of the proposal it arrived behind
    n, states = _by_the_dense_calls(copy.copy(msgs), defer_behind_prop=False)
    assert states == [(101, 2), (102, 2)] and states != want_states and _state(n) == _state(want_n)
