"""tests/request_ref.py against the reference's own tests of MsgReadIndex and
MsgTransferLeader (tests/golden/request_tables.json), and its read answers
against oracle/leader_ref.py's responseToReadIndexReq.  No GPU."""
import json
import os
import subprocess
import sys

import pytest

from oracle import leader_ref as L
from tests import request_pack as Q, request_ref as R

SCENARIOS = Q.load_tables()["scenarios"]


def test_the_table_is_what_its_maker_writes(tmp_path):
    """request_tables.json is make_request_golden.py's output, byte for byte."""
    src = os.path.join(Q.ROOT, "tests", "golden", "make_request_golden.py")
    code = open(src, encoding="utf-8").read().replace(
        "os.path.dirname(os.path.abspath(__file__))", repr(str(tmp_path)))
    subprocess.run([sys.executable, "-c", code], check=True, capture_output=True)
    with open(tmp_path / "request_tables.json", encoding="utf-8") as f:
        assert json.load(f)["scenarios"] == SCENARIOS


def test_every_named_test_is_transcribed():
    names = {s["name"].split("/")[0] for s in SCENARIOS}
    assert names >= {
        "TestReadOnlyOptionSafe", "TestReadOnlyWithLearner", "TestReadOnlyOptionLease",
        "TestReadOnlyForNewLeader", "TestRawNodeReadIndex", "TestNodeReadIndexToOldLeader",
        "TestLeaderTransferToUpToDateNode", "TestLeaderTransferToUpToDateNodeFromFollower",
        "TestLeaderTransferToSlowFollower", "TestLeaderTransferAfterSnapshot",
        "TestLeaderTransferToSelf", "TestLeaderTransferToNonExistingNode", "TestLeaderTransferBack",
        "TestLeaderTransferSecondTransferToAnotherNode",
        "TestLeaderTransferSecondTransferToSameNode"}


@pytest.mark.parametrize("sc", SCENARIOS, ids=[s["name"] for s in SCENARIOS])
def test_golden_scenarios(sc):
    st = R.new_stats()
    Q.replay(sc, lambda n, cfg, reads, xf, xt: R.step(n, reads, xf, xt, cfg, st))
    assert sum(st.values()) >= sum(s["op"] != "set" for s in sc["steps"])


def _leader(**kw):
    """Three voters and a learner (slot 3), own slot 1, everything committed
    at term 3."""
    return Q.make_node(4, 0b0111, 0, 1, terms=[1, 1, 2, 2, 3, 3], term=3, committed=5, **kw)


@pytest.mark.parametrize("read_only", [R.SAFE, R.LEASE])
@pytest.mark.parametrize("frm", [R.NO_SLOT, 0, 1, 2, 3])
def test_answers_agree_with_the_oracle(read_only, frm):
    """A read answered at once (lease, or the singleton) and the oracle's
    responseToReadIndexReq on the same request name the same recipient and
    index; a queued one (safe) leaves the row the oracle would answer from."""
    cfg = R.Config(read_only=read_only, readq_cap=4, max_reads=1)
    for single in (False, True):
        n = _leader()
        if single:
            n.group.mask_in = 0b0010
        res = R.step(n, [(77, frm)], R.NO_SLOT, 0, cfg, R.new_stats())
        g = n.group
        g.msgs = []
        if single or read_only == R.LEASE:
            g.response_to_read_index_req(L.ReadIndexStatus(77, res.reads[0][1], set(), frm))
            want = R.RD_READ_STATE if g.msgs[0].type == L.READ_STATE else R.RD_RESP
            assert res.reads[0] == (want, 5) and not g.readq
            assert (g.msgs[0].to, g.msgs[0].index, g.msgs[0].aux) == \
                (L.NO_SLOT if want == R.RD_READ_STATE else frm, 5, 77)
        else:
            assert res.reads[0] == (R.RD_BCAST, None)
            g.response_to_read_index_req(g.readq[0])
            m = g.msgs[0]
            local = frm in (R.NO_SLOT, 1)
            assert (m.type, m.to, m.index, m.aux) == \
                (L.READ_STATE if local else L.MSG_READ_INDEX_RESP, L.NO_SLOT if local else frm, 5, 77)
            assert g.readq[0].acks == {1} and res.heartbeats == [(0, 0), (2, 0), (3, 0)]


def test_reads_in_order_see_what_earlier_ones_queued():
    cfg = R.Config(readq_cap=2, max_reads=8)
    n = _leader()
    st = R.new_stats()
    res = R.step(n, [(5, R.NO_SLOT), (5, 0), (0, 0), (6, 9), (6, 2), (7, 0), (6, R.NO_SLOT)],
                 R.NO_SLOT, 0, cfg, st)
    assert [s for s, _ in res.reads] == [R.RD_BCAST, R.RD_BCAST_DUP, R.RD_BAD, R.RD_HOST,
                                         R.RD_BCAST, R.RD_QUEUE_FULL, R.RD_BCAST_DUP]
    assert [(r.ctx, r.from_slot) for r in n.group.readq] == [(5, R.NO_SLOT), (6, 2)]
    assert res.qflags == R.QFLAG_HEARTBEATS | R.QFLAG_BAD | R.QFLAG_HOST
    assert st["bcast"] == 2 and st["bcast_dup"] == 2 and st["queue_full"] == 1


def test_more_reads_than_max_reads_are_cut_and_counted():
    st = R.new_stats()
    res = R.step(_leader(), [(5, 0), (6, 0), (7, 0)], R.NO_SLOT, 0, R.Config(max_reads=2), st)
    assert len(res.reads) == 2 and st["bad_count"] == 1 and res.qflags & R.QFLAG_BAD


def test_transfer_to_self_aborts_first_and_a_learner_does_not():
    st = R.new_stats()
    n = _leader(transferee=2)
    res = R.step(n, [], 1, 0, R.Config(), st)
    assert n.group.transferee == R.NO_SLOT and res.qflags == R.QFLAG_TRANSFER_ABORTED
    n = _leader(transferee=2)
    res = R.step(n, [], 3, 0, R.Config(), st)
    assert n.group.transferee == 2 and res.qflags == 0 and st["xf_ign_learner"] == 1


def test_transfer_term_filter():
    for role, lead in ((R.LEADER, 0), (R.FOLLOWER, 9), (R.CANDIDATE, 0)):
        st = R.new_stats()
        lo = R.step(_leader(role=role, lead=lead), [], 0, 2, R.Config(), st)
        hi = R.step(_leader(role=role, lead=lead), [], 0, 4, R.Config(), st)
        assert lo.qflags == 0 and hi.qflags == R.QFLAG_HOST
        assert st["xf_ign_term"] == 1 and st["xf_host"] == 1
