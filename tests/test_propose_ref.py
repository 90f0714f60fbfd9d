"""tests/propose_ref.py against the reference's own tests of the proposal
path (tests/golden/propose_tables.json, transcribed by make_propose_golden.py)
and against oracle/leader_ref.py's LeaderGroup.propose on the subset that
helper covers.  No GPU."""
import copy

import numpy as np
import pytest

from oracle import leader_ref as L
from tests import leader_pack, propose_pack as P, propose_ref as R

SCENARIOS = P.load_tables()["scenarios"]


def ref_apply(n, cfg, inp, k, repeat):
    return R.step(n, *inp, cfg, R.new_stats())


@pytest.mark.parametrize("sc", SCENARIOS, ids=[s["name"] for s in SCENARIOS])
def test_golden_scenarios(sc):
    P.replay(sc, ref_apply)


def test_the_tables_cover_the_listed_reference_tests():
    names = {s["name"].split("/")[0] for s in SCENARIOS}
    assert names >= {"TestProposal", "TestProposalByProxy", "TestUncommittedEntryLimit",
                     "TestStepConfig", "TestStepIgnoreConfig", "TestNewLeaderPendingConfig",
                     "TestLeaderTransferIgnoreProposal", "TestSingleNodeCommit",
                     "TestLeaderStartReplication", "TestMsgAppFlowControlFull",
                     "TestSendAppendForProgressProbe", "TestSendAppendForProgressReplicate",
                     "TestSendAppendForProgressSnapshot", "TestDisableProposalForwarding",
                     "probe_and_replicate"}


def test_the_json_is_what_the_generator_writes():
    from tests.golden import make_propose_golden as M
    assert M.SCENARIOS == SCENARIOS


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_against_the_oracle_helper(seed):
    """LeaderGroup.propose (appendEntry + bcastAppend over the run table, no
    drops, conf changes or size limits) and the restatement (a list of terms)
    agree on every plain proposal at a leader: Progress, rings, committed,
    the log's end and runs, and the messages."""
    rng = np.random.default_rng(seed)
    seen = 0
    for n in P.random_nodes(rng, 400):
        c, g = n.camp, n.group
        if c.state != R.LEADER or c.own >= g.n_slots or g.transferee != L.NO_SLOT:
            continue
        if n.terms[-1] != g.term and len(g.log.runs) >= R.MAX_RUNS:
            continue
        k = int(rng.integers(1, 6))
        o = copy.deepcopy(g)
        o.propose(k)
        st = R.new_stats()
        pf, msgs = R.step(n, R.PROP_ENTRIES, k, 0, 0, 0, R.Config(), st)
        n.sync()
        assert pf & R.PFLAG_APPENDED and pf & R.PFLAG_BCAST and not pf & R.PFLAG_DROPPED
        assert leader_pack.state_key(o) == leader_pack.state_key(g)
        assert (o.log.last, o.log.runs) == (g.log.last, g.log.runs)
        assert [m.key() for m in o.msgs] == msgs
        assert st["msg_app"] + st["msg_snap"] == len(msgs) and st["entries"] == k
        seen += 1
    assert seen > 150
