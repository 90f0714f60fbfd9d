"""tests/replicate.py against the slow path, once per entry point: K = 3 copies
of a G0 = 40 base — active, idle, active — built as 3 * G0 deep-copied node
objects (and interleaved records), packed and stepped by the Python reference,
must equal the replicated base in every array, in and out, and in the stats.
A missed index remap fails here and not as a false mismatch on the device.
All comparisons are integer equality."""
import copy

import numpy as np
import pytest

from tests import append_pack as AP, campaign_pack as CP, follower_pack as FP
from tests import propose_pack as PP, propose_ref as PR, request_pack as QP, request_ref as QR
from tests import replicate as X, tick_pack as TP

G0, WHICH = 40, (0, 1, 0)
K = len(WHICH)
ACT = [c for c, w in enumerate(WHICH) if w == 0]


def check(slow: X.Case, fast: X.Case):
    assert slow.G == fast.G == K * G0 and slow.M == fast.M
    assert X.mismatches(fast.inp, slow.inp) == []
    assert len(slow.calls) == len(fast.calls)
    for (fa, fs), (sa, ss) in zip(fast.calls, slow.calls):
        assert X.mismatches(fa, sa) == []
        assert fs == ss
    for _, (kind, v) in fast.inp.items():
        if kind == X.ROWS:
            assert v.shape[1] == K * G0


def copies(active, idle):
    return [copy.deepcopy(n) for w in WHICH for n in (idle if w else active)]


def cat(active, idle):
    return {k: np.concatenate([idle[k] if w else active[k] for w in WHICH]) for k in active}


def test_kinds_on_a_worked_example():
    """G0 = 2, S0 = 3, K = 2, by hand."""
    assert X.rep_off(np.array([0, 1, 3], np.uint32), 2).tolist() == [0, 1, 3, 4, 6]
    rows = np.array([10, 11, 20, 21], np.uint64)              # rows (10 11) and (20 21)
    idle = np.array([0, 0, 0, 0], np.uint64)
    assert X.rep_rows([rows, idle], [0, 1], 2).tolist() == [[10, 11, 0, 0], [20, 21, 0, 0]]
    assert X.rep_rec(np.array([7, 8]), 2).tolist() == [7, 7, 8, 8]
    assert X.rep_rec_group(np.array([1, 2, 0xFFFFFFFF], np.uint32), [0, 2], 3, 2).tolist() == \
        [1, 5, 6, 6, 0xFFFFFFFF, 0xFFFFFFFF]                  # group 2 = G0 is a bad group: stays one
    eo = np.array([0, 2, 2, 3], np.uint32)
    assert X.rep_ent_off(eo, 2).tolist() == [0, 2, 4, 4, 4, 5, 6]
    assert X.rep_ent(np.array([5, 6, 9]), eo, 2).tolist() == [5, 6, 5, 6, 9, 9]
    stop = np.array([X.NO_STOP, 4], np.uint32)
    none = np.full(2, X.NO_STOP, np.uint32)
    assert X.rep_stop([stop, none], [1, 0, 0], [1, 2]).tolist() == \
        [X.NO_STOP, X.NO_STOP, X.NO_STOP, 8, X.NO_STOP, 9]
    assert X.rep_stats([{"a": 2}, {"a": 1}], [0, 1, 1]) == {"a": 4}


def test_tick():
    rng = np.random.default_rng(5)
    nodes = TP.random_nodes(rng, G0, 4, 1, 1)
    idle = X.tick_idle(nodes)
    fast = X.replicate([X.tick_case(nodes, 4, 1, 1, 1), X.tick_case(idle, 4, 1, 1, 1)], WHICH)
    check(X.tick_case(copies(nodes, idle), 4, 1, 1, 1), fast)
    assert fast.calls[1][1]["beats"] and fast.calls[1][1]["hups"]


@pytest.mark.parametrize("pre_vote", [0, 1])
def test_campaign(pre_vote):
    rng = np.random.default_rng(6 + pre_vote)
    nodes = CP.random_nodes(rng, G0, readq_cap=4)
    action = CP.random_actions(rng, G0)
    zero = np.zeros(G0, np.uint8)
    fast = X.replicate([X.campaign_case(nodes, action, pre_vote, 4),
                        X.campaign_case(nodes, zero, pre_vote, 4)], WHICH)
    slow = X.campaign_case(copies(nodes, nodes),
                           np.concatenate([zero if w else action for w in WHICH]), pre_vote, 4)
    check(slow, fast)
    assert fast.calls[0][1]["vote_requests"]


def test_propose():
    rng = np.random.default_rng(8)
    cfg = PR.Config(max_uncommitted_size=100)
    nodes = PP.random_nodes(rng, G0)
    inp = PP.random_inputs(rng, G0)
    none = PP.inputs(np.zeros(G0, np.uint8), np.zeros(G0, np.uint32))
    fast = X.replicate([X.propose_case(nodes, inp, cfg), X.propose_case(nodes, none, cfg)], WHICH)
    check(X.propose_case(copies(nodes, nodes), cat(inp, none), cfg), fast)
    assert fast.calls[0][1]["msg_app"]


def test_requests():
    rng = np.random.default_rng(9)
    cfg = QR.Config(readq_cap=4, max_reads=3)
    nodes = QP.random_nodes(rng, G0, 4)
    inp = QP.random_inputs(rng, nodes, 3)
    none = X.requests_idle_inputs(G0, 3)
    fast = X.replicate([X.requests_case(nodes, inp, cfg), X.requests_case(nodes, none, cfg)], WHICH)
    # the slow path's k-major inputs: request k of group g of copy c at k * G + c * G0 + g
    G = K * G0
    big = X.requests_idle_inputs(G, 3)
    for c in ACT:
        for g in range(G0):
            big["n_reads"][c * G0 + g] = inp["n_reads"][g]
            big["xf_from"][c * G0 + g] = inp["xf_from"][g]
            big["xf_term"][c * G0 + g] = inp["xf_term"][g]
            for k in range(3):
                big["rd_ctx"][k * G + c * G0 + g] = inp["rd_ctx"][k * G0 + g]
                big["rd_from"][k * G + c * G0 + g] = inp["rd_from"][k * G0 + g]
    check(X.requests_case(copies(nodes, nodes), big, cfg), fast)
    st = fast.calls[0][1]
    assert st["bcast"] and st["xf_started"]


def test_follower():
    nodes, recs = FP.fuzz(3, G=G0, M=200)
    cfg = FP.fuzz_config(True, True)
    base = X.follower_case(nodes, recs, cfg)
    fast = X.replicate([base, X.follower_case(nodes, [], cfg)], WHICH)
    slow = X.follower_case(copies(nodes, nodes), X.interleaved_records(recs, ACT, K, G0), cfg)
    check(slow, fast)
    stop = base.calls[0][0]["stop_at"][1]
    assert (stop != X.NO_STOP).sum() >= 3 and base.calls[0][1]["bad_group"]   # both remaps ran


def test_follower_log():
    nodes, recs = AP.fuzz(4, G=G0, M=200)
    cfg = FP.fuzz_config(True, False)
    base = X.follower_log_case(nodes, recs, cfg)
    fast = X.replicate([base, X.follower_log_case(nodes, [], cfg)], WHICH)
    slow = X.follower_log_case(copies(nodes, nodes), X.interleaved_records(recs, ACT, K, G0), cfg)
    check(slow, fast)
    st = base.calls[0][1]
    assert (base.calls[0][0]["stop_at"][1] != X.NO_STOP).sum() >= 3 and st["bad_group"]
    assert st["entries_appended"] and len(base.arr("ent_term")) > 100
