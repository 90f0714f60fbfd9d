"""qb_dev_switch_config on the device against tests/switch_ref.py, bit-exact:
every in/out array (meta, committed, votes, rq_meta, the new Progress and its
rings), every array the call only reads, swflags, slot_map and the message
columns including the elements a call must leave untouched (pre-filled with
0xA5...), and the accumulated stats.  All comparisons are integer equality."""
import numpy as np
import pytest

from tests import switch_pack as P, switch_ref as R

pytestmark = pytest.mark.gpu

CASES = P.load_tables()["cases"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_cases_on_device(case):
    """The reference's cases, G = 1 each, through the public wrapper: the
    device equals switch_ref, and the transcribed expectations hold for what
    the device produced."""
    from tests import switch_dev as D
    from tests.test_switch_ref import check_case, pack_case
    a, action, Q = pack_case(case)
    run = D.run_batch(a, action, Q, case.get("inflight_cap", P.INFLIGHT_CAP), case["name"])
    got = {k: v for k, v in run.device_arrays().items()}
    msgs = run.out.messages(0)
    assert msgs == run.sent[0]
    check_case(case, got, int(run.out.swflags[0].item()), msgs)


@pytest.mark.parametrize("Q", [0, 1, 16])
@pytest.mark.parametrize("p_act", [1.0, 0.01], ids=["dense", "sparse"])
def test_fuzz(p_act, Q):
    """G = 300 (two tiles, one partial), 1..16 slots: adds, removes,
    promotions, demotions, joint configs, the own slot first / last / removed,
    a transferee kept / demoted / removed, pending reads, votes on removed
    slots, both stops, Probe / full-ring Replicate / Snapshot peers, next below
    first_index under both sendIfEmpty values, restores at followers."""
    from tests import switch_dev as D
    rng = np.random.default_rng(1000 + Q + int(p_act * 7))
    a, action = P.random_batch(rng, 300, Q, p_act=p_act)
    if p_act < 1:
        action[[3, 299]] = R.SW_SWITCH
    run = D.run_batch(a, action, Q, where=f"fuzz Q={Q} p={p_act}")
    if p_act == 1.0:      # the batch reaches every branch the issue lists
        st = run.stats
        for k in ("switched", "restores", "commits", "bcast", "probed", "msg_app",
                  "transfer_aborted", "self_removed", "self_learner", "vote_dropped", "host",
                  "bad_action"):
            assert st[k] > 0, (k, st)


def test_fuzz_snapshots_and_second_call():
    """A batch whose peers lag behind first_index (MsgSnap behind a commit,
    nothing behind a probe), then a second call into the same outputs: the
    new config against itself, so the renumbering is the identity, and the
    stats accumulate."""
    from tests import switch_dev as D
    rng = np.random.default_rng(77)
    a, action = P.random_batch(rng, 300, 1)
    run = D.run_batch(a, action, 1, where="first")
    assert run.stats["msg_snap"] > 0
    first = run.ref_out["swflags"][:300].copy()
    # switch again from the new config to itself
    run.a["old_off"], run.a["old_ids"] = run.a["off"].copy(), run.a["ids"].copy()
    run.old, run.S0 = run.new, run.S
    grow = lambda v, fill: np.concatenate([v, np.full(max(run.S - len(v), 0), fill, v.dtype)])  # noqa: E731
    run.ref_out["slot_map"] = grow(run.ref_out["slot_map"], R.FILL8)[:max(run.S, 1)]
    import torch
    run.out.slot_map = torch.from_numpy(run.ref_out["slot_map"].copy()).to(D.DEV)
    sf = run.switch(action, "second")
    # (a group the first call stopped still holds its old slots' words)
    assert not (sf[(first & R.SWFLAG_SWITCHED) != 0] & R.SWFLAG_VOTE_DROPPED).any()


def test_wrapper_refuses_mistyped_short_and_strided_tensors():
    """On the device the wrapper's checks reach dtype, length and contiguity:
    each is refused before the C call, and the state stays as it was."""
    import torch
    from etcd_amd import _lib
    from tests import switch_dev as D
    a, action = P.random_batch(np.random.default_rng(3), 8, 0)
    run = D.DeviceRun(a)
    act = D._dev(action, np.uint8)
    before = run.device_arrays()
    good = run.new.t["next"]
    for bad in (good.to(torch.int32), good[:-1], torch.stack([good, good], 1)[:, 0]):
        run.new.t["next"] = bad
        with pytest.raises(_lib.QuorumBatchError, match="next"):
            D.qs.switch_config(run.lg, run.es, run.old, run.new, act, out=run.out)
    run.new.t["next"] = good
    with pytest.raises(_lib.QuorumBatchError, match="action"):
        D.qs.switch_config(run.lg, run.es, run.old, run.new, act[:-1], out=run.out)
    after = run.device_arrays()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    run.switch(action, "after the refusals")


def test_every_vote_pattern_on_a_removed_slot():
    """All 64 voted x granted patterns over a removed, a moved and a kept slot
    (tests/switch_pack.py vote_patterns): the device equals the reference and
    the table of expected words."""
    from tests import switch_dev as D
    a, action, want, dropped = P.vote_patterns()
    run = D.run_batch(a, action, 0, where="vote patterns")
    G = len(action)
    assert np.array_equal(run.es.numpy()["votes"], want)
    sf = run.out.swflags.cpu().numpy()[:G]
    assert np.array_equal((sf & R.SWFLAG_VOTE_DROPPED) != 0, dropped)


def test_adopt_false_leaves_the_table_on_its_old_tensors():
    """With adopt=False the call does the same work, but the LeaderGroups table
    keeps its old off / cfg / Progress tensors until the host has dealt with
    the groups the call did not renumber; the messages index the new table."""
    from tests import switch_dev as D
    a, action = P.random_batch(np.random.default_rng(12), 40, 0)
    run = D.DeviceRun(a)
    off0, S0 = run.lg.t["off"], run.lg.S
    res = D.qs.switch_config(run.lg, run.es, run.old, run.new, D._dev(action, np.uint8),
                             adopt=False, out=run.out)
    assert run.lg.t["off"] is off0 and run.lg.S == S0 and res.table is run.new
    ref_out, st = R.new_out(40, run.S0, run.S), R.new_stats()
    sent = P.ref_call(run.a, action, 0, ref_out, st)
    assert res.stats_dict() == st
    assert [res.messages(g) for g in range(40)] == sent
    assert np.array_equal(D.ql._to_np(run.new.t["next"], np.uint64, run.S), run.a["next"][:run.S])


def test_single_group():
    from tests import switch_dev as D
    rng = np.random.default_rng(5)
    for _ in range(4):
        a, _ = P.random_batch(rng, 1, 2)
        D.run_batch(a, np.array([R.SW_SWITCH], np.uint8), 2, where="G=1")


def test_idle_tile_and_idle_call():
    """A tile in which no group acts writes only its swflags; so does a call
    with no acting group at all."""
    from tests import switch_dev as D
    rng = np.random.default_rng(9)
    a, action = P.random_batch(rng, 600, 0)
    action[256:512] = R.SW_NONE
    run = D.run_batch(a, action, 0, where="idle tile")
    assert not run.ref_out["swflags"][256:512].any()
    a, action = P.random_batch(rng, 300, 0, p_act=0.0)
    action[action > R.SW_RESTORE] = R.SW_NONE
    run = D.run_batch(a, action, 0, where="idle call")
    assert run.out.stats_dict() == R.new_stats()
