"""tests/switch_ref.py reproduces every case of tests/golden/switch_tables.json
(the reference's own switchToConfig tests and interaction traces), and the
seeded batches of tests/switch_pack.py reach every branch the GPU tests are
meant to cover.  No GPU."""
import copy

import numpy as np
import pytest

from tests import switch_pack as P, switch_ref as R

CASES = P.load_tables()["cases"]
FLAGS = {"switched": R.SWFLAG_SWITCHED, "committed": R.SWFLAG_COMMITTED, "sent": R.SWFLAG_SENT,
         "transfer_aborted": R.SWFLAG_TRANSFER_ABORTED, "self_removed": R.SWFLAG_SELF_REMOVED,
         "self_learner": R.SWFLAG_SELF_LEARNER, "vote_dropped": R.SWFLAG_VOTE_DROPPED,
         "host": R.SWFLAG_HOST}


def pack_case(c):
    """(arrays, action, readq_cap) of a golden case, G = 1."""
    x = P.group(c["old_ids"], c["ids"], c["voters"], c["voters_out"], self_id=c["self"],
                role=c["role"], term=c["term"], terms=c["terms"], first=c["first"],
                committed=c["committed"], progress=c["progress"], transferee=c["transferee"],
                cap=c.get("inflight_cap", P.INFLIGHT_CAP))
    return P.pack([x], 0, c.get("inflight_cap", P.INFLIGHT_CAP)), \
        np.array([c["action"]], np.uint8), 0


def check_case(c, a, swflags, msgs):
    """a: the arrays behind the call; msgs: (type, to slot, index, log_term,
    commit, n) of group 0."""
    e, ids, where = c["expect"], c["ids"], c["name"]
    want = 0
    for f in e["flags"]:
        want |= FLAGS[f]
    assert swflags == want, f"{where}: swflags {swflags:#x}, want {want:#x}"
    got = [[t, ids[to], i, lt, cm, n] for t, to, i, lt, cm, n in msgs]
    assert got == e["msgs"], f"{where}: messages {got}, want {e['msgs']}"
    meta, cfg = int(a["meta"][0]), int(a["cfg"][0])
    own, xf = meta & 0xFF, (meta >> 8) & 0xFF
    voters = [i for k, i in enumerate(ids) if ((cfg | cfg >> 16) >> k) & 1]
    if "voters" in e:
        assert voters == e["voters"], where
    if "learners" in e:
        assert [i for i in ids if i not in voters] == e["learners"], where
    present = e.get("own_present", True)
    assert (own != 0xFF) == present, f"{where}: own slot {own:#x}"
    if present:
        assert ids[own] == c["self"], where
    if "is_learner" in e:
        assert (present and c["self"] not in voters) == e["is_learner"], where
    if "transferee_after" in e:
        assert (ids[xf] if xf != 0xFF else 0) == e["transferee_after"], where
    if "committed_after" in e:
        assert int(a["committed"][0]) == e["committed_after"], where
    if "role_after" in e:
        assert int(a["role"][0]) & 3 == e["role_after"], where
    for i, w in e.get("progress_after", {}).items():
        j = int(a["off"][0]) + ids.index(int(i))
        got = {"match": int(a["match"][j]), "next": int(a["next"][j]),
               "probe_sent": bool(int(a["pstate"][j]) & R.PROBE_SENT)}
        for k, v in w.items():
            assert got[k] == v, f"{where}: progress[{i}].{k} = {got[k]}, want {v}"


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_cases(case):
    a, action, Q = pack_case(case)
    out, st = R.new_out(1, int(a["old_off"][-1]), int(a["off"][-1])), R.new_stats()
    sent = P.ref_call(a, action, Q, out, st)
    check_case(case, a, int(out["swflags"][0]), sent[0])
    # the slot map is the rank of each surviving old ID in the new list
    want = [case["ids"].index(i) if i in case["ids"] else 0xFF for i in sorted(case["old_ids"])]
    assert out["slot_map"][:len(want)].tolist() == want


def test_golden_file_is_what_the_generator_writes():
    from tests.golden import make_switch_golden as M
    assert P.load_tables() == {"cases": M.CASES}


@pytest.mark.parametrize("Q", [0, 1, 16])
def test_fuzz_batches_reach_every_branch(Q):
    """The dense batches of tests/test_gpu_switch.py (same seeds): every
    counter moves, both kinds of send happen, peers below first_index are met
    under both sendIfEmpty values, and a stopped group keeps every byte."""
    rng = np.random.default_rng(1000 + Q + 7)
    a, action = P.random_batch(rng, 300, Q)
    before = copy.deepcopy(a)
    out, st = R.new_out(300, int(a["old_off"][-1]), int(a["off"][-1])), R.new_stats()
    P.ref_call(a, action, Q, out, st)
    for k in ("switched", "restores", "commits", "bcast", "probed", "msg_app", "transfer_aborted",
              "self_removed", "self_learner", "vote_dropped", "host", "bad_action"):
        assert st[k] > 0, (k, st)
    sf = out["swflags"][:300]
    assert ((sf & R.SWFLAG_SWITCHED) != 0).sum() == st["switched"]
    for g in np.flatnonzero(sf == R.SWFLAG_HOST):
        s0, s1 = int(a["off"][g]), int(a["off"][g + 1])
        for k in P.INOUT:
            if k in ("meta", "committed", "votes"):
                assert a[k][g] == before[k][g]
            elif k == "rq_meta":
                assert np.array_equal(a[k][g * Q:(g + 1) * Q], before[k][g * Q:(g + 1) * Q])
            elif k != "infl_buf":
                assert np.array_equal(a[k][s0:s1], before[k][s0:s1])
        assert (out["msg_type"][s0:s1] == R.FILL8).all()
    # followers under SW_RESTORE ran MaybeUpdate(next - 1) on their own slot
    rest = [g for g in range(300) if action[g] == R.SW_RESTORE and sf[g] & R.SWFLAG_SWITCHED
            and int(a["role"][g]) & 3 != R.LEADER and int(a["meta"][g]) & 0xFF != 0xFF]
    assert rest
    for g in rest:
        j = int(a["off"][g]) + (int(a["meta"][g]) & 0xFF)
        assert int(a["match"][j]) >= int(a["next"][j]) - 1


def test_snapshot_batch_sends_snapshots():
    rng = np.random.default_rng(77)
    a, action = P.random_batch(rng, 300, 1)
    out, st = R.new_out(300, int(a["old_off"][-1]), int(a["off"][-1])), R.new_stats()
    P.ref_call(a, action, 1, out, st)
    assert st["msg_snap"] > 0


def test_every_vote_pattern_on_a_removed_slot():
    """All 64 voted x granted patterns over a removed, a moved and a kept
    slot: the bits of the removed slot go, the others move with their IDs, and
    only a dropped voted bit raises VOTE_DROPPED."""
    a, action, want, dropped = P.vote_patterns()
    G = len(action)
    out, st = R.new_out(G, int(a["old_off"][-1]), int(a["off"][-1])), R.new_stats()
    P.ref_call(a, action, 0, out, st)
    assert np.array_equal(a["votes"], want)
    assert np.array_equal((out["swflags"][:G] & R.SWFLAG_VOTE_DROPPED) != 0, dropped)
    assert ((a["meta"] & 0xFF) == 1).all() and st["vote_dropped"] == int(dropped.sum())
