"""k_long and the two-level scan of the follower pipeline, for
qb_dev_follower_step and qb_dev_follower_log_step, bit-exact against
follower_ref / append_ref on the real objects (tests/test_gpu_follower.py and
tests/test_gpu_follower_log.py's own run(): every in/out array, every output
over 0xA5 pre-fills, every counter):

  * more groups with a run above kInline = 16 than kLongBlocks = 256, so
    k_long's `q += gridDim.x` runs and a block sorts a short run in the LDS
    array a 4096-entry one just used (kLdsRun = 4096: 4096, 4095 and 2049 are
    the in-LDS limit and two non-powers of two);
  * runs of 4097, 5000 and 8193 records, past kLdsRun: the bitonic sort in
    the workspace (device-scope loads and stores, __threadfence);
  * G = 3 * 4096 + 5, past kScanPer = 4096: the scan's block sums and the
    add-back for the cnt table, and run_of's cnt[g - 1] across a block edge.

Terms rise through every long run, so records stepped in a wrong order answer
differently instead of cancelling out, and some long runs hold a stop near
their tail, so AFTER_STOP is counted from the strided loop.  With the log step
MsgApp records sit among the others and the long run walks the run table."""
import numpy as np
import pytest

from tests import append_pack as AP, append_ref as A, follower_pack as P, follower_ref as F
from tests.test_gpu_follower import run as run_plain
from tests.test_gpu_follower_log import run as run_log

pytestmark = pytest.mark.gpu
CFG = F.Config(10, False, True)      # (no lease: a higher-term vote is never dropped)
ROLE = F.FOLLOWER | F.ROLE_PROMOTABLE
both = pytest.mark.parametrize("log", [False, True], ids=["follower_step", "follower_log_step"])


def plain_node():
    return F.Node(term=1, lead=1, committed=2, last_index=40, last_term=1, role=ROLE,
                  election_elapsed=3, heartbeat_elapsed=2)


def log_node():
    return A.new_node([0, 1, 1], 1, term=1, lead=2, role=ROLE, election_elapsed=3,
                      heartbeat_elapsed=2)


def plain_run(rng, n, stop):
    """n records for one group, the term rising every third record."""
    recs = []
    for j in range(n):
        kind = int(rng.choice([F.HEARTBEAT, F.HEARTBEAT, F.VOTE, F.PREVOTE]))
        recs.append(F.Rec(kind, int(rng.integers(1, 4)), 1 + j // 3, int(rng.integers(0, 41)),
                          int(rng.integers(0, 300)), bool(rng.random() < 0.3)))
    if stop is not None and n >= 8:
        at = n - 1 - int(rng.integers(2, 7))
        t = 1 + at // 3
        recs[at] = (F.Rec(F.HOST, 2, t), F.Rec(F.TIMEOUT_NOW, 1, t),
                    F.Rec(F.HEARTBEAT, 1, t, 41 + stop, 0))[stop % 3]   # the last: commitTo past the log
    return recs


def log_run(rng, n, stop):
    """n records for one group over a shadow node that append_ref steps: the
    message term rises every third record, the entries' term six times over
    the run (eight runs at the most), appends at and below the end (the latter
    truncate once the term has risen), rejects past the end, heartbeats and
    pre-votes between them; a record that would stop is replaced."""
    sh = log_node()
    recs = []
    stop_at = n - 1 - int(rng.integers(2, 7)) if stop is not None and n >= 8 else -1
    for j in range(n):
        t, et = 10 + j // 3, 1 + (6 * j) // n
        li = sh.last_index
        if j == stop_at:
            lt = sh.last_term
            recs.append((F.Rec(F.HOST, 2, t), F.Rec(F.TIMEOUT_NOW, 2, t),
                         AP.app(2, t, li + 1, 0, [et]),                        # a gap: LOG_CONFLICT
                         AP.app(2, t, li, lt, [0, 0], li + 2),                 # zero terms "match": COMMIT_RANGE
                         AP.app(2, t, li, lt, list(range(lt + 1, lt + 10))))   # nine more runs: LOG_RUNS
                        [stop % 5])
            continue
        if j > stop_at >= 0:
            recs.append(F.Rec(F.HEARTBEAT, 2, t, 0, 1))
            continue
        r = rng.random()
        if r < 0.4:
            at = max(sh.committed, li - int(rng.integers(0, 5)))   # (mostly re-sends: a short log)
            rec = AP.app(2, t, at, sh.log_term(at), [et] * int(rng.integers(0, 3)), max(at, 2) - 2)
        elif r < 0.5:
            rec = AP.app(2, t, li + 2, et, [et])
        elif r < 0.8:
            rec = F.Rec(F.HEARTBEAT, 2, t, int(rng.integers(0, sh.committed + 1)), 1)
        else:
            rec = F.Rec(F.PREVOTE, 3, t + 1, li, sh.last_term, True)
        if A.step_batch([sh], [(0, rec)], CFG)["stop_at"][0] != F.NO_STOP:   # (nothing was applied)
            rec = F.Rec(F.HEARTBEAT, 2, t, 0, 1)
            A.step_batch([sh], [(0, rec)], CFG)
        recs.append(rec)
    return recs


def batch(log, lens, stops, seed):
    """One group per entry of ``lens`` with that many records, interleaved at
    random; stops: {group: which stop sits near the run's tail}."""
    rng = np.random.default_rng(seed)
    nodes = [log_node() if log else plain_node() for _ in lens]
    make = log_run if log else plain_run
    per_group = [make(rng, int(n), stops.get(g)) for g, n in enumerate(lens)]
    return nodes, P.interleave(per_group, rng)


def step(where, log, nodes, recs):
    return (run_log if log else run_plain)(where, nodes, recs, CFG)[1]


@both
def test_more_long_groups_than_long_blocks(log):
    """G = 1000: 770 groups with 17..40 records, three with 4096, 4095 and
    2049, the rest 0..16; M about 33k.  773 long groups over 256 blocks: about
    three runs each.  Every 13th long run stops near its tail."""
    rng = np.random.default_rng(7)
    lens = np.concatenate([rng.integers(17, 41, 770), [4096, 4095, 2049], rng.integers(0, 17, 227)])
    rng.shuffle(lens)
    assert (lens > 16).sum() == 773 > 3 * 256
    long_ = np.flatnonzero(lens > 16)
    stops = {int(g): k for k, g in enumerate(long_[::13])}
    stops[int(np.flatnonzero(lens == 4095)[0])] = 1
    nodes, recs = batch(log, lens, stops, 8)
    assert 30000 < len(recs) < 36000
    want = step("long blocks", log, nodes, recs)
    st = want["stats"]
    assert (want["stop_at"][list(stops)] != F.NO_STOP).all() and st["after_stop"] >= 2 * len(stops)
    kinds = F.FFLAG_STOPS | (A.FFLAG_STOPS if log else 0)     # every stop the call has was taken
    assert int(np.bitwise_or.reduce(want["gflags"][list(stops)])) & kinds == kinds
    assert st["became_follower"] > 5000 and st["heartbeats"] > 5000
    if log:
        assert st["app_accepted"] > 5000 and st["app_rejected"] > 1000 and st["app_truncated"] > 300


@both
def test_runs_past_the_lds_limit(log):
    """Groups with 4097, 5000 and 8193 records among 300 with 0..8, shuffled
    together; the 5000-record run stops near its tail.  The thresholds are
    somewhat under half of what the reference counts (follower step: 5849
    became_follower, 9207 heartbeats; log step: 6170, 5417, and 7415
    accepted appends of which 207 truncate)."""
    rng = np.random.default_rng(17)
    lens = np.concatenate([[4097, 5000, 8193], rng.integers(0, 9, 300)])
    rng.shuffle(lens)
    hot = {int(n): int(np.flatnonzero(lens == n)[0]) for n in (4097, 5000, 8193)}
    nodes, recs = batch(log, lens, {hot[5000]: 0}, 18)
    want = step("past kLdsRun", log, nodes, recs)
    st = want["stats"]
    print("reference counters:", st)
    assert want["stop_at"][hot[5000]] != F.NO_STOP and 2 <= st["after_stop"] <= 6
    assert want["stop_at"][hot[4097]] == F.NO_STOP and want["stop_at"][hot[8193]] == F.NO_STOP
    assert st["became_follower"] > 2800
    assert st["heartbeats"] > (2600 if log else 4300)
    if log:
        assert st["app_accepted"] > 3400 and st["app_truncated"] > 50


@both
def test_more_than_one_scan_block(log):
    """G = 3 * 4096 + 5: records in the groups on both sides of every scan
    block edge, in the last group and in 2,000 others; some 10,000 groups
    stay empty (gflags 0, stop_at UINT32_MAX, nothing else touched)."""
    G = 3 * 4096 + 5
    rng = np.random.default_rng(27)
    edges = [0, 4095, 4096, 4097, 8191, 8192, 12287, 12288, G - 1]
    lens = np.zeros(G, np.int64)
    lens[rng.choice(G, 2000, replace=False)] = rng.integers(1, 4, 2000)
    lens[edges] = [3, 5, 9, 4, 6, 1, 3, 8, 4]
    nodes, recs = batch(log, lens, {4096: 0, 12288: 1}, 28)
    want = step("scan blocks", log, nodes, recs)
    quiet = lens == 0
    assert quiet.sum() > 10000
    assert not want["gflags"][quiet].any() and (want["stop_at"][quiet] == F.NO_STOP).all()
    assert (want["stop_at"][[4096, 12288]] != F.NO_STOP).all()
