"""qb_dev_follower_snapshot on the device against tests/snapshot_ref.py,
bit-exact: every state column, every output column (and behind the records the
pre-filled elements a call must leave alone), the run rows a restore must
leave alone, and the stats.  All comparisons are integer equality."""
import functools
import json

import numpy as np
import pytest
import torch

from etcd_amd.quorum import snapshot as qs
from tests import snapshot_pack as P, snapshot_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = 300
SIZES = (0, 1, 63, 64, 65, 256, 257)
BAD_AT = 5        # the record that names no group, where a call has that many
SLACK = 3         # output elements behind the records
_SIGNED = {np.uint64: np.int64, np.uint32: np.int32, np.uint16: np.int16, np.uint8: np.uint8}


@functools.lru_cache(maxsize=None)
def base_cases():
    return P.seeded_cases(G, 20241)


def records_for(R, clamp):
    """R records on shuffled distinct groups (one of them a bad group), and
    the ConfState total the call is given (``clamp``: 10 below the arrays')."""
    nodes, msgs, _ = base_cases()
    order = np.random.default_rng(100 + R).permutation(G)[:R]
    recs = [(int(g), msgs[g]) for g in order]
    if R > BAD_AT:
        recs[BAD_AT] = (G + R % 3, recs[BAD_AT][1])
    arrays = P.pack_records(recs)
    C = len(arrays["cs_id"]) - (10 if clamp else 0)
    assert C >= 0
    return nodes, recs, arrays, C


def reference(R, clamp, pending):
    nodes, recs, arrays, C = records_for(R, clamp)
    after, ref = P.run_reference(nodes, P.clamped(recs, C), pending=pending)
    return nodes, after, ref, arrays, C


PARAMS = [(R, False, True) for R in SIZES] + [(65, True, True), (257, True, False),
                                              (64, False, False), (256, False, False)]


def test_inputs_reach_every_flag_counter_and_case():
    """On the CPU: the inputs of the tests below make the reference produce
    every QB_SNF_* bit and a non-zero value of every counter, and hold every
    case the device must meet, so none goes untested unnoticed."""
    seen, tot = 0, S.new_stats()
    for R, clamp, pending in PARAMS:
        _, _, ref, _, _ = reference(R, clamp, pending)
        for f in ref["sflags"]:
            seen |= f
        for k, v in ref["stats"].items():
            tot[k] += v
    assert seen == S.SNF_ALL, hex(seen)
    assert all(v > 0 for v in tot.values()), tot
    nodes, msgs, kinds = base_cases()
    assert {(n.state, n.promotable, n.role_other) for n in nodes} >= {
        (s, p, o) for s in range(4) for p in (False, True) for o in (0, 0x40)}
    assert {k[0] for k in kinds} == set(P.INDEX_KINDS) and {k[1] for k in kinds} == set(P.TERM_KINDS)
    assert {(k[2], k[3]) for k in kinds} >= {(c, s) for c in P.CS_KINDS for s in (1, 16, 40)}
    assert any(k[3] == 0 for k in kinds)
    assert {len(P.runs_of(n)) for n, k in zip(nodes, kinds) if k[0].startswith("boundary")} == set(
        range(1, P.MAX_RUNS + 1))
    assert any(m.index == S.U64 and m.sterm >= S.U64 - 1 for m in msgs)
    assert any(m.term == S.U64 for m in msgs)
    # a restore of a table with more than one run: rows 1.. must stay
    nodes257, after, ref, _, _ = reference(257, True, False)
    assert any(f & S.SNF_RESTORED and len(P.runs_of(nodes257[g])) > 1
               for f, (g, _) in zip(ref["sflags"], records_for(257, True)[1]) if g < G)
    # the clamp cuts IDs off the last records
    _, recs, arrays, C = records_for(257, True)
    assert int(arrays["cs_off"][-1]) > C


def run_on_device(nodes, arrays, C, pending, R):
    before = P.pack_nodes(nodes)
    ds = P.DeviceState(before, DEV, pending=pending)
    inbox = P.device_inbox(arrays, DEV, C=C)
    fill = lambda dt: torch.from_numpy(  # noqa: E731
        np.full(R + SLACK, P._FILLS[dt], dt).view(_SIGNED[dt])).to(DEV)
    out = qs.SnapshotResult(fill(np.uint16), fill(np.uint8), fill(np.uint64), fill(np.uint64),
                            torch.zeros(len(S.SSTAT_NAMES), dtype=torch.int64, device=DEV))
    qs.follower_snapshot(ds.groups, ds.log, ds.ready, ds.self_id, inbox, out=out)
    torch.cuda.synchronize()
    return before, ds, out


def compare(before, ds, out, after, ref, R, where):
    want = P.pack_out(ref, R + SLACK)
    got = {"sflags": out.sflags, "resp_type": out.resp_type, "resp_term": out.resp_term,
           "resp_index": out.resp_index}
    for k, dt in P.OUT.items():
        assert np.array_equal(got[k].cpu().numpy().view(dt), want[k]), (where, k)
    assert out.stats_dict() == ref["stats"], where
    want_state = P.pack_nodes(after, base=before)
    got_state = ds.numpy()
    for k in P.STATE:
        assert np.array_equal(got_state[k], want_state[k]), (where, k)


@pytest.mark.parametrize("R,clamp,pending", PARAMS)
def test_follower_snapshot_fuzz(R, clamp, pending):
    nodes, after, ref, arrays, C = reference(R, clamp, pending)
    before, ds, out = run_on_device(nodes, arrays, C, pending, R)
    compare(before, ds, out, after, ref, R, (R, clamp, pending))
    if not pending:  # the column the call was not given is not the call's to touch
        assert np.array_equal(ds.numpy()["pending"], before["pending"])


def test_restore_leaves_the_table_rows_behind_run_zero():
    """The restored groups' rows 1..7 of run_start / run_term hold what they
    held (spelled out; the fuzz's state comparison holds it too)."""
    R = 257
    nodes, after, ref, arrays, C = reference(R, False, True)
    before, ds, out = run_on_device(nodes, arrays, C, True, R)
    got = ds.numpy()
    restored = [int(g) for g, f in zip(arrays["group"], ref["sflags"]) if f & S.SNF_RESTORED]
    assert len(restored) > 20
    for k in P.ROWS:
        b, a = before[k].reshape(P.MAX_RUNS, G), got[k].reshape(P.MAX_RUNS, G)
        assert np.array_equal(a[1:, restored], b[1:, restored]), k
    assert ((got["meta"][restored] >> 16) & 0xF == 1).all()
    assert (got["meta"][restored] & ~np.uint32(0xF0000) == before["meta"][restored] & ~np.uint32(0xF0000)).all()
    assert (got["role"][restored] & 0x80 == 0).all()


def test_stats_accumulate_and_out_is_reused():
    nodes, after, ref, arrays, C = reference(65, False, True)
    before, ds, out = run_on_device(nodes, arrays, C, True, 65)
    # the same records again: what restored is old now, the rest as the
    # reference says
    again, ref2 = P.run_reference(after, P.clamped(records_for(65, False)[1], C),
                                  stats=dict(ref["stats"]))
    qs.follower_snapshot(ds.groups, ds.log, ds.ready, ds.self_id, P.device_inbox(arrays, DEV),
                         out=out)
    torch.cuda.synchronize()
    compare(before, ds, out, again, ref2, 65, "second call")
    assert ref2["stats"]["old"] > ref["stats"]["old"]


def test_golden_tables_on_the_device():
    """Every node and snapshot of the reference's tables as one batch."""
    from tests.test_snapshot_ref import golden, table_nodes
    cases = table_nodes(golden())
    assert len(cases) >= 14
    nodes = [n for n, _ in cases]
    recs = [(g, m) for g, (_, m) in enumerate(cases)]
    after, ref = P.run_reference(nodes, recs)
    assert sum(1 for f in ref["sflags"] if f & S.SNF_RESTORED) >= 9
    arrays = P.pack_records(recs)
    before, ds, out = run_on_device(nodes, arrays, len(arrays["cs_id"]), True, len(recs))
    compare(before, ds, out, after, ref, len(recs), "golden")


def test_wrapper_round_trip_from_conf_state_dicts():
    """SnapshotInbox.from_numpy packs the dicts as the test packer does, the
    responses carry the restatement's, and restored_conf_states names the
    restored records."""
    nodes, recs, arrays, _ = records_for(64, False)
    recs = [r for r in recs if r[0] < G]
    after, ref = P.run_reference(nodes, recs)
    ds = P.DeviceState(P.pack_nodes(nodes), DEV)
    a = P.pack_records(recs)
    inbox = qs.SnapshotInbox.from_numpy(a["group"], a["from"], a["term"], a["snap_index"],
                                        a["snap_term"], [m.cs for _, m in recs], device=DEV)
    for k in ("cs_off", "cs_id", "cs_set"):
        got = inbox.t[k].cpu().numpy().view(a[k].dtype)[:len(a[k])]
        assert np.array_equal(got, a[k]), k
    res = qs.follower_snapshot(ds.groups, ds.log, ds.ready, ds.self_id, inbox)
    torch.cuda.synchronize()
    assert res.flags().tolist() == ref["sflags"]
    want = [{"i": i, "group": recs[i][0], "type": S.MSG_APP_RESP, "to": recs[i][1].frm,
             "term": ref["resp_term"][i], "index": ref["resp_index"][i]}
            for i in range(len(recs)) if ref["resp_type"][i]]
    assert list(res.responses()) == want
    groups, css = qs.restored_conf_states(inbox, res.sflags)
    idx = [i for i, f in enumerate(ref["sflags"]) if f & S.SNF_RESTORED]
    assert groups.tolist() == [recs[i][0] for i in idx] and css == [recs[i][1].cs for i in idx]
    assert json.dumps(css)  # plain dicts of lists: confchange.restore's shape
