"""qb_dev_follower_snapshot where every workgroup takes a second trip: a base
of 1031 groups, a record each (shuffled) and one record of no group, laid end
to end K times (tests/snapshot_pack.py's layout over tests/replicate.py's
per-kind functions), so the reference runs on the base only and the expectation
is a few numpy calls.  Bit-exact: every output column, every state column and
the stats."""
import numpy as np
import pytest
import torch

from etcd_amd.quorum import snapshot as qs
from tests import snapshot_pack as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
G0 = 1031
TILE = 256          # records per tile (qb_snapshot.hip: a thread per record, kBlock threads)
GRID_CAP = 2048     # kStreamBlocks (qb_span_tile.h): the most workgroups a launch has
K = 509
G = K * G0
R0 = G0 + 1
R = K * R0


def test_the_size_reaches_the_second_trip():
    assert R > GRID_CAP * TILE + TILE      # kStreamBlocks tiles and one more


def test_follower_snapshot_over_half_a_million_records():
    nodes, msgs, _ = P.seeded_cases(G0, 777)
    order = np.random.default_rng(5).permutation(G0)
    recs = [(int(g), msgs[g]) for g in order]
    recs.insert(400, (G0 + 2, msgs[0]))                    # a group outside every copy
    assert len(recs) == R0
    after, ref = P.run_reference(nodes, recs)
    assert all(v > 0 for v in ref["stats"].values()), ref["stats"]
    before = P.pack_nodes(nodes)
    ds = P.DeviceState(P.lay_state(before, K, G0), DEV)
    rec_arrays = P.lay_records(P.pack_records(recs), K, G0)
    assert len(rec_arrays["group"]) == R and int(rec_arrays["group"].max()) >= G
    inbox = P.device_inbox(rec_arrays, DEV)
    out = qs.new_snapshot_result(R, DEV)
    for t in (out.sflags, out.resp_type, out.resp_term, out.resp_index):
        t.fill_(0x5A)
    qs.follower_snapshot(ds.groups, ds.log, ds.ready, ds.self_id, inbox, out=out,
                         check_distinct=False)   # (distinct by construction; np.unique of R is slow)
    torch.cuda.synchronize()
    want = P.lay_out({k: v[:R0] for k, v in P.pack_out(ref, R0).items()}, K)
    got = {"sflags": out.sflags, "resp_type": out.resp_type, "resp_term": out.resp_term,
           "resp_index": out.resp_index}
    for k, dt in P.OUT.items():
        assert np.array_equal(got[k].cpu().numpy().view(dt), want[k]), k
    assert out.stats_dict() == {k: K * v for k, v in ref["stats"].items()}
    want_state = P.lay_state(P.pack_nodes(after, base=before), K, G0)
    got_state = ds.numpy()
    for k in P.STATE:
        assert np.array_equal(got_state[k], want_state[k]), k
