"""qb_dev_switch_config where every workgroup takes a second tile, and over a
table with gaps whose tile span exceeds the staged owner map.  The large batch
is a base of 1032 groups laid end to end 509 times (tests/switch_pack.py
``lay``), so the reference runs on the base only and the expectation is a few
numpy calls.  Bit-exact: every output, every in/out array and the stats."""
import copy

import numpy as np
import pytest

from tests import switch_pack as P, switch_ref as R

pytestmark = pytest.mark.gpu
TILE = 256          # groups per tile (kBlock)
GRID_CAP = 2048     # kStreamBlocks (qb_span_tile.h): the most workgroups a launch has
SPAN_CAP = 4096     # kSpanCap: the slots a staged tile holds
G = GRID_CAP * TILE + 1000
G0, K = 1032, 509
Q = 2


def test_the_size_reaches_the_second_tile():
    assert G0 * K == G and G > GRID_CAP * TILE + TILE


def test_switch_config_over_half_a_million_groups():
    from tests import switch_dev as D
    rng = np.random.default_rng(31)
    a0, act0 = P.random_batch(rng, G0, Q)
    a1 = copy.deepcopy(a0)
    out1, st = R.new_out(G0, int(a0["old_off"][-1]), int(a0["off"][-1])), R.new_stats()
    P.ref_call(a1, act0, Q, out1, st)
    assert st["commits"] and st["probed"] and st["host"] and st["msg_app"], st
    run = D.DeviceRun(P.lay(a0, K, Q), Q)
    assert run.G == G
    run.switch(np.tile(act0, K), "stride",
               expected=(P.lay(a1, K, Q), P.lay(out1, K), {k: K * v for k, v in st.items()}))


def test_gapped_table_takes_the_unstaged_path():
    """Every group holds 16 members and one unused element behind them, so a
    full tile spans 256 * 17 slots: above kSpanCap, each thread walks its own
    group's slots in the global arrays.  The unused elements keep their bytes."""
    from tests import switch_dev as D
    rng = np.random.default_rng(32)
    a, action = P.random_batch(rng, 300, Q, n_new=16, pad=1)
    assert int(a["off"][TILE]) - int(a["off"][0]) > SPAN_CAP
    run = D.run_batch(a, action, Q, where="gapped")
    assert run.stats["msg_app"] and run.stats["commits"] and run.stats["probed"], run.stats
    pads = np.arange(16, 300 * 17, 17)
    assert (run.ref_out["msg_type"][pads] == R.FILL8).all()
