"""k_fixed_lds staging on the GPU: every workgroup lands its rows by LDS-DMA
and its mask pairs by raw 2-byte loads in one memory round trip, and each lane
reads back only what its own DMA landed, so these shapes sit where that can go
wrong -- around one, two and several workgroup spans, both workgroup sizes
(GPT = 4: 1024 groups for n <= 5, GPT = 2: 512 groups for n = 6..8), with and
without the vote masks -- bit for bit against the C oracle
(tests/oracle_c.fixed_eval).  Outputs are pre-filled with a sentinel and carry
a guard tail, so an element left unwritten or written past G shows.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from etcd_amd import _lib
from tests import oracle_c as oc

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX = (1 << 64) - 1
GUARD = 16
C_SENT = 0xA5A5A5A5A5A5A5A5
V_SENT = 0xEE
NS = [1, 3, 5, 6, 8]
MODES = ["commit_vote", "commit", "vote"]


def _span(n):
    return 256 * (4 if n <= 5 else 2)


def _sizes(n):
    s = _span(n)
    return [2, s - 2, s, s + 2, 2 * s - 2, 3 * s, 8 * s + 6]


def _values(seed, n, G):
    """Match rows mixing edge values (top bit set, MaxUint64, zero), ties
    (three small values) and the full u64 range; mask bytes over all 8 bits,
    so bits at and above n are set too."""
    rng = np.random.default_rng(seed)
    pool = np.array([0, 1, 2, MAX, MAX - 1, 1 << 63, (1 << 63) - 1, (1 << 63) + 5], np.uint64)
    kind = rng.integers(0, 3, size=G)
    edge = rng.choice(pool, size=(n, G))
    ties = rng.integers(0, 3, size=(n, G)).astype(np.uint64)
    wide = rng.integers(0, MAX, size=(n, G), dtype=np.uint64, endpoint=True)
    match = np.where(kind == 0, edge, np.where(kind == 1, ties, wide))
    match[:, 0] = 0
    match[:, G - 1] = MAX
    vd = rng.integers(0, 256, size=G).astype(np.uint8)
    gr = rng.integers(0, 256, size=G).astype(np.uint8)
    return np.ascontiguousarray(match), vd, gr


@functools.lru_cache(maxsize=None)
def _case(n, G, seed=0):
    """Inputs and the oracle's outputs for (n, G): computed once, read-only."""
    match, vd, gr = _values(1000 * n + G + seed, n, G)
    ec, ev = oc.fixed_eval(n, match, vd, gr)
    for a in (match, vd, gr, ec, ev):
        a.setflags(write=False)
    return match, vd, gr, ec, ev


def _dev(a, lead=0):
    """``a`` on the device, ``lead`` elements into its allocation."""
    buf = torch.zeros(lead + a.size, dtype={8: torch.int64, 1: torch.uint8}[a.itemsize], device=DEV)
    view = buf[lead:]
    flat = a.reshape(-1).view(np.int64 if a.itemsize == 8 else np.uint8).copy()  # (a is read-only)
    view.copy_(torch.from_numpy(flat))
    return view


def _outputs(G):
    c = torch.full((G + GUARD,), C_SENT - (1 << 64), dtype=torch.int64, device=DEV)
    v = torch.full((G + GUARD,), V_SENT, dtype=torch.uint8, device=DEV)
    return c, v


def _check_outputs(c, v, G, ec, ev, what):
    if c is not None:
        got = c.cpu().numpy().view(np.uint64)
        assert np.array_equal(got[:G], ec), f"{what}: commit"
        assert (got[G:] == np.uint64(C_SENT)).all(), f"{what}: commit written past G"
    if v is not None:
        got = v.cpu().numpy()
        assert np.array_equal(got[:G], ev), f"{what}: vote"
        assert (got[G:] == V_SENT).all(), f"{what}: vote written past G"


def _run(n, G, mode, lead=0):
    match, vd, gr, ec, ev = _case(n, G)
    dm, dvd, dgr = _dev(match, lead), _dev(vd), _dev(gr)
    c, v = _outputs(G)
    want_c, want_v = mode != "vote", mode != "commit"
    torch.cuda.synchronize()
    _lib.call("qb_dev_fixed_committed_vote", n, G, dm.data_ptr(), dvd.data_ptr(), dgr.data_ptr(),
              c.data_ptr() if want_c else None, v.data_ptr() if want_v else None,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    what = f"n={n} G={G} {mode} lead={lead}"
    _check_outputs(c, v, G, ec if want_c else np.full(G, C_SENT, np.uint64),
                   ev if want_v else np.full(G, V_SENT, np.uint8), what)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", NS)
def test_staging_shapes(n, mode):
    for G in _sizes(n):
        _run(n, G, mode)


@pytest.mark.parametrize("n", [5, 8])
def test_unaligned_match_takes_scalar_path(n):
    """match 8 bytes into its allocation: not 16-byte aligned, so the launch
    falls back from LDS-DMA to one group per thread and must still agree."""
    G = 3 * _span(n)
    _run(n, G, "commit_vote", lead=1)


@pytest.mark.parametrize("n", [5, 8])
def test_odd_group_count(n):
    G = 3 * _span(n) + 1
    for mode in MODES:
        _run(n, G, mode)


class _FixedBatch(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in ("match", "voted", "granted", "commit_out", "vote_out")]


def test_batches_entry_two_streams_then_one():
    """6 distinct batches of 8 spans through qb_dev_fixed_committed_vote_batches
    on 2 streams, then on 1 stream, back to back without a sync between the
    calls: the staging depends on nothing outside its own workgroup, so every
    batch of both calls must be complete and exact."""
    n, B = 5, 6
    G = 8 * _span(n)
    lib = _lib.load()
    cases = [_case(n, G, seed=7 * (b + 1)) for b in range(B)]
    ins = [(_dev(m), _dev(vd), _dev(gr)) for m, vd, gr, _, _ in cases]
    streams = [torch.cuda.Stream(DEV) for _ in range(2)]
    runs = []
    torch.cuda.synchronize()
    for ns in (2, 1):
        outs = [_outputs(G) for _ in range(B)]
        torch.cuda.synchronize()
        tab = (_FixedBatch * B)(*[_FixedBatch(m.data_ptr(), vd.data_ptr(), gr.data_ptr(),
                                              c.data_ptr(), v.data_ptr())
                                  for (m, vd, gr), (c, v) in zip(ins, outs)])
        sp = (C.c_void_p * ns)(*[s.cuda_stream for s in streams[:ns]])
        runs.append((ns, outs, tab, sp))
    for ns, outs, tab, sp in runs:
        _lib.check(lib.qb_dev_fixed_committed_vote_batches(n, G, B, tab, sp, ns), "batches")
    torch.cuda.synchronize()
    for ns, outs, _, _ in runs:
        for b, ((c, v), (_, _, _, ec, ev)) in enumerate(zip(outs, cases)):
            _check_outputs(c, v, G, ec, ev, f"streams={ns} batch={b}")
