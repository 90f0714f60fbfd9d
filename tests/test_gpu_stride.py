"""The step kernels' tile loops past their first trip, bit-exact against the
Python references at G = 524,779 groups.

k_tick, k_campaign, k_propose, k_requests and k_step<LOG> stride the tiles of
256 groups with a grid of at most 2048 workgroups (resident_blocks() <= 2048;
kStepBlocks = 2048), so a later trip of `for (tile = blockIdx.x; ...; tile +=
gridDim.x)` — the LDS Tile reused, stale owner bytes, BlockTally and k_step's
counters carried across tiles — runs only when G > 2048 * 256.  The shape
follows from those caps: G0 = 1031 groups (1031 mod 256 = 7: successive copies
sit on different lanes and straddle tile edges) times K = 509 copies is at
least 2048 * 256 + 257, so every workgroup of a 2048-block grid takes a second
trip and some a partial last tile; a smaller reported cap only adds trips.
The follower batches also give 6 groups of every copy a run above kInline =
16, so a striding k_step lists more than kLongBlocks = 256 long groups and
k_long strides too, and G > kScanPer = 4096 takes the scan's second level.

The batch is tests/replicate.py's: the reference runs once on the base of G0
groups, packed arrays and expected outputs are replicated with numpy and go up
through the mirrors' array constructors.  Two layouts per entry point: every
copy active, and every copy idle but the last three (the workgroups that reach
the tail take an idle trip, LDS never written, before an active one).
Everything the small tests compare is compared, with their pre-fills, over
all G, S and M: every in/out array, every output including elements that must
stay untouched, the accumulated stats.  All comparisons are integer
equality."""
import functools
import importlib

import numpy as np
import pytest
import torch

from etcd_amd.quorum import follower as qf, leader as ql, propose as qp, request as qr, tick as qt
from tests import append_pack as AP, campaign_pack as CP, follower_pack as FP
from tests import propose_pack as PP, propose_ref as PR, request_pack as QP, request_ref as QR
from tests import replicate as X, tick_pack as TP, tick_ref as TR

qc = importlib.import_module("etcd_amd.quorum.campaign")

pytestmark = pytest.mark.gpu
DEV = "cuda"
G0, K = 1031, 509
M0 = 3000
FILL = TP.FILL
FILL_I64 = FILL - (1 << 64)
LAYOUTS = {"all_active": (0,) * K, "tail_active": (1,) * (K - 3) + (0,) * 3}
layouts = pytest.mark.parametrize("layout", list(LAYOUTS))


def big(bases, layout) -> X.Case:
    case = X.replicate(list(bases), LAYOUTS[layout])
    assert case.G == G0 * K and case.G > 2048 * 256 + 256   # a second trip for every workgroup
    return case


def compare(where, got, want: X.Arrays):
    """Every array of ``want`` against the device's; a mismatch names the
    first elements, and for a per-group array their tile and trip."""
    assert got.keys() == want.keys(), (where, sorted(set(got) ^ set(want)))
    for k, (kind, w) in want.items():
        g, w = np.asarray(got[k]).reshape(-1), np.asarray(w).reshape(-1)
        assert g.dtype == w.dtype and g.shape == w.shape, (where, k, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = np.flatnonzero(g != w)
            tiles = (at[:8] // 256).tolist() if kind in (X.GROUP, X.STOP) else None
            raise AssertionError((where, k, kind, len(at), at[:8].tolist(), "tile", tiles, "trip",
                                  tiles and [t // 2048 for t in tiles], g[at[:8]].tolist(),
                                  w[at[:8]].tolist()))


def f8(n):
    return torch.full((max(n, 1),), 0xA5, dtype=torch.uint8, device=DEV)


def f64(n):
    return torch.full((max(n, 1),), FILL_I64, dtype=torch.int64, device=DEV)


def table(case, cap, readq_cap, read_only=ql.READ_ONLY_SAFE):
    a = {k: case.arr(k).reshape(-1) for k in ql.GROUP_ARRAYS}
    return ql.LeaderGroups(a, cap, readq_cap, read_only, device=DEV)


def election(case, lg, rand_timeout=None):
    e = {k[2:]: v for k, (_, v) in case.inp.items() if k.startswith("e.")}
    rt = np.zeros(case.G, np.uint32) if rand_timeout is None else rand_timeout
    state = qt.TickState.from_numpy(e["role"], e["election_elapsed"], e["heartbeat_elapsed"], rt,
                                    device=DEV)
    return qc.ElectionState.for_table(lg, state, e["self_id"], e["vote"], e["lead"], e["last_term"],
                                      10, True, True, votes=e["votes"])


def table_state(lg, es=None):
    got = dict(lg.numpy())
    if es is not None:
        got.update({"e." + k: v for k, v in es.numpy().items()})
    return got


# --------------------------------------------------------------------- tick ---

TICK = (1, 1, 1)    # sweep, step-down and beat on one tick
READQ = 4


@functools.lru_cache(None)
def tick_bases():
    nodes = TP.random_nodes(np.random.default_rng(41), G0, READQ, TICK[0], TICK[1])
    active = X.tick_case(nodes, READQ, *TICK)
    seen = int(np.bitwise_or.reduce(active.calls[0][0]["tflags"][1]))
    want = (TR.TFLAG_HUP | TR.TFLAG_BEAT | TR.TFLAG_CHECK_QUORUM | TR.TFLAG_STEPPED_DOWN |
            TR.TFLAG_TRANSFER_ABORTED)
    assert seen & want == want, hex(seen)
    idle = X.tick_case(X.tick_idle(nodes), READQ, *TICK)
    assert not any(c[0]["tflags"][1].any() for c in idle.calls)
    return active, idle


@layouts
def test_tick_two_ticks(layout):
    """(et, ht, cq) = (1, 1, 1), readq_cap 4, two consecutive ticks: the
    second acts on what the first left.  Rests on the 2048-block cap."""
    case = big(tick_bases(), layout)
    G = case.G
    lg = table(case, 1, READQ)
    state = qt.TickState.from_numpy(*[case.arr("t." + k) for k in (
        "role", "election_elapsed", "heartbeat_elapsed", "rand_timeout")], device=DEV)
    out = qt.TickResult(f8(G), f64(lg.S), f64(G), torch.zeros(8, dtype=torch.int64, device=DEV), lg)
    for k, (want, stats) in enumerate(case.calls):
        lg.tick(state, *TICK[:2], bool(TICK[2]), out=out)
        got = table_state(lg)
        got.update({"t." + n: v for n, v in state.numpy(G).items()})
        got.update(tflags=ql._to_np(out.tflags, np.uint8, G),
                   hb_commit=ql._to_np(out.hb_commit, np.uint64, lg.S),
                   hb_ctx=ql._to_np(out.hb_ctx, np.uint64, G))
        compare(f"tick {layout} #{k}", got, want)
        assert out.stats_dict() == stats, (layout, k, out.stats_dict(), stats)


# ----------------------------------------------------------------- campaign ---

@functools.lru_cache(None)
def campaign_bases(pre_vote):
    rng = np.random.default_rng(42 + pre_vote)
    nodes = CP.random_nodes(rng, G0, readq_cap=READQ)
    active = X.campaign_case(nodes, CP.random_actions(rng, G0), pre_vote, READQ)
    st = active.calls[0][1]
    assert all(st[k] > 0 for k in st if pre_vote or k != "pre_campaigns"), st
    idle = X.campaign_case(nodes, np.zeros(G0, np.uint8), pre_vote, READQ)
    assert not idle.calls[0][0]["cflags"][1].any()
    return active, idle


@layouts
@pytest.mark.parametrize("pre_vote", [0, 1])
def test_campaign(pre_vote, layout):
    """One call over the generator's ragged slot counts.  Rests on the
    2048-block cap."""
    case = big(campaign_bases(pre_vote), layout)
    G = case.G
    lg = table(case, CP.INFLIGHT_CAP, READQ)
    es = election(case, lg)
    es.follower.pre_vote = bool(pre_vote)
    out = qc.CampaignResult(f8(G), f8(G), f64(G),
                            torch.full((G,), 0xA5A5 - (1 << 16), dtype=torch.int16, device=DEV),
                            torch.zeros(len(qc.CSTAT_NAMES), dtype=torch.int64, device=DEV))
    want, stats = case.calls[0]
    lg.campaign(es, torch.from_numpy(case.arr("action").copy()).to(DEV), out=out)
    got = table_state(lg, es)
    got.update(cflags=ql._to_np(out.cflags, np.uint8, G), req_type=ql._to_np(out.req_type, np.uint8, G),
               req_term=ql._to_np(out.req_term, np.uint64, G),
               req_mask=ql._to_np(out.req_mask, np.uint16, G))
    compare(f"campaign pv{pre_vote} {layout}", got, want)
    assert out.stats_dict() == stats, (layout, out.stats_dict(), stats)


# ------------------------------------------------------------------ propose ---

PCFG = PR.Config(max_uncommitted_size=100)


@functools.lru_cache(None)
def propose_bases():
    rng = np.random.default_rng(43)
    nodes = PP.random_nodes(rng, G0)
    active = X.propose_case(nodes, PP.random_inputs(rng, G0), PCFG)
    st = active.calls[0][1]
    for k in ("proposals", "entries", "drop_size", "forwarded", "cc_accepted", "cc_refused",
              "msg_app", "leader_entries", "bad_action"):
        assert st[k] > 0, (k, st)
    idle = X.propose_case(nodes, PP.inputs(np.zeros(G0, np.uint8), np.zeros(G0, np.uint32)), PCFG)
    assert not idle.calls[0][0]["pflags"][1].any()
    return active, idle


@layouts
def test_propose(layout):
    """One call over the generator's ragged slot counts.  Rests on the
    2048-block cap."""
    case = big(propose_bases(), layout)
    G = case.G
    lg = table(case, PP.INFLIGHT_CAP, 0)
    es = election(case, lg)
    ps = qp.ProposeState.from_numpy(*[case.arr("p." + k) for k in (
        "applied", "uncommitted_size", "pending_conf_index")], device=DEV)
    ib = qp.ProposeInbox.from_numpy(*[case.arr("in." + k) for k in (
        "action", "n_ents", "payload", "cc_at", "cc_payload")], device=DEV)
    S = lg.S
    out = qp.ProposeResult(f8(G), f8(S), f64(S), f64(S), f64(S),
                           torch.zeros(len(qp.PSTAT_NAMES), dtype=torch.int64, device=DEV))
    want, stats = case.calls[0]
    qp.leader_propose(lg, es, ps, ib, max_uncommitted_size=PCFG.max_uncommitted_size,
                      disable_proposal_forwarding=PCFG.disable_proposal_forwarding, out=out)
    got = table_state(lg, es)
    got.update({"p." + k: v for k, v in ps.numpy(G).items()})
    got["pflags"] = ql._to_np(out.pflags, np.uint8, G)
    got["msg_type"] = ql._to_np(out.msg_type, np.uint8, S)
    for k in ("msg_index", "msg_log_term", "msg_n"):
        got[k] = ql._to_np(getattr(out, k), np.uint64, S)
    compare(f"propose {layout}", got, want)
    assert out.stats_dict() == stats, (layout, out.stats_dict(), stats)


# ----------------------------------------------------------------- requests ---

QCFG = QR.Config(read_only=QR.SAFE, readq_cap=READQ, max_reads=4)


@functools.lru_cache(None)
def requests_bases():
    rng = np.random.default_rng(44)
    nodes = QP.random_nodes(rng, G0, QCFG.readq_cap)
    active = X.requests_case(nodes, QP.random_inputs(rng, nodes, QCFG.max_reads), QCFG)
    st = active.calls[0][1]
    for k in ("bcast", "bcast_dup", "postponed", "rd_forward", "queue_full", "bad_count",
              "xf_started", "xf_timeout_now", "xf_msg_app", "xf_forward"):
        assert st[k] > 0, (k, st)
    idle = X.requests_case(nodes, X.requests_idle_inputs(G0, QCFG.max_reads), QCFG)
    assert not idle.calls[0][0]["qflags"][1].any()
    return active, idle


@layouts
def test_requests(layout):
    """One call over the generator's ragged slot counts, k-major request rows.
    Rests on the 2048-block cap."""
    case = big(requests_bases(), layout)
    G, R = case.G, QCFG.max_reads
    lg = table(case, QP.INFLIGHT_CAP, QCFG.readq_cap, QCFG.read_only)
    es = election(case, lg)
    inp = {k: case.arr("in." + k).reshape(-1) for k in X.REQ_IN_KINDS}
    ib = qr.RequestInbox.from_numpy(R, inp["n_reads"], inp["rd_ctx"], inp["rd_from"],
                                    inp["xf_from"], inp["xf_term"], device=DEV)
    S = lg.S
    out = qr.RequestResult(f8(G * R), f64(G * R), f64(S), f8(G), f64(G), f64(G), f64(G), f8(G),
                           torch.zeros(len(qr.QSTAT_NAMES), dtype=torch.int64, device=DEV))
    want, stats = case.calls[0]
    qr.leader_requests(lg, es, ib, out=out)
    got = table_state(lg, es)
    n = {"rd_status": G * R, "rd_index": G * R, "hb_commit": S}
    for k in QP.OUT_KEYS:
        got[k] = ql._to_np(getattr(out, k), want[k][1].dtype, n.get(k, G))
    compare(f"requests {layout}", got, want)
    for k, v in inp.items():   # the inputs are read only
        assert np.array_equal(ql._to_np(getattr(ib, k), v.dtype, len(v)), v), (layout, k)
    assert out.stats_dict() == stats, (layout, out.stats_dict(), stats)


# ----------------------------------------------------- follower, follower_log ---

FCFG = FP.fuzz_config(True, True)
HOT = 6     # groups of the base whose run passes kInline


def heat(recs, seed):
    """A twentieth of the records moved to HOT groups: runs of about 25,
    above kInline = 16, beside the short ones."""
    rng = np.random.default_rng(seed)
    hot = rng.choice(G0, HOT, replace=False)
    return [(int(hot[int(rng.integers(0, HOT))]) if g < G0 and rng.random() < 0.05 else g, r)
            for g, r in recs]


def check_runs(case):
    """Most runs short, HOT of them above kInline."""
    g = case.arr("r.group")
    n = np.bincount(g[g < G0], minlength=G0)
    assert (n > 16).sum() == HOT and (n == 0).sum() > 20 and np.median(n) <= 4
    assert case.calls[0][1]["after_stop"] > 0


@functools.lru_cache(None)
def follower_bases():
    nodes, recs = FP.fuzz(45, G=G0, M=M0)
    active = X.follower_case(nodes, heat(recs, 45), FCFG)
    check_runs(active)
    return active, X.follower_case(nodes, [], FCFG)


@functools.lru_cache(None)
def follower_log_bases():
    nodes, recs = AP.fuzz(46, G=G0, M=M0)
    active = X.follower_log_case(nodes, heat(recs, 46), FCFG)
    check_runs(active)
    st = active.calls[0][1]
    assert st["app_accepted"] > 200 and st["app_rejected"] > 50 and st["app_truncated"] > 10
    return active, X.follower_log_case(nodes, [], FCFG)


def follower_upload(case):
    a = {k: case.arr(k) for k in FP.GROUP_DTYPES}
    state = qt.TickState.from_numpy(a["role"], a["election_elapsed"], a["heartbeat_elapsed"],
                                    np.zeros(case.G, np.uint32), device=DEV)
    fg = qf.FollowerGroups.from_numpy(a, state, FCFG.election_timeout, FCFG.check_quorum,
                                      FCFG.pre_vote, device=DEV)
    ib = qf.FollowerInbox.from_numpy(*[case.arr("r." + k) for k in (
        "group", "flags", "from", "term", "index", "aux")], device=DEV)
    return a, fg, ib


def follower_outputs(res, G, M, cols):
    got = {k: ql._to_np(getattr(res, k), dt, M) for k, dt in cols}
    got["stop_at"] = ql._to_np(res.stop_at, np.uint32, G)
    got["gflags"] = ql._to_np(res.gflags, np.uint8, G)
    return got


@layouts
def test_follower_step(layout):
    """M0 = 3000 records on the base (1.5M in all when every copy is active),
    the copies interleaved.  Rests on kStepBlocks = 2048, and with kInline =
    16 on kLongBlocks = 256 (3054 / 18 long groups) and kScanPer = 4096."""
    case = big(follower_bases(), layout)
    G, M = case.G, case.M
    _, fg, ib = follower_upload(case)
    need = qf.follower_workspace_bytes(G, M)
    out = qf.FollowerResult(f8(M), torch.full((max(M, 1),), -1, dtype=torch.int64, device=DEV),
                            torch.full((G,), 0x5A5A5A5A, dtype=torch.int32, device=DEV), f8(G),
                            torch.zeros(len(qf.FSTAT_NAMES), dtype=torch.int64, device=DEV),
                            torch.full(((need + 7) // 8,), -1, dtype=torch.int64, device=DEV))
    res = qf.follower_step(fg, ib, out=out)
    want, stats = case.calls[0]
    got = dict(fg.numpy())
    got.update(follower_outputs(res, G, M, (("resp_type", np.uint8), ("resp_term", np.uint64))))
    compare(f"follower {layout}", got, want)
    assert res.stats_dict() == stats, (layout, res.stats_dict(), stats)


LOG_COLS = (("resp_type", np.uint8), ("resp_term", np.uint64), ("resp_index", np.uint64),
            ("resp_hint", np.uint64), ("resp_log_term", np.uint64), ("app_from", np.uint64))


@layouts
def test_follower_log_step(layout):
    """The same shape with MsgApp records: the run table (run-major) and the
    entry runs follow their copies.  Rests on the same constants."""
    case = big(follower_log_bases(), layout)
    G, M = case.G, case.M
    a, fg, ib = follower_upload(case)
    lg = qf.FollowerLog.from_numpy(case.arr("l.meta"), case.arr("l.first_index"),
                                   case.arr("l.run_start"), case.arr("l.run_term"), a, device=DEV)
    app = qf.FollowerAppInbox.from_numpy(*[case.arr(k) for k in (
        "commit", "ent_off", "ent_term", "ent_len")], device=DEV)
    need = qf.follower_log_workspace_bytes(G, M)
    out = qf.FollowerLogResult(f8(M), f64(M),
                               torch.full((G,), 0x5A5A5A5A, dtype=torch.int32, device=DEV), f8(G),
                               torch.zeros(len(qf.FLSTAT_NAMES), dtype=torch.int64, device=DEV),
                               torch.full(((need + 7) // 8,), -1, dtype=torch.int64, device=DEV),
                               None, f64(M), f64(M), f64(M), f64(M))
    res = qf.follower_log_step(fg, lg, ib, app, out=out)
    want, stats = case.calls[0]
    got = dict(fg.numpy())
    got.update({"l." + k: v for k, v in lg.numpy().items()})
    got.update(follower_outputs(res, G, M, LOG_COLS))
    compare(f"follower_log {layout}", got, want)
    assert res.stats_dict() == stats, (layout, res.stats_dict(), stats)
