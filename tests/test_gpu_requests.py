"""qb_dev_leader_requests on the device against tests/request_ref.py, bit-exact
after every call: every array of the table (the read queue with its rows past
the count, which hold a marker) and of the election state, so nothing a
request does not own can have moved; rd_status / rd_index / hb_commit / xf_* /
qflags including the elements a call must leave untouched (pre-filled with
0xA5...), and the accumulated stats.  All comparisons are integer equality."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from etcd_amd import _lib
from etcd_amd.quorum import leader as ql, request as qr, tick as qt
from oracle import leader_ref as L
from tests import propose_pack as P, request_pack as Q, request_ref as R

qc = importlib.import_module("etcd_amd.quorum.campaign")

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL_I64 = Q.FILL - (1 << 64)
U64 = (1 << 64) - 1
NO = R.NO_SLOT


class DeviceRun:
    """A batch of RequestNodes on the device beside its reference copy."""

    def __init__(self, nodes, cfg=None, cap=Q.INFLIGHT_CAP):
        self.nodes, self.cfg, self.cap = nodes, cfg or R.Config(), cap
        a, e = Q.pack_nodes(nodes, self.cfg.readq_cap, cap)
        self.lg = ql.LeaderGroups(self.layout(a), cap, self.cfg.readq_cap, self.cfg.read_only,
                                  device=DEV)
        G, S, M = self.lg.G, self.lg.S, self.cfg.max_reads
        self.off = self.lg.numpy()["off"]
        self.state = qt.TickState.from_numpy(e["role"], e["election_elapsed"],
                                             e["heartbeat_elapsed"], np.zeros(G, np.uint32),
                                             device=DEV)
        self.es = qc.ElectionState.for_table(self.lg, self.state, e["self_id"], e["vote"],
                                             e["lead"], e["last_term"], 10, True, True,
                                             votes=e["votes"])
        n, s, r = max(G, 1), max(S, 1), max(G * M, 1)
        f8 = lambda k: torch.full((k,), 0xA5, dtype=torch.uint8, device=DEV)  # noqa: E731
        f64 = lambda k: torch.full((k,), FILL_I64, dtype=torch.int64, device=DEV)  # noqa: E731
        self.out = qr.RequestResult(f8(r), f64(r), f64(s), f8(n), f64(n), f64(n), f64(n), f8(n),
                                    torch.zeros(len(qr.QSTAT_NAMES), dtype=torch.int64, device=DEV))
        self.want = Q.new_out(G, S, M)
        self.stats = R.new_stats()

    def layout(self, a):
        """The table as the device holds it (the dense one here)."""
        return a

    def check_state(self, where):
        a, e = Q.pack_nodes(self.nodes, self.cfg.readq_cap, self.cap)
        want = self.layout(a)
        got = self.lg.numpy()
        for key in got:
            assert np.array_equal(got[key], want[key]), (where, key,
                                                         np.flatnonzero(got[key] != want[key])[:8])
        ge = self.es.numpy()
        e.update(term=a["term"], committed=a["committed"], last_index=a["last_index"])
        for key, w in e.items():
            assert np.array_equal(ge[key], w), (where, key, np.flatnonzero(ge[key] != w)[:8])
        assert ge.keys() == e.keys()

    def call(self, inp, where, xf_term_null=False):
        G, S, M = self.lg.G, self.lg.S, self.cfg.max_reads
        ib = qr.RequestInbox.from_numpy(M, inp["n_reads"], inp["rd_ctx"], inp["rd_from"],
                                        inp["xf_from"], None if xf_term_null else inp["xf_term"],
                                        device=DEV)
        res = qr.leader_requests(self.lg, self.es, ib, out=self.out)
        assert res is self.out
        st, results = Q.ref_requests(self.nodes, inp, self.cfg, self.off, self.want)
        for k, v in st.items():
            self.stats[k] += v
        self.check_state(where)
        n = {"rd_status": G * M, "rd_index": G * M, "hb_commit": S}
        for key in Q.OUT_KEYS:
            w = self.want[key]
            got = ql._to_np(getattr(res, key), w.dtype, n.get(key, G))
            assert np.array_equal(got, w), (where, key, np.flatnonzero(got != w)[:8],
                                            got[got != w][:8], w[got != w][:8])
        for key, v in inp.items():   # the inputs are read only
            t = getattr(ib, key)
            if t is not None:
                assert np.array_equal(ql._to_np(t, v.dtype, len(v)), v), (where, key)
        assert res.stats_dict() == self.stats, (where, res.stats_dict(), self.stats)
        self.results = results
        return results

    def views_match(self, g):
        """The result object's per-group views against the restatement's."""
        res, r = self.out, self.results[g]
        assert [(s, i) for s, _, _, i in res.reads(g)] == r.reads, (g, res.reads(g), r.reads)
        assert res.heartbeats(g) == [h for h in (r.heartbeats or []) if h[0] < 16], g
        t, idx, lt, k = r.xf
        got = res.transfer(g)
        if not t:
            assert got is None, (g, got)
        else:
            assert (got[0], got[2], got[3], got[5]) == (t, idx, lt, k), (g, got, r.xf)
            assert got[1] == int(self.out.inbox.xf_from[g].item())


# --------------------------------------------------------- golden scenarios ---

SCENARIOS = Q.load_tables()["scenarios"]


@pytest.mark.parametrize("sc", SCENARIOS, ids=[s["name"] for s in SCENARIOS])
def test_golden_scenarios_on_device(sc):
    """The reference's tests, G = 1 each, through the device: the transcribed
    expectations hold for the device's outputs (equal to request_ref's after
    every call, which is what check_expect then reads)."""
    cap = sc["node"]["inflight_cap"]

    def apply(n, cfg, reads, xf_from, xf_term):
        run = DeviceRun([n], cfg, cap)    # (the scenario may have set node fields between steps)
        res = run.call(Q.inputs(1, cfg.max_reads, [reads], [xf_from], [xf_term]), sc["name"])
        run.views_match(0)
        return res[0]
    Q.replay(sc, apply)


# --------------------------------------------------------------------- fuzz ---

FUZZ = {"G1": (1, None, R.SAFE, 4, 16), "G257": (257, None, R.SAFE, 4, 16),
        "G1000-lease": (1000, None, R.LEASE, 0, 1), "G513-n16": (513, (16,), R.SAFE, 4, 3)}


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("name", list(FUZZ))
def test_fuzz_two_calls(name, seed):
    """Seeded batches (request_pack.random_nodes) through two calls into the
    same outputs: the second acts on what the first left (queued contexts,
    set transferees), and the stats accumulate."""
    G, slots, ro, qcap, maxr = FUZZ[name]
    rng = np.random.default_rng(100 * seed + G)
    cfg = R.Config(read_only=ro, readq_cap=qcap, max_reads=maxr)
    run = DeviceRun(Q.random_nodes(rng, G, qcap, slots), cfg)
    for k in range(2):
        run.call(Q.random_inputs(rng, run.nodes, maxr), f"{name} seed {seed} call {k}",
                 xf_term_null=False)
        for g in (0, G // 2, G - 1):
            run.views_match(g)
    if name == "G257":   # the main branches were reached
        for k in ("bcast", "bcast_dup", "postponed", "rd_forward", "rd_ignored", "queue_full",
                  "rd_host", "bad_ctx", "bad_count", "xf_started", "xf_timeout_now", "xf_msg_app",
                  "xf_ign_term", "xf_ign_no_progress", "xf_host", "xf_forward"):
            assert run.stats[k] > 0, (k, run.stats)
    if name == "G1000-lease":
        assert run.stats["read_states"] and run.stats["read_resps"] and not run.stats["bcast"]


def test_idle_tile_next_to_a_one_actor_tile():
    """Three tiles: seeded requests, nothing at all, and exactly one group
    that reads among 255 idle ones; then a call with nothing to do."""
    rng = np.random.default_rng(31)
    cfg = R.Config(readq_cap=4, max_reads=2)
    nodes = Q.random_nodes(rng, 768, 4)
    nodes[600] = Q.make_node(3, 0b111, 0, 1, terms=[2, 2, 2], term=2, committed=2)
    inp = Q.random_inputs(rng, nodes, 2)
    inp["n_reads"][256:] = 0
    inp["xf_from"][256:] = NO
    inp["n_reads"][600], inp["rd_ctx"][600], inp["rd_from"][600] = 1, 77, NO
    run = DeviceRun(nodes, cfg)
    res = run.call(inp, "skip paths")
    assert all(r.qflags == 0 for i, r in enumerate(res) if i >= 256 and i != 600)
    assert res[600].reads == [(R.RD_BCAST, None)] and res[600].heartbeats == [(0, 0), (2, 0)]
    inp["n_reads"][:] = 0
    inp["xf_from"][:] = NO
    assert all(r.qflags == 0 for r in run.call(inp, "all idle"))


# ---------------------------------------------------------------- wide span ---

class GappedRun(DeviceRun):
    """The same batch in a table whose groups sit `stride` slots apart: the
    slots between a group's end and the next group's start belong to nobody
    and must keep their bytes."""
    FILLS = (("match", 7), ("next", 8), ("pending_snapshot", 9), ("pstate", 0x0D), ("infl_pos", 1),
             ("infl_buf", 5))

    def __init__(self, nodes, stride, **kw):
        self.stride = stride
        super().__init__(nodes, **kw)

    def layout(self, a):
        G = len(a["cfg"])
        dense = a["off"].astype(np.int64)
        goff = np.arange(G + 1, dtype=np.uint32) * self.stride
        b = dict(a)
        b["off"] = goff
        for key, fill in self.FILLS:
            w = self.cap if key == "infl_buf" else 1
            out = np.full(int(goff[-1]) * w, fill, dtype=a[key].dtype)
            for i in range(G):
                n = int(dense[i + 1] - dense[i]) * w
                out[int(goff[i]) * w:int(goff[i]) * w + n] = a[key][dense[i] * w:dense[i + 1] * w]
            b[key] = out
        return b


def test_gapped_table_takes_the_unstaged_path_and_writes_at_most_16_slots():
    """300 groups of 16 slots, 20 slots apart: a workgroup's span is 5120
    slots, wider than its LDS stage, so the heartbeats are written from each
    group's own thread.  Every group declares 20 slots, read as 16; the four
    slots past each group keep their sentinels, in the table and in
    hb_commit."""
    rng = np.random.default_rng(20)
    cfg = R.Config(readq_cap=4, max_reads=2)
    run = GappedRun(Q.random_nodes(rng, 300, 4, (16,)), 20, cfg=cfg)
    run.call(Q.random_inputs(rng, run.nodes, 2, p_none=0.1), "gapped")
    assert run.stats["bcast_groups"] > 20 and run.stats["xf_msg_app"]
    run.call(Q.random_inputs(rng, run.nodes, 2, p_none=0.1), "gapped, second call")


# -------------------------------------------------------------------- edges ---

REPL, PROBE, SNAP = L.STATE_REPLICATE, L.STATE_PROBE, L.STATE_SNAPSHOT
QCAP = 4


def edge_cases(cap=Q.INFLIGHT_CAP):
    """(name, node, reads, xf_from, xf_term, want) under ReadOnlySafe,
    readq_cap 4, max_reads 16.  want: dict of st (statuses), xt (xf_type),
    qf (qflags), each optional."""
    mk, pr = Q.make_node, P.progress
    t5 = [1, 1, 2, 2, 3, 3]                    # indexes 0..5, last = 5
    out = []

    def add(name, node, reads=(), xf=NO, xterm=0, **want):
        out.append((name, node, list(reads), xf, xterm, want))

    def three(own_match, peers):
        """Progress of a 3-slot group whose own slot is 1."""
        return [peers[0], pr(own_match, own_match + 1, REPL, True, cap=cap), peers[1]]

    def leader(prs=None, **kw):
        """Three voters, own slot 1, everything committed at term 3."""
        kw.setdefault("terms", t5)
        kw.setdefault("term", 3)
        kw.setdefault("committed", kw.get("first", 1) - 1 + len(kw["terms"]) - 1)
        return mk(3, 0b111, 0, 1, prs=prs, cap=cap, **kw)

    def rows(k):
        return [(100 + i, 4, {1}, NO) for i in range(k)]
    HB = R.QFLAG_HEARTBEATS
    # the queue's fill
    add("queue empty", leader(), [(9, NO)], st=[R.RD_BCAST], qf=HB)
    add("queue at cap - 1", leader(readq=rows(3)), [(9, 0)], st=[R.RD_BCAST], qf=HB)
    add("queue full, a new context", leader(readq=rows(4)), [(9, 0)], st=[R.RD_QUEUE_FULL], qf=0)
    add("a duplicate of a pending context", leader(readq=[(100, 4, set(), 2)]), [(100, 0)],
        st=[R.RD_BCAST_DUP], qf=HB)
    add("a duplicate of a context queued earlier in the call", leader(), [(9, NO), (9, 2)],
        st=[R.RD_BCAST, R.RD_BCAST_DUP], qf=HB)
    add("a duplicate behind a full queue", leader(readq=rows(4)), [(200, NO), (103, 0)],
        st=[R.RD_QUEUE_FULL, R.RD_BCAST_DUP], qf=HB)
    add("sixteen reads fill the queue and overflow it", leader(),
        [(50 + (k % 6), NO if k % 2 else 2) for k in range(16)], qf=HB)
    add("n_reads past max_reads", leader(), [(60 + k, NO) for k in range(17)], qf=HB | R.QFLAG_BAD)
    add("a context of 0", leader(), [(0, NO), (9, NO)], st=[R.RD_BAD, R.RD_BCAST],
        qf=HB | R.QFLAG_BAD)
    add("rd_from names no slot", leader(), [(9, 3), (9, 16), (9, 0xFE)], st=[R.RD_HOST] * 3,
        qf=R.QFLAG_HOST)
    add("the largest context", leader(), [(U64, 0)], st=[R.RD_BCAST], qf=HB)
    # committedEntryInCurrentTerm over 8 runs: indexes 0..10, the last run starts at 8
    t8 = [1, 1, 2, 3, 4, 5, 6, 7, 8, 8, 8]
    for name, com, ok in (("at first_index - 1", 0, False), ("inside an older run", 1, False),
                          ("one before the last run's start", 7, False),
                          ("at the last run's start", 8, True), ("inside the last run", 9, True),
                          ("at last_index", 10, True), ("past last_index", 11, False)):
        add(f"8 runs, committed {name}", leader(terms=t8, term=8, committed=com), [(9, NO)],
            st=[R.RD_BCAST if ok else R.RD_POSTPONED], qf=HB if ok else R.QFLAG_POSTPONED)
    add("compacted log of the leader's term, committed at first_index - 1",
        leader(terms=[3, 3], first=10, committed=9), [(9, NO)], st=[R.RD_BCAST])
    add("committed below first_index - 1", leader(terms=[3, 3], first=10, committed=8), [(9, NO)],
        st=[R.RD_POSTPONED])
    add("postponed already, postponed again", leader(term=4, pending=True), [(9, NO), (10, 2)],
        st=[R.RD_POSTPONED] * 2, qf=R.QFLAG_POSTPONED)
    # the singleton, and what is none
    add("singleton: the own slot is the sole voter", mk(3, 0b010, 0, 1, terms=t5, term=3, cap=cap,
                                                        committed=4),
        [(9, NO), (10, 1), (11, 0)], st=[R.RD_READ_STATE, R.RD_READ_STATE, R.RD_RESP], qf=0)
    add("singleton: the leader is not the sole voter, nothing of its term committed",
        mk(3, 0b001, 0, 1, terms=t5, term=4, cap=cap, committed=4), [(9, 2)], st=[R.RD_RESP], qf=0)
    add("one incoming voter and an outgoing half is no singleton",
        mk(3, 0b010, 0b010, 1, terms=t5, term=3, cap=cap, committed=5), [(9, NO)], st=[R.RD_BCAST])
    add("a joint config", mk(4, 0b0011, 0b0110, 1, terms=t5, term=3, cap=cap, committed=5),
        [(9, 3)], st=[R.RD_BCAST], qf=HB)
    add("a learner reads", mk(4, 0b0111, 0, 1, terms=t5, term=3, cap=cap, committed=5), [(9, 3)],
        st=[R.RD_BCAST], qf=HB)
    add("the own slot past the slots: no ack bit, every slot a heartbeat",
        mk(3, 0b111, 0, 0xFF, terms=t5, term=3, cap=cap, committed=5), [(9, NO)], st=[R.RD_BCAST])
    add("the own slot 15 of 16", mk(16, 0xFFFF, 0, 15, terms=t5, term=3, cap=cap, committed=5),
        [(9, 14)], st=[R.RD_BCAST], qf=HB)
    for ns in range(1, 17):
        add(f"{ns} slots, own slot last", mk(ns, (1 << ns) - 1, 0, ns - 1, terms=t5, term=3, cap=cap,
                                             committed=5), [(9, NO)],
            st=[R.RD_READ_STATE if ns == 1 else R.RD_BCAST])
    # roles
    for role in (R.FOLLOWER, R.CANDIDATE, R.LEADER, R.PRE_CANDIDATE):
        for lead in (0, 7):
            for xterm in (0, 2, 3, 4):
                add(f"role {role} lead {lead} transfer term {xterm}", leader(role=role, lead=lead),
                    [(9, NO), (0, 9)], 2, xterm)
    # transfers: the outcomes
    lag = lambda **kw: three(5, [pr(5, 6, REPL, True, cap=cap), pr(2, 3, PROBE, True, cap=cap, **kw)])  # noqa: E731
    ST = R.QFLAG_TRANSFER_STARTED
    add("transfer to a caught-up peer", leader(lag(), ee=7), xf=0, xt=R.MSG_TIMEOUT_NOW, qf=ST)
    add("transfer to a lagging probe", leader(lag(), ee=7), xf=2, xt=R.MSG_APP, qf=ST)
    add("transfer to a paused probe", leader(lag(probe_sent=True)), xf=2, xt=0, qf=ST)
    add("transfer to a learner", mk(4, 0b0111, 0, 1, terms=t5, term=3, cap=cap), xf=3, xt=0, qf=0)
    add("transfer to an outgoing voter", mk(4, 0b0011, 0b1000, 1, terms=t5, term=3, cap=cap), xf=3,
        xt=R.MSG_APP, qf=ST)
    for s in (3, 16, 0xFE):
        add(f"transfer to slot {s} of 3", leader(), xf=s, xt=0, qf=0)
    add("transfer to self", leader(), xf=1, xt=0, qf=0)
    add("transfer to the pending transferee", leader(lag(), transferee=2, ee=5), xf=2, xt=0, qf=0)
    add("transfer to another than the pending one", leader(lag(), transferee=2, ee=5), xf=0,
        xt=R.MSG_TIMEOUT_NOW, qf=ST | R.QFLAG_TRANSFER_ABORTED)
    add("abort, then self", leader(lag(), transferee=2, ee=5), xf=1, xt=0,
        qf=R.QFLAG_TRANSFER_ABORTED)
    add("a read and a transfer", leader(lag()), [(9, NO)], 2, 3, st=[R.RD_BCAST], xt=R.MSG_APP,
        qf=HB | ST)
    # sendAppend's branches
    full = tuple(range(6, 6 + cap))
    add("sendAppend: ring full", leader(three(5, [pr(3, 6 + cap, REPL, True, ring=full, cap=cap),
                                                  pr(5, 6, REPL, True, cap=cap)])), xf=0, xt=0, qf=ST)
    add("sendAppend: ring start at cap - 1, the add wraps",
        leader(three(5, [pr(3, 5, REPL, True, ring=(4,) if cap > 1 else (), start=cap - 1, cap=cap),
                         pr(5, 6, REPL, True, cap=cap)])), xf=0, xt=R.MSG_APP, qf=ST)
    add("sendAppend: replicate with nothing to send", leader(three(5, [pr(3, 6, REPL, True, cap=cap),
                                                                      pr(5, 6, REPL, True, cap=cap)])),
        xf=0, xt=R.MSG_APP, qf=ST)
    add("sendAppend: snapshot state is paused",
        leader(three(5, [pr(3, 4, SNAP, True, 0, 5, cap=cap), pr(5, 6, REPL, True, cap=cap)])),
        xf=0, xt=0, qf=ST)
    add("sendAppend: max_ents 1", leader(lag(), max_ents=1), xf=2, xt=R.MSG_APP, qf=ST)
    add("sendAppend: next - 1 inside an older run",
        leader(three(10, [pr(10, 11, REPL, True, cap=cap), pr(2, 4, REPL, True, cap=cap)]),
               terms=t8, term=8), xf=2, xt=R.MSG_APP, qf=ST)
    cterms = [2, 2, 3]                          # indexes 3..5
    for name, active, snap, xt in (("a snapshot", True, None, R.MSG_SNAP),
                                   ("RecentActive off", False, None, 0), ("snap_index 0", True, 0, 0)):
        for state in (PROBE, REPL):
            add(f"sendAppend: next < first_index, {name}, state {state}",
                leader(three(5, [pr(1, 2, state, active, cap=cap), pr(5, 6, REPL, True, cap=cap)]),
                       terms=cterms, first=4, snap_index=snap, snap_term=2, committed=3),
                xf=0, xt=xt, qf=ST)
    # the arithmetic's edges
    add("indexes and terms at 2^64 - 1: a read",    # the log is [2^64 - 6, 2^64 - 2]
        leader(three(U64 - 1, [pr(U64 - 3, U64 - 2, REPL, True, cap=cap),
                               pr(U64 - 1, U64, REPL, True, cap=cap)]),
               terms=[U64] * 5, term=U64, first=U64 - 4, committed=U64 - 1), [(U64, 0)], 0, U64,
        st=[R.RD_BCAST], xt=R.MSG_APP, qf=HB | ST)
    add("a transfer term above 2^63", leader(term=1 << 63, terms=[1, 1 << 63]), xf=0,
        xterm=(1 << 63) - 1, xt=0, qf=0)
    return out


def run_edges(cases, cfg, cap=Q.INFLIGHT_CAP, check_want=True):
    nodes = [copy.deepcopy(c[1]) for c in cases]
    for n in nodes:    # (a case's queue, cut to what this configuration holds)
        n.queue = n.queue[:cfg.readq_cap]
        n.pending = {c: n.pending[c] for c in n.queue}
    G = len(cases)
    run = DeviceRun(nodes, cfg, cap)
    inp = Q.inputs(G, cfg.max_reads, [c[2] for c in cases], [c[3] for c in cases],
                   [c[4] for c in cases])
    res = run.call(inp, "edges")
    for i, (name, _, _, _, _, want) in enumerate(cases):
        run.views_match(i)
        if not check_want:
            continue
        if "st" in want:
            assert [s for s, _ in res[i].reads] == want["st"], (name, res[i].reads)
        if "xt" in want:
            assert res[i].xf[0] == want["xt"], (name, res[i].xf)
        if "qf" in want:
            assert res[i].qflags == want["qf"], (name, hex(res[i].qflags))
    return run, res, {c[0]: i for i, c in enumerate(cases)}, inp


def test_edges():
    cases = edge_cases()
    run, res, by, inp = run_edges(cases, R.Config(R.SAFE, QCAP, 16))
    n = run.nodes
    g = n[by["a duplicate of a pending context"]].group
    assert [(r.ctx, r.acks, r.from_slot) for r in g.readq] == [(100, {1}, 2)]
    g = n[by["sixteen reads fill the queue and overflow it"]].group
    assert [r.ctx for r in g.readq] == [50, 51, 52, 53]
    assert [s for s, _ in res[by["sixteen reads fill the queue and overflow it"]].reads].count(
        R.RD_QUEUE_FULL) == 4
    assert len(res[by["n_reads past max_reads"]].reads) == 16
    g = n[by["the own slot past the slots: no ack bit, every slot a heartbeat"]].group
    assert g.readq[0].acks == set()
    assert len(res[by["the own slot past the slots: no ack bit, every slot a heartbeat"]].heartbeats) == 3
    assert n[by["the own slot 15 of 16"]].group.readq[0].acks == {15}
    i = by["transfer to a caught-up peer"]
    assert n[i].camp.election_elapsed == 0 and n[i].group.transferee == 0
    i = by["transfer to a lagging probe"]
    assert res[i].xf == (R.MSG_APP, 2, 2, 3) and n[i].group.prs[2].probe_sent
    i = by["abort, then self"]
    assert n[i].group.transferee == NO and n[i].camp.election_elapsed == 5
    i = by["sendAppend: ring start at cap - 1, the add wraps"]
    assert n[i].group.prs[0].inflights.fifo() == [4, 5] and n[i].group.prs[0].next == 6
    assert res[by["sendAppend: next - 1 inside an older run"]].xf == (R.MSG_APP, 3, 3, 7)
    assert res[by["sendAppend: max_ents 1"]].xf == (R.MSG_APP, 2, 2, 1)
    i = by["sendAppend: next < first_index, a snapshot, state 1"]
    assert res[i].xf == (R.MSG_SNAP, 3, 2, 0) and n[i].group.prs[0].state == SNAP
    i = by["indexes and terms at 2^64 - 1: a read"]
    assert res[i].xf == (R.MSG_APP, U64 - 3, U64, 2) and n[i].group.readq[0].index == U64 - 1
    for k in R.QSTAT_NAMES:
        assert run.stats[k] > 0, k
    # a second call on what the first left: every context is pending now or
    # the queue is full, the transferees are set
    run.call(inp, "edges: the same requests again")
    assert run.stats["xf_ign_same"] > 5


def test_edges_lease_without_a_queue_and_one_read_per_call():
    """ReadOnlyLeaseBased with readq_cap 0 (no queue arrays to speak of) and
    max_reads 1: every second read of a case is cut and counted."""
    cases = edge_cases()
    run, res, by, _ = run_edges(cases, R.Config(R.LEASE, 0, 1), check_want=False)
    assert res[by["queue empty"]].reads == [(R.RD_READ_STATE, 5)]
    assert res[by["a learner reads"]].reads == [(R.RD_RESP, 5)]
    assert res[by["8 runs, committed at first_index - 1"]].reads == [(R.RD_POSTPONED, None)]
    assert run.stats["bcast"] == 0 and run.stats["bcast_groups"] == 0 and run.stats["bad_count"] > 3


def test_safe_without_a_queue_hands_every_read_back():
    cases = [c for c in edge_cases() if c[0].startswith(("queue", "a dup", "8 runs"))]
    run, res, by, _ = run_edges(cases, R.Config(R.SAFE, 0, 2), check_want=False)
    assert res[by["queue empty"]].reads == [(R.RD_QUEUE_FULL, None)]
    assert run.stats["queue_full"] > 5 and run.stats["bcast_groups"] == 0


@pytest.mark.parametrize("cap", [1, 3])
def test_inflight_cap(cap):
    cases = [c for c in edge_cases(cap) if c[0].startswith(("sendAppend", "transfer"))]
    run_edges(cases, R.Config(R.SAFE, QCAP, 1), cap, check_want=False)


def test_xf_term_null_reads_every_transfer_as_local():
    cases = [c for c in edge_cases() if c[0].startswith(("role", "transfer"))]
    nodes = [copy.deepcopy(c[1]) for c in cases]
    G = len(cases)
    run = DeviceRun(nodes, R.Config(R.SAFE, QCAP, 2))
    inp = Q.inputs(G, 2, [c[2] for c in cases], [c[3] for c in cases], None)
    run.call(inp, "xf_term NULL", xf_term_null=True)
    assert run.stats["xf_ign_term"] == 0 and run.stats["xf_host"] == 0


# ------------------------------------------------------------------ raw ABI ---

def test_requests_raw_abi():
    """One call through plain ctypes with the library's own stream, memory and
    copies (no torch), as a cgo embedder makes it."""
    from tests.test_gpu_abi_raw import Stream
    rng = np.random.default_rng(78)
    G, M = 600, 3
    cfg = R.Config(R.SAFE, QCAP, M)
    nodes = Q.random_nodes(rng, G, QCAP)
    inp = Q.random_inputs(rng, nodes, M)
    a, e = Q.pack_nodes(nodes, QCAP)
    S = int(a["off"][-1])
    s = Stream()
    keys_a = ("off", "cfg", "meta", "term", "committed", "first_index", "last_index", "snap_index",
              "snap_term", "max_ents", "run_start", "run_term", "match", "next", "pending_snapshot",
              "pstate", "infl_pos", "infl_buf", "rq_ctx", "rq_index", "rq_meta")
    keys_e = ("role", "lead", "last_term", "election_elapsed")
    d = {k: s.up(a[k]) for k in keys_a}
    d.update({k: s.up(e[k]) for k in keys_e})
    rg = qr.RequestGroupsC(G=G, inflight_cap=Q.INFLIGHT_CAP, readq_cap=QCAP, read_only=R.SAFE,
                           max_reads=M, **d)
    d_in = {k: s.up(v) for k, v in inp.items()}
    want = Q.new_out(G, S, M)
    d_out = {k: s.zeros(v.nbytes, 0xA5) for k, v in want.items()}
    d_st = s.zeros(8 * len(qr.QSTAT_NAMES))
    rin, rout = qr.RequestInC(**d_in), qr.RequestOutC(**d_out)
    _lib.check(s.lib.qb_dev_leader_requests(C.byref(rg), C.byref(rin), C.byref(rout), d_st, s.st),
               "requests")
    st, _ = Q.ref_requests(nodes, inp, cfg, a["off"], want)
    want_a, want_e = Q.pack_nodes(nodes, QCAP)
    for k, v in want.items():
        assert np.array_equal(s.down(d_out[k], v), v), k
    for k, v in inp.items():
        assert np.array_equal(s.down(d_in[k], v), v), k
    for k in keys_a:
        assert np.array_equal(s.down(d[k], want_a[k]), want_a[k]), k
    for k in keys_e:
        assert np.array_equal(s.down(d[k], want_e[k]), want_e[k]), k
    got = s.down(d_st, np.zeros(len(qr.QSTAT_NAMES), np.uint64))
    assert {k: int(got[i]) for i, k in enumerate(R.QSTAT_NAMES)} == st
    s.close()
