"""qb_dev_leader_tick on the device against tests/tick_ref.py, bit-exact after
every tick: every in/out array of the table (so nothing but meta's transferee
byte and pstate's RecentActive bit can have moved), the tick's own state,
tflags, the accumulated stats, and hb_commit / hb_ctx including the elements a
tick must leave untouched (both pre-filled with 0xA5A5...).  All comparisons
are integer equality."""
import ctypes as C

import numpy as np
import pytest
import torch

from etcd_amd import _lib
from etcd_amd.quorum import leader as ql, tick as qt
from tests import tick_pack as P, tick_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL_I64 = P.FILL - (1 << 64)


class DeviceRun:
    """A batch of TickNodes on the device beside its reference copy."""

    def __init__(self, nodes, readq_cap, arrays=None, tick_arrays=None):
        self.nodes, self.readq_cap = nodes, readq_cap
        a, t = P.pack_nodes(nodes, readq_cap)
        self.off = a["off"]              # the reference's (dense) slot offsets
        self.a = arrays if arrays is not None else a
        self.lg = ql.LeaderGroups(self.a, 1, readq_cap, device=DEV)
        self.state = qt.TickState.from_numpy(**(tick_arrays or t), device=DEV)
        G, S = self.lg.G, self.lg.S
        self.out = qt.TickResult(torch.full((max(G, 1),), 0xA5, dtype=torch.uint8, device=DEV),
                                 torch.full((max(S, 1),), FILL_I64, dtype=torch.int64, device=DEV),
                                 torch.full((max(G, 1),), FILL_I64, dtype=torch.int64, device=DEV),
                                 torch.zeros(8, dtype=torch.int64, device=DEV), self.lg)
        self.hb_commit = np.full(int(self.off[-1]), P.FILL, np.uint64)
        self.hb_ctx = np.full(G, P.FILL, np.uint64)
        self.stats = {k: 0 for k in T.TSTAT_NAMES}

    def expected_arrays(self):
        return P.pack_nodes(self.nodes, self.readq_cap)

    def hb_commit_layout(self, dense):
        return dense

    def tick(self, et, ht, cq, where):
        G = self.lg.G
        self.lg.tick(self.state, et, ht, bool(cq), out=self.out)
        tf, st = P.ref_tick(self.nodes, self.off, et, ht, cq, self.hb_commit, self.hb_ctx)
        for k, v in st.items():
            self.stats[k] += v
        got_tf = self.out.tflags.cpu().numpy()[:G]
        assert np.array_equal(got_tf, tf), (where, "tflags", np.nonzero(got_tf != tf)[0][:8])
        want_a, want_t = self.expected_arrays()
        got_a = self.lg.numpy()
        for key, want in want_a.items():
            assert np.array_equal(got_a[key], want), (where, key)
        got_t = self.state.numpy(G)
        for key, want in want_t.items():
            assert np.array_equal(got_t[key], want), (where, key)
        hc = ql._to_np(self.out.hb_commit, np.uint64, self.lg.S)
        assert np.array_equal(hc, self.hb_commit_layout(self.hb_commit)), (where, "hb_commit")
        assert np.array_equal(ql._to_np(self.out.hb_ctx, np.uint64, G), self.hb_ctx), (where, "hb_ctx")
        assert self.out.stats_dict() == self.stats, (where, self.out.stats_dict(), self.stats)
        return tf

    def set_recent_active(self, mask):
        """RecentActive := true where mask (dense per-slot), on both sides."""
        P.set_recent_active(self.nodes, self.off, mask)
        m = torch.from_numpy(self.hb_commit_layout(mask.astype(np.uint8) * 8)).to(DEV)
        self.lg.t["pstate"][: m.numel()] |= m


# --------------------------------------------------------- golden scenarios ---

SCENARIOS = P.load_tables()["scenarios"]


@pytest.mark.parametrize("sc", SCENARIOS, ids=[s["name"] for s in SCENARIOS])
def test_golden_scenarios_on_device(sc):
    """The reference's tests, G = 1 each, through the device: the transcribed
    expectations hold for the device's messages, and the device equals
    tick_ref after every tick."""
    run = DeviceRun([P.build_node(sc)], 0)
    node = run.nodes[0]
    for k, op in enumerate(sc["ops"]):
        if op["op"] == "hb_resp":
            mask = np.zeros(node.group.n_slots, bool)
            mask[op["slot"]] = True
            run.set_recent_active(mask)
            continue
        where = f"{sc['name']} op{k}"
        run.tick(sc["election_timeout"], sc["heartbeat_timeout"], sc["check_quorum"], where)
        msgs = run.out.heartbeats(0)
        P.check_tick_expect(where, op["expect"], msgs, node)


# --------------------------------------------------------------------- fuzz ---

@pytest.mark.parametrize("readq_cap", [0, 4, 16])
@pytest.mark.parametrize("timeouts", P.TIMEOUTS, ids=lambda t: "et%d_ht%d_cq%d" % t)
@pytest.mark.parametrize("G", [1, 255, 257, 1031])
def test_fuzz_consecutive_ticks(G, timeouts, readq_cap):
    """Ragged seeded batches (tick_pack.random_nodes) for 2 * election_timeout
    + 2 consecutive ticks with no host repair in between; a seeded fraction of
    RecentActive bits is set on both sides between ticks.  (3,3,1) and (1,1,1)
    put the sweep and the beat on one tick: a step-down suppresses the beat."""
    et, ht, cq = timeouts
    rng = np.random.default_rng(1000 * G + 100 * et + 10 * ht + cq + readq_cap)
    run = DeviceRun(P.random_nodes(rng, G, readq_cap, et, ht), readq_cap)
    S = int(run.off[-1])
    seen = 0
    for k in range(2 * et + 2):
        run.set_recent_active(rng.random(S) < 0.3)
        tf = run.tick(et, ht, cq, f"G{G} {timeouts} rq{readq_cap} tick {k}")
        seen |= int(np.bitwise_or.reduce(tf))
        for g in (0, G // 2, G - 1):   # the mirror's message view == the reference's
            got = run.out.heartbeats(g)
            assert [(m["to"], m["commit"], m["aux"]) for m in got] == \
                [(m.to, m.commit, m.aux) for m in run.nodes[g].msgs]
    if G >= 255:  # every branch was reached
        want = T.TFLAG_HUP | T.TFLAG_BEAT | T.TFLAG_TRANSFER_ABORTED
        if cq:
            want |= T.TFLAG_CHECK_QUORUM | T.TFLAG_STEPPED_DOWN
        assert seen & want == want, hex(seen)


# ---------------------------------------------------------------- wide span ---

def wide_nodes(G, ee, he):
    rng = np.random.default_rng(G)
    nodes = []
    for i in range(G):
        match = [int(x) for x in rng.integers(0, 100, 16)]
        g = P.make_group(16, 0x0FFF, 0xF000 if i % 3 == 0 else 0, i % 16, 50, match,
                         rng.random(16) < 0.45, readq_ctx=(i + 1,))
        nodes.append(T.TickNode(g, T.LEADER | T.ROLE_PROMOTABLE, ee, he, 15))
    return nodes


def test_wide_span_sweep_and_beat():
    """300 groups of 16 slots: a workgroup's 256 groups span 4096 slots, the
    widest a well-formed table gets (and past any stage sized like the leader
    step's 1536).  One sweep tick, then one beat tick."""
    run = DeviceRun(wide_nodes(300, 9, 0), 1)
    tf = run.tick(10, 2, 1, "wide sweep")
    assert (tf & T.TFLAG_CHECK_QUORUM).all() and not (tf & T.TFLAG_BEAT).any()
    assert (tf & T.TFLAG_STEPPED_DOWN).any() and not (tf & T.TFLAG_STEPPED_DOWN).all()
    tf = run.tick(10, 2, 1, "wide beat")
    assert ((tf & T.TFLAG_BEAT) != 0).sum() == 300 - run.stats["stepped_down"]


class GappedRun(DeviceRun):
    """The same batch in a table whose groups sit `stride` slots apart: the
    slots between a group's end and the next group's start belong to nobody
    and must keep their bytes."""

    def __init__(self, nodes, readq_cap, stride):
        a, t = P.pack_nodes(nodes, readq_cap)
        G = len(nodes)
        self.stride, self.dense_off = stride, a["off"].astype(np.int64)
        self.goff = np.arange(G + 1, dtype=np.uint32) * stride
        super().__init__(nodes, readq_cap, arrays=self.spread_arrays(a))

    def scatter(self, dense, fill):
        out = np.full(int(self.goff[-1]), fill, dtype=dense.dtype)
        for i in range(len(self.goff) - 1):
            n = int(self.dense_off[i + 1] - self.dense_off[i])
            out[int(self.goff[i]):int(self.goff[i]) + n] = dense[self.dense_off[i]:self.dense_off[i + 1]]
        return out

    def spread_arrays(self, a):
        b = dict(a)
        b["off"] = self.goff
        for k, fill in (("match", 7), ("next", 8), ("pending_snapshot", 0), ("pstate", 0x09),
                        ("infl_pos", 0), ("infl_buf", 0)):
            b[k] = self.scatter(a[k], fill)
        return b

    def expected_arrays(self):
        a, t = P.pack_nodes(self.nodes, self.readq_cap)
        return self.spread_arrays(a), t

    def hb_commit_layout(self, dense):
        return self.scatter(dense, P.FILL if dense.dtype == np.uint64 else 0)


def test_gapped_table_takes_the_unstaged_path_and_reads_at_most_16_slots():
    """Groups 20 slots apart, 16 of them the group's own Progress and 4 that
    the tick must read as absent (a slot count above 16 is read as 16): a
    workgroup's span is 5120 slots, wider than its LDS stage, so the slot
    phases run from the global arrays.  The four slots past each group keep
    their RecentActive bit and their hb_commit fill."""
    run = GappedRun(wide_nodes(300, 9, 1), 1, stride=20)
    tf = run.tick(10, 2, 1, "gapped sweep + beat")
    assert (tf & T.TFLAG_CHECK_QUORUM).all() and (tf & T.TFLAG_BEAT).any()
    assert (tf & T.TFLAG_STEPPED_DOWN).any()
    run.set_recent_active(np.ones(int(run.off[-1]), bool))
    run.tick(10, 2, 1, "gapped idle")
    run.tick(10, 2, 1, "gapped beat")


# ---------------------------------------------------------------- singleton ---

def test_singleton_leader_beats_nobody_and_wins_its_own_sweep():
    g = P.make_group(1, 1, 0, 0, 5, [5], [False])
    run = DeviceRun([T.TickNode(g, T.LEADER | T.ROLE_PROMOTABLE, 1, 0, 4)], 0)
    tf = run.tick(3, 1, 1, "singleton beat")
    assert tf[0] == T.TFLAG_BEAT and run.out.heartbeats(0) == []
    tf = run.tick(3, 1, 1, "singleton sweep")
    assert tf[0] == T.TFLAG_BEAT | T.TFLAG_CHECK_QUORUM
    assert run.stats["heartbeats"] == 0 and run.stats["stepped_down"] == 0
    assert run.lg.numpy()["pstate"][0] & 8


# -------------------------------------------------------------- loop closed ---

def test_tick_heartbeats_responses_step_close_the_loop():
    """64 five-voter leaders with CheckQuorum: tick to a beat, answer the
    heartbeats of three peers per group through the leader step
    (QB_IN_HEARTBEAT_RESP), tick on to the sweep: nobody steps down.  The
    same with one peer answering: everybody does.  meta stays a word the step
    accepts: only the transferee byte may differ from what the step left."""
    G, n, et = 64, 5, 10
    lg, _ = ql.synth_streaming(G, W=4, D=1, n=n, device=DEV)
    lg.t["pstate"].fill_(1)  # Replicate, nobody RecentActive yet
    state = qt.TickState.from_numpy(np.full(G, T.LEADER | T.ROLE_PROMOTABLE, np.uint8),
                                    np.zeros(G, np.uint32), np.zeros(G, np.uint32),
                                    np.full(G, 15, np.uint32), device=DEV)
    meta0 = lg.numpy()["meta"].copy()
    term = int(lg.numpy()["term"][0])

    def answer(peers):
        res = lg.tick(state, et, 1, True)
        tf = res.tflags.cpu().numpy()
        assert (tf == T.TFLAG_BEAT).all()
        hbs = [res.heartbeats(g) for g in range(G)]
        assert all([m["to"] for m in h] == [1, 2, 3, 4] for h in hbs)
        grp = np.repeat(np.arange(G, dtype=np.uint32), len(peers))
        slot = np.tile(np.array(peers, np.uint8), G)
        ctx = np.array([hbs[g][0]["aux"] for g in grp], np.uint64)
        ib = ql.LeaderInbox.from_numpy(grp, slot, np.full(len(grp), ql.IN_HEARTBEAT_RESP, np.uint8),
                                       ctx, np.full(len(grp), term, np.uint64), device=DEV)
        r = lg.step(ib)
        assert r.stats["applied"] == len(grp)
        return res

    def to_sweep():
        flags = []
        for _ in range(et - 1):
            flags.append(lg.tick(state, et, 1, True).tflags.cpu().numpy().copy())
        return flags

    answer((1, 2, 3))
    flags = to_sweep()
    assert all((f == T.TFLAG_BEAT).all() for f in flags[:-1])
    assert (flags[-1] == T.TFLAG_BEAT | T.TFLAG_CHECK_QUORUM).all()     # 4 of 5 active
    a = lg.numpy()
    assert np.array_equal(a["meta"], meta0)
    assert np.array_equal(a["pstate"] & 8, np.tile(np.array([8, 0, 0, 0, 0], np.uint8), G))
    answer((4,))
    flags = to_sweep()
    assert (flags[-1] == T.TFLAG_CHECK_QUORUM | T.TFLAG_STEPPED_DOWN).all()  # 2 of 5
    a, s = lg.numpy(), state.numpy(G)
    assert np.array_equal(a["meta"], meta0) and not (a["pstate"] & 8).any()
    assert (s["role"] == T.FOLLOWER | T.ROLE_PROMOTABLE).all()
    assert not s["election_elapsed"].any() and not s["heartbeat_elapsed"].any()


# ------------------------------------------------------------------ raw ABI ---

def test_tick_raw_abi():
    """One call through plain ctypes with the library's own stream, memory and
    copies (no torch), as a cgo embedder makes it."""
    from tests.test_gpu_abi_raw import Stream
    et, ht, cq, rcap = 3, 1, 1, 4
    rng = np.random.default_rng(77)
    nodes = P.random_nodes(rng, 600, rcap, et, ht)
    a, t = P.pack_nodes(nodes, rcap)
    G, S = len(nodes), int(a["off"][-1])
    s = Stream()
    d = {k: s.up(a[k]) for k in ("off", "cfg", "meta", "committed", "match", "pstate", "rq_ctx")}
    d.update({k: s.up(v) for k, v in t.items()})
    tg = qt.TickGroupsC(G=G, readq_cap=rcap, election_timeout=et, heartbeat_timeout=ht,
                        check_quorum=cq, **d)
    d_tf, d_hc, d_hx, d_st = s.zeros(G, 0xA5), s.zeros(8 * S, 0xA5), s.zeros(8 * G, 0xA5), s.zeros(64)
    _lib.check(s.lib.qb_dev_leader_tick(C.byref(tg), d_tf, d_hc, d_hx, d_st, s.st), "tick")
    hc, hx = np.full(S, P.FILL, np.uint64), np.full(G, P.FILL, np.uint64)
    tf, st = P.ref_tick(nodes, a["off"], et, ht, cq, hc, hx)
    want_a, want_t = P.pack_nodes(nodes, rcap)
    assert np.array_equal(s.down(d_tf, tf), tf)
    assert np.array_equal(s.down(d_hc, hc), hc) and np.array_equal(s.down(d_hx, hx), hx)
    for k in ("meta", "pstate", "committed", "match", "cfg", "off", "rq_ctx"):
        assert np.array_equal(s.down(d[k], want_a[k]), want_a[k]), k
    for k in want_t:
        assert np.array_equal(s.down(d[k], want_t[k]), want_t[k]), k
    got = s.down(d_st, np.zeros(8, np.uint64))
    assert {k: int(got[i]) for i, k in enumerate(T.TSTAT_NAMES)} == st
    s.close()
