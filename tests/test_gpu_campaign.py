"""qb_dev_campaign on the device against tests/campaign_ref.py, bit-exact after
every call: every array of the table and of the election state (so nothing a
transition does not own can have moved — the Progress of groups that do not
reset holds seeded junk, and the gaps of a gapped table a sentinel), cflags,
req_type, req_term / req_mask including the elements a call must leave
untouched (pre-filled with 0xA5...), and the accumulated stats.  All
comparisons are integer equality."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from etcd_amd import _lib
from etcd_amd.quorum import batch, follower as qf, leader as ql, tick as qt
from tests import campaign_loop as loop, campaign_pack as P, campaign_ref as R, tick_ref as T
from tests.test_campaign_ref import SCENARIOS, replay

qc = importlib.import_module("etcd_amd.quorum.campaign")

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL_I64 = P.FILL - (1 << 64)
FILL16 = 0xA5A5


class DeviceRun:
    """A batch of CampaignNodes on the device beside its reference copy."""

    def __init__(self, nodes, pre_vote, readq_cap=0, rand_timeout=None, check_quorum=True):
        self.nodes, self.pre_vote, self.readq_cap = nodes, bool(pre_vote), readq_cap
        a, e = P.pack_nodes(nodes, readq_cap)
        self.lg = ql.LeaderGroups(self.layout(a), P.INFLIGHT_CAP, readq_cap, device=DEV)
        G = self.lg.G
        rt = rand_timeout if rand_timeout is not None else np.zeros(G, np.uint32)
        self.state = qt.TickState.from_numpy(e["role"], e["election_elapsed"],
                                             e["heartbeat_elapsed"], rt, device=DEV)
        self.es = qc.ElectionState.for_table(self.lg, self.state, e["self_id"], e["vote"],
                                             e["lead"], e["last_term"], loop.ET, check_quorum,
                                             self.pre_vote, votes=e["votes"])
        n = max(G, 1)
        self.out = qc.CampaignResult(torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV),
                                     torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV),
                                     torch.full((n,), FILL_I64, dtype=torch.int64, device=DEV),
                                     torch.full((n,), FILL16 - (1 << 16), dtype=torch.int16,
                                                device=DEV),
                                     torch.zeros(len(qc.CSTAT_NAMES), dtype=torch.int64, device=DEV))
        self.req_term = np.full(G, P.FILL, np.uint64)
        self.req_mask = np.full(G, FILL16, np.uint16)
        self.stats = R.new_stats()
        # the read queue's contents are dead after a reset (only its length in
        # meta is cleared): no call here may write them at all
        self.rq0 = {k: v.copy() for k, v in self.lg.numpy().items() if k.startswith("rq_")}

    def layout(self, a):
        """The table as the device holds it (the dense one here)."""
        return a

    def check_state(self, where):
        G = self.lg.G
        a, e = P.pack_nodes(self.nodes, self.readq_cap)
        want = self.layout(a)
        got = self.lg.numpy()
        want.update(self.rq0)
        for key in got:
            assert np.array_equal(got[key], want[key]), (where, key,
                                                         np.flatnonzero(got[key] != want[key])[:8])
        ge = self.es.numpy()
        e.update(term=a["term"], committed=a["committed"], last_index=a["last_index"])
        for key, w in e.items():
            assert np.array_equal(ge[key], w), (where, key, np.flatnonzero(ge[key] != w)[:8])
        assert ge.keys() == e.keys()
        return G

    def campaign(self, action, where):
        action = np.asarray(action, np.uint8)
        res = self.lg.campaign(self.es, torch.from_numpy(action.copy()).to(DEV), out=self.out)
        assert res is self.out
        cf, rt, st = P.ref_campaign(self.nodes, action, self.pre_vote, self.req_term, self.req_mask)
        for k, v in st.items():
            self.stats[k] += v
        G = self.check_state(where)
        got_cf, got_rt = res.cflags.cpu().numpy()[:G], res.req_type.cpu().numpy()[:G]
        assert np.array_equal(got_cf, cf), (where, "cflags", np.flatnonzero(got_cf != cf)[:8])
        assert np.array_equal(got_rt, rt), (where, "req_type", np.flatnonzero(got_rt != rt)[:8])
        assert np.array_equal(ql._to_np(res.req_term, np.uint64, G), self.req_term), (where, "req_term")
        assert np.array_equal(ql._to_np(res.req_mask, np.uint16, G), self.req_mask), (where, "req_mask")
        assert res.stats_dict() == self.stats, (where, res.stats_dict(), self.stats)
        return cf, rt

    def requests_match(self, g):
        got = self.out.requests(g)
        assert [tuple(m[k] for k in ("type", "to", "term", "index", "log_term", "transfer"))
                for m in got] == [r.key() for r in self.nodes[g].reqs], g
        return got


# --------------------------------------------------------- golden scenarios ---

@pytest.mark.parametrize("sc", SCENARIOS, ids=[s["name"] for s in SCENARIOS])
def test_golden_scenarios_on_device(sc):
    """The reference's tests, G = 1 each, through the device: the transcribed
    expectations hold for the device's outputs, and the device equals
    campaign_ref after every call.  (A vote response is recorded on the
    reference side and the votes word copied over; the outcome it decides is
    a device call.)"""
    run = None

    def apply(n, act):
        nonlocal run
        if run is None:
            run = DeviceRun([n], sc["pre_vote"])
        run.es.votes[0] = int(np.array([P.votes_word(n.votes)], np.uint32).view(np.int32)[0])
        cf, _ = run.campaign([act], sc["name"])
        return int(cf[0]), run.requests_match(0)
    replay(sc, apply)


# --------------------------------------------------------------------- fuzz ---

@pytest.mark.parametrize("pre_vote", [0, 1])
@pytest.mark.parametrize("G", [1, 255, 256, 257, 513])
def test_fuzz_two_calls(G, pre_vote):
    """Ragged seeded batches (campaign_pack.random_nodes: 1-16 slots,
    learners, joint and empty configs, every role, bad action codes) through
    two calls into the same outputs: the second acts on what the first left
    (candidates win and lose, leaders ignore), and the stats accumulate."""
    rng = np.random.default_rng(100 * G + pre_vote)
    run = DeviceRun(P.random_nodes(rng, G, readq_cap=4), pre_vote, readq_cap=4)
    for k in range(2):
        run.campaign(P.random_actions(rng, G), f"G{G} pv{pre_vote} call {k}")
        for g in (0, G // 2, G - 1):
            run.requests_match(g)
    if G >= 255:  # every branch was reached
        assert all(run.stats[k] > 0 for k in R.CSTAT_NAMES if pre_vote or k != "pre_campaigns"), \
            run.stats


@pytest.mark.parametrize("pre_vote", [0, 1])
def test_every_action_role_promotable_pending_combination(pre_vote):
    """513 groups: every action x role x promotable bit x QB_CAMP_PENDING_CONF
    six times over seeded configs, and 33 more at random."""
    rng = np.random.default_rng(7 + pre_vote)
    nodes = P.random_nodes(rng, 513)
    action = P.random_actions(rng, 513)
    combos = [(a, r, p, c) for a in range(5) for r in range(4) for p in (0, 1) for c in (0, 1)]
    for i in range(480):
        a, r, p, c = combos[i % 80]
        nodes[i].role = r | (R.ROLE_PROMOTABLE if p else 0)
        action[i] = a | (R.CAMP_PENDING_CONF if c else 0)
    run = DeviceRun(nodes, pre_vote)
    cf, rt = run.campaign(action, "combinations")
    seen = {(int(action[i]) & 0x7F, int(cf[i])) for i in range(480)}
    for want in (R.CFLAG_IGNORED, R.CFLAG_REQUESTS, R.CFLAG_BECAME_LEADER, R.CFLAG_BCAST_APPEND):
        assert any(f & want for _, f in seen), hex(want)
    assert all(f == 0 for a, f in seen if a == R.CAMP_NONE)
    assert ((rt & 0x7F) == R.MSG_PREVOTE).any() == bool(pre_vote)


# --------------------------------------------------------------- skip paths ---

def test_idle_tile_and_single_reset_tile():
    """Three tiles: seeded actions, no action at all, and exactly one group
    that resets (a candidate that lost) among 255 idle ones."""
    rng = np.random.default_rng(31)
    nodes = P.random_nodes(rng, 768)
    action = np.zeros(768, np.uint8)
    action[:256] = P.random_actions(rng, 256)
    nodes[600].role = R.CANDIDATE
    action[600] = R.CAMP_LOST
    run = DeviceRun(nodes, 1)
    cf, _ = run.campaign(action, "skip paths")
    assert not cf[256:600].any() and not cf[601:].any()
    assert cf[600] & R.CFLAG_RESET and run.stats["became_follower"] >= 1
    run.campaign(np.zeros(768, np.uint8), "all idle")


# -------------------------------------------------------------------- edges ---

def edge_nodes():
    """(name, node) of the cases a seeded batch may miss."""
    P_ = R.ROLE_PROMOTABLE
    mk = P.make_node
    rng = np.random.default_rng(99)
    kw = dict(term=4, last_index=7, last_term=4, committed=3, rng=rng)
    out = [
        ("single voter", mk(1, 1, 0, 0, role=P_, **kw)),
        ("single voter, committed ahead", mk(1, 1, 0, 0, role=P_, term=4, last_index=7, last_term=4,
                                             committed=8, rng=rng)),
        ("single voter with learners", mk(4, 0b0100, 0, 2, role=P_, **kw)),
        ("single voter in both halves", mk(3, 0b010, 0b010, 1, role=P_, **kw)),
        ("joint: outgoing {self}, incoming not", mk(3, 0b111, 0b001, 0, role=P_, **kw)),
        ("joint: incoming empty, outgoing {self}", mk(3, 0, 0b001, 0, role=P_, **kw)),
        ("own slot 0 of 16", mk(16, 0xFFFF, 0, 0, role=P_, **kw)),
        ("own slot 15 of 16", mk(16, 0xFFFF, 0, 15, role=P_, **kw)),
        ("own slot last of 5", mk(5, 0b11111, 0, 4, role=P_, **kw)),
        ("own slot == slot count", mk(3, 0b111, 0, 3, role=P_, **kw)),
        ("own slot 0xFF", mk(3, 0b111, 0, 0xFF, role=P_, **kw)),
        ("own slot a learner", mk(3, 0b011, 0, 2, role=P_, **kw)),
        ("nobody votes", mk(3, 0, 0, 1, role=P_, **kw)),
        ("term 2^64 - 1", mk(3, 0b111, 0, 1, role=P_, term=(1 << 64) - 1, last_index=7, last_term=4,
                             committed=3, rng=rng)),
        ("last_index 2^40", mk(3, 0b111, 0, 1, role=P_, term=4, last_index=1 << 40, last_term=4,
                               committed=9, rng=rng)),
        ("last_index 2^63 - 1, alone", mk(1, 1, 0, 0, role=P_, term=4, last_index=(1 << 63) - 1,
                                          last_term=4, committed=9, rng=rng)),
        ("last_index 2^63", mk(3, 0b111, 0, 1, role=P_, term=4, last_index=1 << 63, last_term=4,
                               committed=1 << 62, rng=rng)),
    ]
    return out


@pytest.mark.parametrize("pre_vote", [0, 1])
def test_edges_under_every_action(pre_vote):
    """Every edge node as follower, pre-candidate and candidate under HUP,
    TRANSFER, WON and LOST (one group each), then a second call of outcomes
    on what the first left."""
    import copy
    base = edge_nodes()
    nodes, action, names = [], [], []
    for name, n in base:
        for state in (R.FOLLOWER, R.PRE_CANDIDATE, R.CANDIDATE):
            for act in (R.CAMP_HUP, R.CAMP_TRANSFER, R.CAMP_WON, R.CAMP_LOST):
                m = copy.deepcopy(n)
                m.role = m.role & ~3 | state
                nodes.append(m)
                action.append(act)
                names.append((name, state, act))
    run = DeviceRun(nodes, pre_vote)
    cf, rt = run.campaign(action, "edges")
    by = {k: i for i, k in enumerate(names)}

    def at(name, state, act):
        i = by[(name, state, act)]
        return run.nodes[i], int(cf[i]), int(rt[i])
    # leader in one call, committed advancing only when it should
    for name, com in (("single voter", 8), ("single voter, committed ahead", 8),
                      ("single voter with learners", 8), ("single voter in both halves", 8),
                      ("joint: incoming empty, outgoing {self}", 8)):
        n, f, t = at(name, R.FOLLOWER, R.CAMP_HUP)
        assert n.state == R.LEADER and t == 0 and n.group.log.committed == com, name
        assert f & R.CFLAG_BECAME_LEADER and not f & R.CFLAG_BCAST_APPEND, name
        assert run.stats["pre_campaigns"] > 0 or not pre_vote
    n, f, t = at("single voter, committed ahead", R.FOLLOWER, R.CAMP_HUP)
    assert f & R.CFLAG_HARDSTATE  # (term and vote moved; committed did not)
    n, f, t = at("joint: outgoing {self}, incoming not", R.CANDIDATE, R.CAMP_WON)
    assert n.state == R.LEADER and n.group.log.committed == 3 and f & R.CFLAG_BCAST_APPEND
    n, f, t = at("joint: outgoing {self}, incoming not", R.FOLLOWER, R.CAMP_HUP)
    assert n.state != R.LEADER and t != 0
    for name in ("own slot == slot count", "own slot 0xFF", "own slot a learner"):
        n, f, t = at(name, R.FOLLOWER, R.CAMP_HUP)
        assert f == R.CFLAG_IGNORED and n.state == R.FOLLOWER, name
    n, f, t = at("term 2^64 - 1", R.FOLLOWER, R.CAMP_TRANSFER)
    assert n.group.term == 0 and n.state == R.CANDIDATE and t == R.MSG_VOTE | R.CREQ_TRANSFER
    n, f, t = at("last_index 2^63", R.CANDIDATE, R.CAMP_WON)
    assert n.group.prs[1].match == (1 << 63) + 1 and n.group.prs[0].next == (1 << 63) + 1
    for g in range(len(nodes)):
        run.requests_match(g)
    rng = np.random.default_rng(3)
    run.campaign(rng.integers(3, 5, len(nodes)).astype(np.uint8), "edges: outcomes")


# ---------------------------------------------------------------- wide span ---

class GappedRun(DeviceRun):
    """The same batch in a table whose groups sit `stride` slots apart: the
    slots between a group's end and the next group's start belong to nobody
    and must keep their bytes."""
    FILLS = (("match", 7), ("next", 8), ("pending_snapshot", 9), ("pstate", 0x0D), ("infl_pos", 1),
             ("infl_buf", 5))

    def __init__(self, nodes, pre_vote, stride):
        self.stride = stride
        super().__init__(nodes, pre_vote)

    def layout(self, a):
        G = len(a["cfg"])
        dense = a["off"].astype(np.int64)
        goff = np.arange(G + 1, dtype=np.uint32) * self.stride
        b = dict(a)
        b["off"] = goff
        for key, fill in self.FILLS:
            w = P.INFLIGHT_CAP if key == "infl_buf" else 1
            out = np.full(int(goff[-1]) * w, fill, dtype=a[key].dtype)
            for i in range(G):
                n = int(dense[i + 1] - dense[i]) * w
                out[int(goff[i]) * w:int(goff[i]) * w + n] = a[key][dense[i] * w:dense[i + 1] * w]
            b[key] = out
        return b


@pytest.mark.parametrize("pre_vote", [0, 1])
def test_gapped_table_takes_the_unstaged_path_and_writes_at_most_16_slots(pre_vote):
    """300 groups of 16 slots, 20 slots apart: a workgroup's span is 5120
    slots, wider than its LDS stage, so the slot phase runs from the global
    arrays.  Every group declares 20 slots, read as 16; the four slots past
    each group keep their sentinels."""
    rng = np.random.default_rng(20 + pre_vote)
    nodes = []
    for i in range(300):
        vin, vout = P.random_config(rng, 16)
        nodes.append(P.make_node(16, vin, vout, i % 16, self_id=i + 1, term=5, last_index=40 + i,
                                 last_term=5, committed=i, rng=rng,
                                 role=int(rng.integers(0, 4)) | R.ROLE_PROMOTABLE))
    run = GappedRun(nodes, pre_vote, stride=20)
    run.campaign(P.random_actions(rng, 300, p_none=0.1), "gapped")
    assert run.stats["became_leader"] and run.stats["became_follower"] and run.stats["campaigns"]
    run.campaign(P.random_actions(rng, 300, p_none=0.1), "gapped, second call")


# ----------------------------------------------------------------- the loop ---

class DeviceCluster:
    """campaign_loop's cluster interface over the device, beside a RefCluster:
    every method runs both, compares the outputs and every array of the
    node's table, and returns the device's outputs."""

    def __init__(self, nodes, rand, pre_vote):
        self.ref = loop.RefCluster(nodes, rand, pre_vote)
        self.N, self.G = self.ref.N, self.ref.G
        self.runs = [DeviceRun(nodes[j], pre_vote, rand_timeout=rand[j]) for j in range(self.N)]
        self.csr = [batch.CsrGroups(r.lg.t["off"], r.lg.t["cfg"], r.lg.t["match"], votes=r.es.votes)
                    for r in self.runs]
        self.calls = 0

    def _same(self, what, j, got, want):
        assert np.array_equal(got, want), (what, j, np.flatnonzero(got != want)[:8])
        self.runs[j].check_state(f"{what} node {j}")
        self.calls += 1
        return got

    def tick(self, j):
        r = self.runs[j]
        res = r.lg.tick(r.state, loop.ET, loop.HT, True)
        return self._same("tick", j, res.tflags.cpu().numpy()[:self.G], self.ref.tick(j))

    def campaign(self, j, action):
        cf, rt = self.runs[j].campaign(action, f"campaign node {j}")
        self.calls += 1
        o = self.runs[j].out
        return cf, rt, ql._to_np(o.req_term, np.uint64, self.G), ql._to_np(o.req_mask, np.uint16, self.G)

    def requests(self, j, g):
        return self.runs[j].requests_match(g)

    def follower_step(self, j, recs):
        from tests import follower_pack
        r = self.runs[j]
        cols = follower_pack.pack_recs(recs)
        ib = qf.FollowerInbox.from_numpy(cols["group"], cols["flags"], cols["from"], cols["term"],
                                         cols["index"], cols["aux"], device=DEV)
        res = qf.follower_step(r.es.follower, ib)
        want_rt, want_term = self.ref.follower_step(j, recs)
        M = len(recs)
        got_rt = res.resp_type.cpu().numpy()[:M]
        got_term = ql._to_np(res.resp_term, np.uint64, M)
        assert np.array_equal(got_term, want_term), ("resp_term", j)
        assert (ql._to_np(res.stop_at, np.uint32, self.G) == qf.NO_STOP).all()
        return self._same("follower step", j, got_rt, want_rt), got_term

    def record_votes(self, j, prevote, recs):
        r = self.runs[j]
        b = batch.AppRespBatch.from_numpy([x[0] for x in recs], [x[1] for x in recs],
                                          np.zeros(len(recs), np.uint64),
                                          np.array([x[3] for x in recs], np.uint64),
                                          [x[2] for x in recs], device=DEV)
        sd, dec, _ = self.csr[j].record_votes(b, r.lg.t["term"], prevote=prevote)
        want_sd, want_dec = self.ref.record_votes(j, prevote, recs)
        got_dec = ql._to_np(dec, np.uint32, self.G)
        assert np.array_equal(got_dec, want_dec), ("decided_at", j)
        return self._same("record votes", j, ql._to_np(sd, np.uint32, self.G), want_sd), got_dec

    def tally(self, j):
        res = self.csr[j].tally_votes()[2]
        return self._same("tally", j, res.cpu().numpy()[:self.G], self.ref.tally(j))


@pytest.mark.parametrize("pre_vote", [0, 1])
@pytest.mark.parametrize("N", [3, 5])
def test_the_election_loop(N, pre_vote):
    """300 groups x N nodes, one table per node, a seeded mix of up-to-date
    and stale logs and of one, two or N candidates per group: tick until
    MsgHup, campaign, follower step on the peers with the requests formed
    from requests(g), record votes, tally, campaign (WON / LOST), one leader
    tick — the device and the restatements side by side, every array compared
    after every call.  The device ends with exactly the restatement's
    leaders, and each of them beats."""
    nodes, rand = loop.make_cluster(1000 + 10 * N + pre_vote, N, 300)
    c = DeviceCluster(nodes, rand, bool(pre_vote))
    rounds, tf = loop.run_election(c)
    assert rounds == (3 if pre_vote else 2) and c.calls > 4 * N
    leaders = 0
    for j in range(N):
        role = c.runs[j].state.numpy(300)["role"]
        want = np.array([n.role for n in nodes[j]], np.uint8)
        assert np.array_equal(role, want)
        lead = (role & 3) == R.LEADER
        assert np.array_equal((tf[j] & T.TFLAG_BEAT) != 0, lead)
        leaders += int(lead.sum())
    per_group = sum(((c.runs[j].state.numpy(300)["role"] & 3) == R.LEADER).astype(int)
                    for j in range(N))
    assert per_group.max() == 1 and 100 < leaders < 300
    st = [c.runs[j].stats for j in range(N)]
    assert sum(s["became_leader"] for s in st) == leaders
    assert sum(s["became_follower"] for s in st) > 0


# ------------------------------------------------------------------ raw ABI ---

def test_campaign_raw_abi():
    """One call through plain ctypes with the library's own stream, memory and
    copies (no torch), as a cgo embedder makes it."""
    from tests.test_gpu_abi_raw import Stream
    rng = np.random.default_rng(78)
    G = 600
    nodes = P.random_nodes(rng, G)
    action = P.random_actions(rng, G)
    a, e = P.pack_nodes(nodes)
    s = Stream()
    keys_a = ("off", "cfg", "meta", "term", "committed", "last_index", "match", "next",
              "pending_snapshot", "pstate", "infl_pos")
    d = {k: s.up(a[k]) for k in keys_a}
    d.update({k: s.up(v) for k, v in e.items()})
    cg = qc.CampaignGroupsC(G=G, pre_vote=1, reserved=0, **d)
    d_act = s.up(action)
    d_cf, d_rt = s.zeros(G, 0xA5), s.zeros(G, 0xA5)
    d_term, d_mask, d_st = s.zeros(8 * G, 0xA5), s.zeros(2 * G, 0xA5), s.zeros(8 * len(qc.CSTAT_NAMES))
    _lib.check(s.lib.qb_dev_campaign(C.byref(cg), d_act, d_cf, d_rt, d_term, d_mask, d_st, s.st),
               "campaign")
    req_term, req_mask = np.full(G, P.FILL, np.uint64), np.full(G, FILL16, np.uint16)
    cf, rt, st = P.ref_campaign(nodes, action, True, req_term, req_mask)
    want_a, want_e = P.pack_nodes(nodes)
    assert np.array_equal(s.down(d_cf, cf), cf) and np.array_equal(s.down(d_rt, rt), rt)
    assert np.array_equal(s.down(d_term, req_term), req_term)
    assert np.array_equal(s.down(d_mask, req_mask), req_mask)
    assert np.array_equal(s.down(d_act, action), action)
    for k in keys_a:
        assert np.array_equal(s.down(d[k], want_a[k]), want_a[k]), k
    for k in want_e:
        assert np.array_equal(s.down(d[k], want_e[k]), want_e[k]), k
    got = s.down(d_st, np.zeros(len(qc.CSTAT_NAMES), np.uint64))
    assert {k: int(got[i]) for i, k in enumerate(R.CSTAT_NAMES)} == st
    s.close()
