"""qb_dev_leader_propose on the device against tests/propose_ref.py, bit-exact
after every call: every array of the table, of the election state and of the
propose state (so nothing a proposal does not own can have moved — run rows
past the count, slots of idle groups and the gaps of a gapped table keep
their bytes), pflags, and msg_type / msg_index / msg_log_term / msg_n including
the elements a call must leave untouched (pre-filled with 0xA5...), and the
accumulated stats.  All comparisons are integer equality."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from etcd_amd import _lib
from etcd_amd.quorum import leader as ql, propose as qp, tick as qt
from oracle import leader_ref as L
from tests import propose_pack as P, propose_ref as R

qc = importlib.import_module("etcd_amd.quorum.campaign")

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL_I64 = P.FILL - (1 << 64)
MSG_KEYS = ("msg_type", "msg_index", "msg_log_term", "msg_n")


class DeviceRun:
    """A batch of ProposeNodes on the device beside its reference copy."""

    def __init__(self, nodes, cfg=None, cap=P.INFLIGHT_CAP):
        self.nodes, self.cfg, self.cap = nodes, cfg or R.Config(), cap
        a, e, p = P.pack_nodes(nodes, cap)
        self.lg = ql.LeaderGroups(self.layout(a), cap, 0, device=DEV)
        G, S = self.lg.G, self.lg.S
        self.off = self.lg.numpy()["off"]
        self.state = qt.TickState.from_numpy(e["role"], e["election_elapsed"],
                                             e["heartbeat_elapsed"], np.zeros(G, np.uint32),
                                             device=DEV)
        self.es = qc.ElectionState.for_table(self.lg, self.state, e["self_id"], e["vote"],
                                             e["lead"], e["last_term"], 10, True, True,
                                             votes=e["votes"])
        self.ps = qp.ProposeState.from_numpy(p["applied"], p["uncommitted_size"],
                                             p["pending_conf_index"], device=DEV)
        n, s = max(G, 1), max(S, 1)
        self.out = qp.ProposeResult(
            torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV),
            torch.full((s,), 0xA5, dtype=torch.uint8, device=DEV),
            *[torch.full((s,), FILL_I64, dtype=torch.int64, device=DEV) for _ in range(3)],
            torch.zeros(len(qp.PSTAT_NAMES), dtype=torch.int64, device=DEV))
        self.msg = P.new_msg(S)
        self.stats = R.new_stats()

    def layout(self, a):
        """The table as the device holds it (the dense one here)."""
        return a

    def check_state(self, where):
        G = self.lg.G
        a, e, p = P.pack_nodes(self.nodes, self.cap)
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
        gp = self.ps.numpy(G)
        for key, w in p.items():
            assert np.array_equal(gp[key], w), (where, key, np.flatnonzero(gp[key] != w)[:8])

    def propose(self, inp, where):
        G, S = self.lg.G, self.lg.S
        ib = qp.ProposeInbox.from_numpy(inp["action"], inp["n_ents"], inp["payload"], inp["cc_at"],
                                        inp["cc_payload"], device=DEV)
        res = qp.leader_propose(
            self.lg, self.es, self.ps, ib, max_uncommitted_size=self.cfg.max_uncommitted_size,
            disable_proposal_forwarding=self.cfg.disable_proposal_forwarding, out=self.out)
        assert res is self.out
        pf, st, sent = P.ref_propose(self.nodes, inp, self.cfg, self.off, self.msg)
        for k, v in st.items():
            self.stats[k] += v
        self.check_state(where)
        got_pf = res.pflags.cpu().numpy()[:G]
        assert np.array_equal(got_pf, pf), (where, "pflags", np.flatnonzero(got_pf != pf)[:8],
                                            got_pf[got_pf != pf][:8], pf[got_pf != pf][:8])
        for key in MSG_KEYS:
            got = ql._to_np(getattr(res, key), self.msg[key].dtype, S)
            assert np.array_equal(got, self.msg[key]), (where, key,
                                                        np.flatnonzero(got != self.msg[key])[:8])
        assert res.stats_dict() == self.stats, (where, res.stats_dict(), self.stats)
        self.sent = sent
        return pf

    def messages_match(self, g):
        got = self.out.messages(g)
        assert got == self.sent[g], (g, got, self.sent[g])
        return got


# --------------------------------------------------------- golden scenarios ---

SCENARIOS = P.load_tables()["scenarios"]


@pytest.mark.parametrize("sc", SCENARIOS, ids=[s["name"] for s in SCENARIOS])
def test_golden_scenarios_on_device(sc):
    """The reference's tests, G = 1 each, through the device: the transcribed
    expectations hold for the device's outputs, and the device equals
    propose_ref after every call.  (A step that repeats hundreds of times runs
    its first two and last two calls on the device and the ones between on the
    restatement alone, whose state is then uploaded again.)"""
    cap = sc["node"]["inflight_cap"]
    run = None

    def apply(n, cfg, inp, k, repeat):
        nonlocal run
        if 2 <= k < repeat - 2:
            run = None
            return R.step(n, *inp, cfg, R.new_stats())
        if k == 0 or run is None:    # (the scenario may have set node fields between steps)
            run = DeviceRun([n], cfg, cap)
        pf = run.propose(P.inputs(*[[x] for x in inp]), sc["name"])
        return int(pf[0]), run.messages_match(0)
    P.replay(sc, apply)


# --------------------------------------------------------------------- fuzz ---

@pytest.mark.parametrize("slots", [None, (1,), (3,), (16,)], ids=["ragged", "n1", "n3", "n16"])
@pytest.mark.parametrize("G", [1, 255, 256, 257, 513])
def test_fuzz_two_calls(G, slots):
    """Seeded batches (propose_pack.random_nodes: learners, joint halves,
    every role, logs of 1..8 runs, every Progress state, rings empty to full)
    through two calls into the same outputs at the tile edges: the second
    acts on what the first left, and the stats accumulate."""
    rng = np.random.default_rng(1000 * G + (slots[0] if slots else 0))
    run = DeviceRun(P.random_nodes(rng, G, slots), R.Config(max_uncommitted_size=100))
    for k in range(2):
        run.propose(P.random_inputs(rng, G), f"G{G} {slots} call {k}")
        for g in (0, G // 2, G - 1):
            run.messages_match(g)
    if G >= 255 and slots != (1,):  # the main branches were reached
        for k in ("proposals", "entries", "drop_size", "drop_candidate", "forwarded", "cc_accepted",
                  "cc_refused", "msg_app", "leader_entries", "bad_action"):
            assert run.stats[k] > 0, (k, run.stats)


def test_idle_tile_next_to_a_one_actor_tile():
    """Three tiles: seeded proposals, no action at all, and exactly one group
    that proposes among 255 idle ones; then a call with nothing to do."""
    rng = np.random.default_rng(31)
    nodes = P.random_nodes(rng, 768)
    inp = P.random_inputs(rng, 768)
    inp["action"][256:] = R.PROP_NONE
    nodes[600] = P.make_node(3, 0b111, 0, 1, terms=[2, 2, 2], term=2)
    inp["action"][600], inp["n_ents"][600] = R.PROP_ENTRIES, 2
    run = DeviceRun(nodes)
    pf = run.propose(inp, "skip paths")
    assert not pf[256:600].any() and not pf[601:].any()
    assert pf[600] == R.PFLAG_APPENDED | R.PFLAG_BCAST
    assert [m[:2] for m in run.messages_match(600)] == [(R.MSG_APP, 0), (R.MSG_APP, 2)]
    inp["action"][:] = R.PROP_NONE
    assert not run.propose(inp, "all idle").any()


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
    slots, wider than its LDS stage, so the slot phase runs from the global
    arrays.  Every group declares 20 slots, read as 16; the four slots past
    each group keep their sentinels, in the table and in the messages."""
    rng = np.random.default_rng(20)
    run = GappedRun(P.random_nodes(rng, 300, (16,)), 20, cfg=R.Config(max_uncommitted_size=100))
    run.propose(P.random_inputs(rng, 300, p_none=0.1), "gapped")
    assert run.stats["msg_app"] and run.stats["proposals"]
    run.propose(P.random_inputs(rng, 300, p_none=0.1), "gapped, second call")


# -------------------------------------------------------------------- edges ---

REPL, PROBE, SNAP = L.STATE_REPLICATE, L.STATE_PROBE, L.STATE_SNAPSHOT
ENT, LENT = R.PROP_ENTRIES, R.PROP_LEADER_ENTRY
CC, LEAVE = R.PROP_CONF_CHANGE, R.PROP_CC_LEAVE_JOINT
LIMIT = 100


def edge_cases(cap=P.INFLIGHT_CAP):
    """(name, node, (action, n_ents, payload, cc_at, cc_payload), expected
    pflags or None) under max_uncommitted_size = LIMIT."""
    mk, pr = P.make_node, P.progress
    t5 = [1, 1, 2, 2, 3, 3]                    # indexes 0..5, last = 5
    out = []

    def add(name, node, act, n=1, pay=0, at=0, ccp=0, want=None):
        out.append((name, node, (act, n, pay, at, ccp), want))

    def three(own_match, peers):
        """Progress of a 3-slot group whose own slot is 1."""
        return [peers[0], pr(own_match, own_match + 1, REPL, True, cap=cap), peers[1]]

    def leader(prs=None, **kw):
        """Three voters, own slot 1, everything committed."""
        kw.setdefault("terms", t5)
        kw.setdefault("term", 3)
        kw.setdefault("committed", kw.get("first", 1) - 1 + len(kw["terms"]) - 1)
        return mk(3, 0b111, 0, 1, prs=prs, cap=cap, **kw)
    ok = R.PFLAG_APPENDED | R.PFLAG_BCAST
    # Inflights
    full = tuple(range(6, 6 + cap))
    add("ring full: paused, no message",
        leader(three(5, [pr(3, 6 + cap, REPL, True, ring=full, cap=cap), pr(5, 6, REPL, True, cap=cap)])),
        ENT, 2, want=ok)
    add("ring start at cap - 1: the add wraps",
        leader(three(5, [pr(3, 6, REPL, True, ring=(5,) if cap > 1 else (), start=cap - 1, cap=cap),
                         pr(5, 6, REPL, True, start=cap - 1, cap=cap)])), ENT, 3, want=ok)
    add("max_ents 1", leader(three(5, [pr(2, 3, REPL, True, cap=cap), pr(0, 4, PROBE, True, cap=cap)]),
                             max_ents=1), ENT, 4, want=ok)
    # snapshot fallback: first_index 4, peers at next 2
    cterms = [2, 2, 3]                          # indexes 3..5
    for name, active, snap in (("RecentActive on", True, None), ("RecentActive off", False, None),
                               ("snap_index 0", True, 0)):
        add(f"next < first_index, {name}",
            leader(three(5, [pr(1, 2, PROBE, active, cap=cap), pr(1, 2, REPL, active, cap=cap)]),
                   terms=cterms, first=4, snap_index=snap, snap_term=2, committed=3), ENT, 1, want=ok)
    add("next - 1 inside an older run: the table walk",
        leader(three(5, [pr(1, 2, PROBE, True, cap=cap), pr(2, 4, REPL, True, cap=cap)])), ENT, 2,
        want=ok)
    add("next - 1 inside an older run, a new term on top",
        leader(three(5, [pr(1, 2, PROBE, True, cap=cap), pr(2, 4, REPL, True, cap=cap)]), term=4),
        ENT, 2, want=ok)
    # run table
    t8 = [1, 2, 3, 4, 5, 6, 7, 8]
    add("8 runs, a new term: LOG_RUNS", leader(terms=t8, term=9), ENT, 1, want=R.PFLAG_LOG_RUNS)
    add("8 runs, a new term, leader entry: LOG_RUNS", leader(terms=t8, term=9), LENT,
        want=R.PFLAG_LOG_RUNS)
    add("8 runs, the same term", leader(terms=t8, term=8), ENT, 1, want=ok)
    add("7 runs, a new term: the run is added", leader(terms=t8[:7], term=9), ENT, 2, want=ok)
    add("7 runs, a new term, leader entry", leader(terms=t8[:7], term=9), LENT,
        want=R.PFLAG_APPENDED)
    # size limit
    add("uncommitted_size exactly at the limit", leader(unc=90), ENT, 1, 10, want=ok)
    add("uncommitted_size one past the limit", leader(unc=90), ENT, 1, 11, want=R.PFLAG_DROPPED)
    add("over the limit with s == 0", leader(unc=LIMIT + 5), ENT, 3, 0, want=ok)
    add("uncommitted_size 0 takes any size", leader(unc=0), ENT, 1, 10 ** 6, want=ok)
    add("uncommitted_size + s wraps", leader(unc=(1 << 64) - 5), ENT, 1, 10, want=ok)
    # the conf-change rule
    for joint in (0, 0b011):
        for leave in (0, LEAVE):
            for d in (0, 1):
                refused = bool(d) or bool(joint) != bool(leave)
                add(f"conf change: joint={bool(joint)} leave={bool(leave)} pending at applied+{d}",
                    mk(3, 0b111, joint, 1, terms=t5, term=3, cap=cap, applied=4, pci=4 + d,
                       committed=5),
                    ENT | CC | leave, 3, 30, 1, 20, want=ok | (R.PFLAG_CC_REFUSED if refused else 0))
    add("conf change at cc_at >= n_ents reads as clear", leader(applied=4, pci=9), ENT | CC, 2, 5, 2, 5,
        want=ok)
    add("conf change refused, then dropped for size", leader(applied=4, pci=5, unc=95),
        ENT | CC, 2, 30, 0, 20, want=R.PFLAG_CC_REFUSED | R.PFLAG_DROPPED)
    add("conf change refused, the rest fits", leader(applied=4, pci=5, unc=95), ENT | CC, 2, 25, 0, 20,
        want=ok | R.PFLAG_CC_REFUSED)
    add("conf change accepted, then dropped for size", leader(applied=4, pci=4, unc=95),
        ENT | CC, 2, 30, 1, 20, want=R.PFLAG_DROPPED)
    # drops and ignores
    add("transferee set", leader(transferee=2), ENT, 1, want=R.PFLAG_DROPPED)
    add("transferee set, leader entry", leader(transferee=2), LENT, want=R.PFLAG_APPENDED)
    add("own slot == slot count", mk(3, 0b111, 0, 3, terms=t5, term=3, cap=cap), ENT, 1,
        want=R.PFLAG_DROPPED)
    add("own slot 0xFF", mk(3, 0b111, 0, 0xFF, terms=t5, term=3, cap=cap), ENT, 1,
        want=R.PFLAG_DROPPED)
    add("n_ents 0", leader(), ENT, 0, want=R.PFLAG_BAD)
    add("n_ents 0, transferee set", leader(transferee=0), ENT, 0, want=R.PFLAG_BAD)
    for role in (R.FOLLOWER, R.CANDIDATE, R.LEADER, R.PRE_CANDIDATE):
        for lead in (0, 7):
            for act in (R.PROP_NONE, ENT, LENT, 3, 0x3F):
                add(f"role {role} lead {lead} action {act}", leader(role=role, lead=lead), act, 1, 5)
    add("single voter commits at once", mk(3, 0b010, 0, 1, terms=t5, term=3, cap=cap), ENT, 2,
        want=ok | R.PFLAG_COMMITTED)
    add("single voter, a new term on top",
        mk(1, 1, 0, 0, terms=t5, term=4, cap=cap, committed=3), ENT, 1, want=ok | R.PFLAG_COMMITTED)
    # last_index + n_ents across 2^64 - 1
    add("last_index + n_ents wraps", leader(terms=[3] * 5, first=(1 << 64) - 9, committed=(1 << 64) - 8),
        ENT, 10, want=ok)
    return out


def run_edges(cases, cfg, cap=P.INFLIGHT_CAP):
    """(the expected pflags are those under max_uncommitted_size = LIMIT with
    forwarding on, and are checked under that configuration only)"""
    nodes = [copy.deepcopy(c[1]) for c in cases]
    cols = list(zip(*[c[2] for c in cases]))
    run = DeviceRun(nodes, cfg, cap)
    pf = run.propose(P.inputs(*cols), "edges")
    for i, (name, _, _, want) in enumerate(cases):
        if want is not None and cfg == R.Config(LIMIT):
            assert int(pf[i]) == want, (name, hex(int(pf[i])), hex(want))
        run.messages_match(i)
    return run, pf, {c[0]: i for i, c in enumerate(cases)}


def test_edges():
    cases = edge_cases()
    run, pf, by = run_edges(cases, R.Config(max_uncommitted_size=LIMIT))
    n = run.nodes
    sent = run.sent
    assert [m[1] for m in sent[by["ring full: paused, no message"]]] == [2]
    g = by["ring start at cap - 1: the add wraps"]
    assert n[g].group.prs[0].inflights.fifo() == [5, 8] and n[g].group.prs[2].inflights.start == 1
    assert [(m[0], m[5]) for m in sent[by["max_ents 1"]]] == [(R.MSG_APP, 1), (R.MSG_APP, 1)]
    assert [m[0] for m in sent[by["next < first_index, RecentActive on"]]] == [R.MSG_SNAP] * 2
    assert sent[by["next < first_index, RecentActive off"]] == []
    assert sent[by["next < first_index, snap_index 0"]] == []
    assert [m[3] for m in sent[by["next - 1 inside an older run: the table walk"]]] == [1, 2]
    g = by["7 runs, a new term: the run is added"]
    assert n[g].group.log.runs[-1] == (7, 9) and len(n[g].group.log.runs) == 8
    g = by["8 runs, a new term: LOG_RUNS"]
    assert n[g].group.log.last == 7 and n[g].camp.last_term == 8
    assert n[by["uncommitted_size + s wraps"]].uncommitted_size == 5
    assert n[by["conf change refused, then dropped for size"]].pending_conf_index == 5
    assert n[by["conf change accepted, then dropped for size"]].pending_conf_index == 7
    assert n[by["conf change: joint=False leave=False pending at applied+0"]].pending_conf_index == 7
    g = by["last_index + n_ents wraps"]
    assert n[g].group.log.last == 4 and n[g].group.prs[1].match == (1 << 64) - 6
    for k in ("drop_no_progress", "drop_transfer", "drop_size", "drop_no_leader", "drop_candidate",
              "forwarded", "cc_accepted", "cc_refused", "msg_app", "msg_snap", "commits",
              "leader_entries", "log_runs", "empty", "ignored_role", "bad_action"):
        assert run.stats[k] > 0, k
    # a second round of plain proposals on what the first left
    G = len(cases)
    run.propose(P.inputs([ENT] * G, [2] * G, [1] * G), "edges: second call")


def test_edges_without_a_size_limit_and_without_forwarding():
    """max_uncommitted_size 0 is no limit; disable_proposal_forwarding drops
    at a follower that knows its leader."""
    cases = edge_cases()
    run, pf, by = run_edges(cases, R.Config(0, True))
    assert int(pf[by["uncommitted_size one past the limit"]]) & R.PFLAG_APPENDED
    assert int(pf[by["role 0 lead 7 action 1"]]) == R.PFLAG_DROPPED
    assert run.stats["drop_forwarding"] > 0 and run.stats["forwarded"] == 0
    assert run.stats["drop_size"] == 0


@pytest.mark.parametrize("cap", [1, 2])
def test_inflight_cap(cap):
    """inflight_cap 1 and 2: a ring that fills with this proposal, then is
    full (paused) for the next."""
    cases = [c for c in edge_cases(cap) if c[0].startswith(("ring", "max_ents", "next"))]
    run, pf, by = run_edges(cases, R.Config(), cap)
    G = len(cases)
    for k in range(2):
        run.propose(P.inputs([ENT] * G, [1] * G), f"cap {cap}: call {k + 2}")
    g = by["ring start at cap - 1: the add wraps"]
    assert all(p.inflights.full() for s, p in enumerate(run.nodes[g].group.prs) if s != 1)
    assert run.sent[g] == []


# ------------------------------------------------------------------ raw ABI ---

def test_propose_raw_abi():
    """One call through plain ctypes with the library's own stream, memory and
    copies (no torch), as a cgo embedder makes it."""
    from tests.test_gpu_abi_raw import Stream
    rng = np.random.default_rng(78)
    G = 600
    nodes = P.random_nodes(rng, G)
    inp = P.random_inputs(rng, G)
    a, e, p = P.pack_nodes(nodes)
    S = int(a["off"][-1])
    s = Stream()
    keys_a = ("off", "cfg", "term", "first_index", "snap_index", "snap_term", "max_ents", "meta",
              "committed", "last_index", "run_start", "run_term", "match", "next",
              "pending_snapshot", "pstate", "infl_pos", "infl_buf")
    keys_e = ("role", "lead", "last_term")
    d = {k: s.up(a[k]) for k in keys_a}
    d.update({k: s.up(e[k]) for k in keys_e})
    d.update({k: s.up(v) for k, v in p.items()})
    pg = qp.ProposeGroupsC(G=G, inflight_cap=P.INFLIGHT_CAP, disable_proposal_forwarding=0,
                           max_uncommitted_size=100, **d)
    d_in = {k: s.up(v) for k, v in inp.items()}
    msg = P.new_msg(S)
    d_out = {k: s.zeros(v.nbytes, 0xA5) for k, v in msg.items()}
    d_out["pflags"] = s.zeros(G, 0xA5)
    d_st = s.zeros(8 * len(qp.PSTAT_NAMES))
    pin, pout = qp.ProposeInC(**d_in), qp.ProposeOutC(**d_out)
    _lib.check(s.lib.qb_dev_leader_propose(C.byref(pg), C.byref(pin), C.byref(pout), d_st, s.st),
               "propose")
    pf, st, _ = P.ref_propose(nodes, inp, R.Config(max_uncommitted_size=100), a["off"], msg)
    want_a, want_e, want_p = P.pack_nodes(nodes)
    assert np.array_equal(s.down(d_out["pflags"], pf), pf)
    for k, v in msg.items():
        assert np.array_equal(s.down(d_out[k], v), v), k
    for k, v in inp.items():
        assert np.array_equal(s.down(d_in[k], v), v), k
    for k in keys_a:
        assert np.array_equal(s.down(d[k], want_a[k]), want_a[k]), k
    for k in keys_e:
        assert np.array_equal(s.down(d[k], want_e[k]), want_e[k]), k
    for k in want_p:
        assert np.array_equal(s.down(d[k], want_p[k]), want_p[k]), k
    got = s.down(d_st, np.zeros(len(qp.PSTAT_NAMES), np.uint64))
    assert {k: int(got[i]) for i, k in enumerate(R.PSTAT_NAMES)} == st
    s.close()
