"""The write path on the device with no per-group host code between the calls:
qb_dev_campaign (WON) -> qb_dev_leader_propose (LEADER_ENTRY, ENTRIES) ->
qb_dev_follower_log_step at the peers -> qb_dev_leader_step on the responses
-> commit, for three-node groups, one table per node.  Every call is compared
bit-exact with its own restatement every round: tests/campaign_ref.py,
tests/propose_ref.py, tests/append_ref.py and oracle/leader_ref.py, all over
the same ProposeNodes."""
import importlib

import numpy as np
import pytest
import torch

from etcd_amd.quorum import follower as qf, leader as ql
from oracle import leader_ref as L
from tests import append_pack as AP, append_ref as A, campaign_ref as CR, follower_ref as F
from tests import propose_pack as P, propose_ref as R
from tests.test_gpu_propose import DEV, DeviceRun

qc = importlib.import_module("etcd_amd.quorum.campaign")

pytestmark = pytest.mark.gpu
G, T = 24, 3                      # groups, the election's term
FCFG = F.Config(10, True, True)   # as DeviceRun builds its FollowerGroups


class Cluster:
    """G groups x 3 nodes; node j holds slot j (raft ID j + 1) of every group.
    Node 0 is a candidate that has its quorum of votes; the others follow."""

    def __init__(self, logs):
        """logs[j][g]: node j's terms of [0 .. last] in group g."""
        self.nodes = []
        for j in range(3):
            row = []
            for g in range(G):
                n = P.make_node(3, 0b111, 0, j, terms=logs[j][g], term=T, self_id=j + 1,
                                role=R.CANDIDATE if j == 0 else R.FOLLOWER, committed=1)
                n.camp.vote = 1
                if j == 0:
                    n.camp.votes = {0: True, 1: True}
                row.append(n)
            self.nodes.append(row)
        self.runs = [DeviceRun(self.nodes[j]) for j in range(3)]

    def check(self, j, where, loose_runs=False):
        """Node j's arrays against its ProposeNodes.  A truncation at a
        follower leaves the dropped run rows as they were (the follower log
        step's contract): there only the rows below the count are compared."""
        run = self.runs[j]
        self.loose = getattr(self, "loose", set()) | ({j} if loose_runs else set())
        if j not in self.loose:
            return run.check_state(where)
        keep = {k: run.lg.t[k].clone() for k in ("run_start", "run_term")}
        a = P.pack_nodes(run.nodes)[0]
        live = (np.arange(8)[:, None] < ((a["meta"] >> 16) & 0xF)[None, :]).ravel()
        for k in keep:
            got = ql._to_np(run.lg.t[k], np.uint64, 8 * G)
            assert np.array_equal(got[live], a[k][live]), (where, k)
            run.lg.t[k].copy_(ql._to_dev(np.where(live, got, a[k]), np.uint64, DEV))
        run.check_state(where)
        for k, v in keep.items():
            run.lg.t[k].copy_(v)

    # ---- the four calls -------------------------------------------------
    def campaign_won(self):
        run = self.runs[0]
        res = run.lg.campaign(run.es, torch.full((G,), CR.CAMP_WON, dtype=torch.uint8, device=DEV))
        cf = np.array([CR.step(n.camp, CR.CAMP_WON, True, CR.new_stats()) for n in run.nodes],
                      np.uint8)
        assert np.array_equal(res.cflags.cpu().numpy()[:G], cf)
        assert (cf & CR.CFLAG_BCAST_APPEND).all()
        self.check(0, "campaign")
        # the host's share of QB_CFLAG_BCAST_APPEND: the probe
        # with the empty entry, formed from the log as it stood at entry
        return [[(R.MSG_APP, s, n.last, n.terms[-1], n.group.log.committed, 1) for s in (1, 2)]
                for n in run.nodes]

    def propose(self, action, n_ents=1, payload=8):
        run = self.runs[0]
        pf = run.propose(P.inputs([action] * G, [n_ents] * G, [payload] * G), f"propose {action}")
        return pf, [list(m) for m in run.sent]

    def follower_step(self, j, msgs):
        """The MsgApps addressed to slot j through qb_dev_follower_log_step."""
        run, lead = self.runs[j], self.nodes[0]
        recs = []
        for g in range(G):
            for t, to, idx, lt, commit, k in msgs[g]:
                assert t == R.MSG_APP
                if to == j:
                    ents = [lead[g].log_term(idx + 1 + q) for q in range(k)]
                    recs.append((g, AP.app(1, T, idx, lt, ents, commit)))
        if not recs:
            return []
        lognodes = []
        for n in run.nodes:
            c, g_ = n.camp, n.group
            lognodes.append(A.new_node(n.terms, n.first, term=g_.term, vote=c.vote, lead=c.lead,
                                       committed=g_.log.committed, role=c.role,
                                       election_elapsed=c.election_elapsed,
                                       heartbeat_elapsed=c.heartbeat_elapsed))
        want = A.step_batch(lognodes, recs, FCFG)
        truncated = want["stats"]["app_truncated"] > 0
        for n, ln in zip(run.nodes, lognodes):
            c, g_ = n.camp, n.group
            n.terms = list(ln.terms)
            g_.term, c.vote, c.lead, c.role = ln.term, ln.vote, ln.lead, ln.role
            g_.log.committed = ln.committed
            c.election_elapsed, c.heartbeat_elapsed = ln.election_elapsed, ln.heartbeat_elapsed
            n.sync()
        r, ap = AP.pack_recs(recs)
        ib = qf.FollowerInbox.from_numpy(r["group"], r["flags"], r["from"], r["term"], r["index"],
                                         r["aux"], device=DEV)
        app = qf.FollowerAppInbox.from_numpy(ap["commit"], ap["ent_off"], ap["ent_term"],
                                             ap["ent_len"], device=DEV)
        t = run.lg.t
        flog = qf.FollowerLog(G, t["meta"], t["first_index"], t["run_start"], t["run_term"])
        res = qf.follower_log_step(run.es.follower, flog, ib, app)
        M = len(recs)
        assert np.array_equal(res.resp_type.cpu().numpy()[:M], np.array(want["resp_type"], np.uint8))
        for key in ("resp_term", "resp_index", "app_from"):
            assert np.array_equal(ql._to_np(getattr(res, key), np.uint64, M),
                                  np.array(want[key], np.uint64)), key
        assert (ql._to_np(res.stop_at, np.uint32, G) == F.NO_STOP).all()
        assert np.array_equal(res.gflags.cpu().numpy()[:G], np.array(want["gflags"], np.uint8))
        hint = ql._to_np(res.resp_hint, np.uint64, M)
        lterm = ql._to_np(res.resp_log_term, np.uint64, M)
        out = []
        for i, (g, _) in enumerate(recs):
            rej = bool(want["resp_type"][i] & F.REJECT)
            if rej:
                assert (int(hint[i]), int(lterm[i])) == (want["resp_hint"][i], want["resp_log_term"][i])
            out.append((g, L.Inbound(L.IN_APP_RESP, j, want["resp_term"][i], want["resp_index"][i],
                                     rej, want["resp_hint"][i] or 0, want["resp_log_term"][i] or 0)))
        self.check(j, f"follower log step node {j}", loose_runs=truncated)
        return out

    def leader_step(self, resps):
        """The MsgAppResps through qb_dev_leader_step; returns its messages."""
        run = self.runs[0]
        for n in run.nodes:
            n.sync()
            n.group.msgs = []
        for i, (g, m) in enumerate(resps):
            assert run.nodes[g].group.step(m, i) == "applied"
        ib = ql.LeaderInbox.from_numpy(
            [g for g, _ in resps], [m.slot for _, m in resps], [m.kind for _, m in resps],
            np.array([m.index for _, m in resps], np.uint64),
            np.array([m.term for _, m in resps], np.uint64), [m.reject for _, m in resps],
            np.array([m.hint for _, m in resps], np.uint64),
            np.array([m.log_term for _, m in resps], np.uint64), device=DEV)
        res = run.lg.step(ib)
        want = [[m.key() for m in n.group.msgs] for n in run.nodes]
        got = [[] for _ in range(G)]
        for m in res.msgs:
            got[int(m["group"])].append((int(m["type"]), int(m["to"]), int(m["index"]),
                                         int(m["log_term"]), int(m["commit"]), int(m["aux"])))
        assert got == want
        assert res.stats["applied"] == len(resps)
        self.check(0, "leader step")
        return got

    def deliver(self, msgs):
        """Messages -> followers -> responses -> leader -> its messages."""
        resps = self.follower_step(1, msgs) + self.follower_step(2, msgs)
        resps.sort(key=lambda x: x[0])   # (group order; a group's responses keep theirs)
        return self.leader_step(resps) if resps else [[] for _ in range(G)]

    def settled(self):
        for g in range(G):
            last = self.nodes[0][g].last
            for j in range(3):
                n = self.nodes[j][g]
                assert (n.last, n.group.log.committed) == (last, last), (g, j)
                assert n.terms == self.nodes[0][g].terms
        for j in range(3):
            a = self.runs[j].lg.numpy()
            assert np.array_equal(a["committed"], a["last_index"])


def shared_logs(rng):
    return [[1] * int(rng.integers(1, 4)) + [2] * int(rng.integers(1, 4)) for _ in range(G)]


def run_loop(c, second_proposal_after):
    msgs = c.campaign_won()
    pf, none = c.propose(R.PROP_LEADER_ENTRY)
    assert (pf == R.PFLAG_APPENDED).all() and not any(none)
    a = c.runs[0].lg.numpy()
    assert np.array_equal(a["match"][0::3], a["last_index"])       # match[own] == last_index
    pf, sent = c.propose(R.PROP_ENTRIES, 3, 24)
    assert (pf == R.PFLAG_APPENDED | R.PFLAG_BCAST).all()
    assert not any(sent)                     # every peer's probe is in flight: paused
    for rnd in range(12):
        msgs = c.deliver(msgs)
        if rnd == second_proposal_after:     # a proposal arrives while the followers catch up
            pf, sent = c.propose(R.PROP_ENTRIES, 2, 16)
            assert (pf & R.PFLAG_APPENDED).all()
            msgs = [m + s for m, s in zip(msgs, sent)]
        if not any(msgs):
            break
    assert rnd > second_proposal_after and not any(msgs)
    c.settled()


def test_campaign_propose_append_ack_commit():
    """Three nodes with the same log: the probe, the catch-up, a second
    proposal that goes out as MsgApps of its own, and the commit everywhere."""
    rng = np.random.default_rng(5)
    logs = [[0] + x for x in shared_logs(rng)]
    c = Cluster([logs, logs, logs])
    run_loop(c, second_proposal_after=0)
    st = c.runs[0].stats
    assert st["msg_app"] > 0 and st["leader_entries"] == G and st["proposals"] == 2 * G


def test_a_divergent_follower_is_probed_and_converges():
    """Node 2 holds an uncommitted tail of term 1 the leader never had: it
    rejects the probe, is probed downwards (findConflictByTerm on both sides),
    overwrites its tail and converges, with a proposal arriving in between."""
    rng = np.random.default_rng(6)
    logs = [[0] + x for x in shared_logs(rng)]
    tail = [[0] + [1] * (len([t for t in x if t == 1]) + int(rng.integers(1, 4))) for x in logs]
    c = Cluster([logs, logs, tail])
    run_loop(c, second_proposal_after=1)
