"""The two loops qb_dev_leader_requests closes, on the device with no
per-group host code between the calls, for three-node groups, one table per
node (node j holds slot j and raft ID j + 1; node 0 leads):

  the linearizable read   requests (queue + heartbeats) -> a tick whose hb_ctx
                          is the newest context -> qb_dev_follower_step at the
                          peers -> qb_dev_leader_step on the acks: the
                          ReadState / MsgReadIndexResp at the queued index;
  the leadership transfer requests (transferee + MsgApp to a lagging peer) ->
                          qb_dev_leader_propose reports the drop ->
                          qb_dev_follower_log_step accepts -> qb_dev_leader_step
                          sends MsgTimeoutNow -> qb_dev_follower_step stops
                          with FFLAG_CAMPAIGN -> qb_dev_campaign (TRANSFER).

Every call is compared bit-exact with its own restatement every round
(tests/request_ref.py, tick_ref.py, follower_ref.py, append_ref.py,
propose_ref.py, campaign_ref.py and oracle/leader_ref.py, all over the same
RequestNodes), and every array of the node's table after it."""
import numpy as np
import pytest
import torch

from etcd_amd.quorum import follower as qf, leader as ql, propose as qp
from oracle import leader_ref as L
from tests import append_pack as AP, append_ref as A, campaign_pack as CP, campaign_ref as CR
from tests import follower_pack, follower_ref as F, propose_pack as P, propose_ref as PR
from tests import request_pack as Q, request_ref as R, tick_ref as T
from tests.test_gpu_requests import DEV, DeviceRun

pytestmark = pytest.mark.gpu
G, TERM = 257, 2                  # a full tile plus one group; the leader's term
ET, HT = 10, 1
FCFG = F.Config(10, True, True)   # as DeviceRun builds its FollowerGroups
CFG = R.Config(R.SAFE, 4, 2)
NO = R.NO_SLOT


class Cluster:
    def __init__(self, logs, lag):
        """logs[g]: the leader's terms of [0 .. last] in group g; node 1's log
        lacks the last lag[g] entries (the leader's Progress says so)."""
        pr = P.progress
        self.nodes = []
        for j in range(3):
            row = []
            for g in range(G):
                terms = logs[g][:len(logs[g]) - lag[g]] if j == 1 else logs[g]
                last, behind = len(logs[g]) - 1, len(logs[g]) - 1 - lag[g]
                prs = None
                if j == 0:
                    p1 = pr(behind, behind + 1, L.STATE_PROBE if g % 2 else L.STATE_REPLICATE, True)
                    if not lag[g]:
                        p1 = pr(last, last + 1, L.STATE_REPLICATE, True)
                    prs = [pr(last, last + 1, L.STATE_REPLICATE, True), p1,
                           pr(last, last + 1, L.STATE_REPLICATE, True)]
                n = Q.make_node(3, 0b111, 0, j, terms=terms, term=TERM, self_id=j + 1,
                                role=R.LEADER if j == 0 else R.FOLLOWER, lead=1,
                                committed=len(terms) - 1, prs=prs, ee=g % 3)
                n.camp.vote = 1
                row.append(n)
            self.nodes.append(row)
        self.runs = [DeviceRun(self.nodes[j], CFG) for j in range(3)]
        z = np.zeros(G, np.uint64)
        self.ps = qp.ProposeState.from_numpy(z, z, z, device=DEV)

    def check(self, j, where, dequeued=False):
        """Node j's arrays against its RequestNodes.  The leader step leaves
        the queue rows it dequeued as they were (rows past the count are
        nobody's): behind it the rows below the count are compared, and the
        rest gets the marker back that the request tests keep there."""
        run = self.runs[j]
        for n in run.nodes:
            n.sync()
        if dequeued:
            a = Q.pack_nodes(run.nodes, CFG.readq_cap)[0]
            live = (np.arange(CFG.readq_cap)[None, :] < ((a["meta"] >> 20) & 0x1F)[:, None]).ravel()
            for k, dt in (("rq_ctx", np.uint64), ("rq_index", np.uint64), ("rq_meta", np.uint32)):
                got = ql._to_np(run.lg.t[k], dt, G * CFG.readq_cap)
                assert np.array_equal(got[live], a[k][live]), (where, k)
                run.lg.t[k].copy_(ql._to_dev(np.where(live, got, a[k]), dt, DEV))
        run.check_state(where)

    # ---- the calls ------------------------------------------------------
    def requests(self, reads, xf_from):
        run = self.runs[0]
        return run.call(Q.inputs(G, CFG.max_reads, reads, xf_from), "requests")

    def tick(self):
        """One tick at the leader; returns hb_ctx where it beat (else None)."""
        run = self.runs[0]
        res = run.lg.tick(run.state, ET, HT, True)
        tf = res.tflags.cpu().numpy()[:G]
        ctx = ql._to_np(res.hb_ctx, np.uint64, G)
        hb = ql._to_np(res.hb_commit, np.uint64, run.lg.S)
        out = []
        for g, n in enumerate(run.nodes):
            c = n.camp
            t = T.TickNode(n.group, c.role, c.election_elapsed, c.heartbeat_elapsed, 0)
            assert T.tick(t, ET, HT, True) == tf[g], g
            c.role, c.election_elapsed, c.heartbeat_elapsed = (t.role, t.election_elapsed,
                                                               t.heartbeat_elapsed)
            for m in t.msgs:
                assert (int(hb[3 * g + m.to]), int(ctx[g])) == (m.commit, m.aux), (g, m)
            out.append(int(ctx[g]) if t.msgs else None)
        self.check(0, "tick")
        return out

    def follower_step(self, j, recs, stops=False):
        """(group, F.Rec) through qb_dev_follower_step at node j; returns
        (resp_type, gflags)."""
        run = self.runs[j]
        fn = [F.Node(n.group.term, n.camp.vote, n.camp.lead, n.group.log.committed, n.prop.last,
                     n.camp.last_term, n.camp.role, n.camp.election_elapsed,
                     n.camp.heartbeat_elapsed) for n in run.nodes]
        rt, rterm, stop, gfl, _ = F.step_batch(fn, recs, FCFG)
        for n, f in zip(run.nodes, fn):
            c = n.camp
            n.group.term, c.vote, c.lead, n.group.log.committed = f.term, f.vote, f.lead, f.committed
            c.role, c.election_elapsed, c.heartbeat_elapsed = (f.role, f.election_elapsed,
                                                               f.heartbeat_elapsed)
        cols = follower_pack.pack_recs(recs)
        ib = qf.FollowerInbox.from_numpy(cols["group"], cols["flags"], cols["from"], cols["term"],
                                         cols["index"], cols["aux"], device=DEV)
        res = qf.follower_step(run.es.follower, ib)
        M = len(recs)
        assert np.array_equal(res.resp_type.cpu().numpy()[:M], np.array(rt, np.uint8))
        assert np.array_equal(ql._to_np(res.resp_term, np.uint64, M), np.array(rterm, np.uint64))
        assert np.array_equal(ql._to_np(res.stop_at, np.uint32, G), np.array(stop, np.uint32))
        assert np.array_equal(res.gflags.cpu().numpy()[:G], np.array(gfl, np.uint8))
        assert stops or all(s == F.NO_STOP for s in stop)
        self.check(j, f"follower step node {j}")
        return rt, gfl

    def follower_log_step(self, j, msgs):
        """The MsgApps (group, index, log_term, commit, n) through
        qb_dev_follower_log_step at node j; returns the leader's inbox records."""
        run, lead = self.runs[j], self.nodes[0]
        recs = [(g, AP.app(1, TERM, idx, lt, [lead[g].prop.log_term(idx + 1 + q) for q in range(k)],
                           commit)) for g, idx, lt, commit, k in msgs]
        lognodes = []
        for n in run.nodes:
            c, g_ = n.camp, n.group
            lognodes.append(A.new_node(n.prop.terms, n.prop.first, term=g_.term, vote=c.vote,
                                       lead=c.lead, committed=g_.log.committed, role=c.role,
                                       election_elapsed=c.election_elapsed,
                                       heartbeat_elapsed=c.heartbeat_elapsed))
        want = A.step_batch(lognodes, recs, FCFG)
        assert want["stats"]["app_truncated"] == 0
        for n, ln in zip(run.nodes, lognodes):
            c, g_ = n.camp, n.group
            n.prop.terms = list(ln.terms)
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
        assert not any(x & F.REJECT for x in want["resp_type"])
        self.check(j, f"follower log step node {j}")
        return [(g, L.Inbound(L.IN_APP_RESP, j, want["resp_term"][i], want["resp_index"][i]))
                for i, (g, _) in enumerate(recs)]

    def leader_step(self, resps):
        """Inbox records through qb_dev_leader_step; returns its messages."""
        run = self.runs[0]
        for n in run.nodes:
            n.sync()
            n.group.msgs = []
        for i, (g, m) in enumerate(resps):
            assert run.nodes[g].group.step(m, i) == "applied"
        for n in run.nodes:       # the step dequeues on the group: readOnly follows it
            n.queue = [r.ctx for r in n.group.readq]
            n.pending = {r.ctx: r for r in n.group.readq}
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
        self.check(0, "leader step", dequeued=True)
        return got

    def propose(self):
        """One entry proposed at every leader, through qb_dev_leader_propose."""
        run = self.runs[0]
        inp = P.inputs([PR.PROP_ENTRIES] * G, [1] * G, [8] * G)
        ib = qp.ProposeInbox.from_numpy(inp["action"], inp["n_ents"], inp["payload"], device=DEV)
        res = qp.leader_propose(run.lg, run.es, self.ps, ib)
        pf, _, _ = P.ref_propose([n.prop for n in run.nodes], inp, PR.Config(), run.off,
                                 P.new_msg(run.lg.S))
        assert np.array_equal(res.pflags.cpu().numpy()[:G], pf)
        self.check(0, "propose")
        return pf

    def campaign(self, j, action):
        run = self.runs[j]
        res = run.lg.campaign(run.es, torch.from_numpy(np.asarray(action, np.uint8)).to(DEV))
        req_term, req_mask = np.zeros(G, np.uint64), np.zeros(G, np.uint16)
        cf, rt, _ = CP.ref_campaign([n.camp for n in run.nodes], action, True, req_term, req_mask)
        assert np.array_equal(res.cflags.cpu().numpy()[:G], cf)
        assert np.array_equal(res.req_type.cpu().numpy()[:G], rt)
        live = rt != 0
        assert np.array_equal(ql._to_np(res.req_term, np.uint64, G)[live], req_term[live])
        assert np.array_equal(ql._to_np(res.req_mask, np.uint16, G)[live], req_mask[live])
        self.check(j, f"campaign node {j}")
        return cf, rt, req_term


def make_logs(rng):
    return [[0] + [1] * int(rng.integers(1, 4)) + [TERM] * int(rng.integers(3, 6)) for _ in range(G)]


def test_read_index_round_trip():
    """A read queued by the requests call is released by the leader step at
    the queued index once a peer's heartbeat response carries its context
    back; every third group's read is a peer's (a MsgReadIndexResp), every
    seventh group reads nothing."""
    rng = np.random.default_rng(11)
    logs = make_logs(rng)
    c = Cluster(logs, [0] * G)
    ctx = [1000 + g for g in range(G)]
    frm = [2 if g % 3 == 0 else NO for g in range(G)]
    reads = [[] if g % 7 == 6 else [(ctx[g], frm[g])] for g in range(G)]
    res = c.requests(reads, None)
    assert all(r.reads == [(R.RD_BCAST, None)] for r, rd in zip(res, reads) if rd)
    queued = [n.group.readq[0].index if rd else None for n, rd in zip(c.nodes[0], reads)]
    assert queued == [len(logs[g]) - 1 if reads[g] else None for g in range(G)]
    # the tick in between carries the newest pending context
    beat = c.tick()
    assert beat == [ctx[g] if reads[g] else 0 for g in range(G)]
    # the broadcast's heartbeats (the request's context) at both peers
    acks = []
    for j in (1, 2):
        recs = [(g, F.Rec(F.HEARTBEAT, 1, TERM, commit, ctx[g]))
                for g, r in enumerate(res) if r.heartbeats for s, commit in r.heartbeats if s == j]
        assert len(recs) == sum(1 for rd in reads if rd)
        rt, _ = c.follower_step(j, recs)
        assert all(x == F.MSG_HEARTBEAT_RESP for x in rt)
        # the host answers with the heartbeat's context (raft.go:1515)
        acks += [(g, L.Inbound(L.IN_HEARTBEAT_RESP, j, TERM, m.aux)) for g, m in recs]
    acks.sort(key=lambda x: x[0])
    msgs = c.leader_step(acks)
    for g in range(G):
        if not reads[g]:
            assert msgs[g] == []
        elif frm[g] == NO:
            assert msgs[g] == [(L.READ_STATE, NO, queued[g], 0, 0, ctx[g])]
        else:
            assert msgs[g] == [(L.MSG_READ_INDEX_RESP, 2, queued[g], 0, 0, ctx[g])]
    assert all(not n.group.readq for n in c.nodes[0])
    assert c.tick() == [0] * G      # the queue is empty again: no context


def test_leader_transfer_round_trip():
    """A transfer to a lagging peer: the MsgApp of the requests call catches
    it up, the leader step's MsgTimeoutNow stops the follower step with
    FFLAG_CAMPAIGN, and the campaign runs with CAMP_TRANSFER; a proposal at
    the old leader in between is dropped."""
    rng = np.random.default_rng(12)
    logs = make_logs(rng)
    lag = [1 + g % 2 for g in range(G)]
    c = Cluster(logs, lag)
    res = c.requests([[] for _ in range(G)], [1] * G)
    apps = []
    for g, r in enumerate(res):
        t, idx, lt, k = r.xf
        assert r.qflags == R.QFLAG_TRANSFER_STARTED and (t, k) == (R.MSG_APP, lag[g]), (g, r)
        apps.append((g, idx, lt, c.nodes[0][g].group.log.committed, k))
    assert all(n.group.transferee == 1 and n.camp.election_elapsed == 0 for n in c.nodes[0])
    pf = c.propose()
    assert (pf == PR.PFLAG_DROPPED).all()
    resps = c.follower_log_step(1, apps)
    msgs = c.leader_step(resps)
    for g, m in enumerate(msgs):   # (a probe that was paused gets an empty MsgApp first)
        assert m[-1] == (L.MSG_TIMEOUT_NOW, 1, 0, 0, 0, 0), (g, m)
        assert all(x[:2] == (L.MSG_APP, 1) and x[5] == 0 for x in m[:-1]), (g, m)
    rt, gfl = c.follower_step(1, [(g, F.Rec(F.TIMEOUT_NOW, 1, TERM)) for g in range(G)], stops=True)
    assert all(x & F.FFLAG_CAMPAIGN for x in gfl) and not any(rt)
    cf, req, req_term = c.campaign(1, np.full(G, CR.CAMP_TRANSFER, np.uint8))
    assert (req == (CR.MSG_VOTE | CR.CREQ_TRANSFER)).all() and (req_term == TERM + 1).all()
    assert all((n.camp.role & 3) == R.CANDIDATE for n in c.nodes[1])
