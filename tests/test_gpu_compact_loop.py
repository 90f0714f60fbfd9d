"""The loop qb_dev_log_compact closes, on the device over one set of buffers
with no per-group host code between the calls, for 257 three-node groups
(tests/test_gpu_requests_loop.py's Cluster: node 0 leads at term 8, node 1 is
far behind and probing, node 2 follows).  Every log holds eight runs — the
dummy entry and terms 1..7 — so the first entry of the leader's own term is a
ninth:

  qb_dev_leader_propose              refused with QB_PFLAG_LOG_RUNS
  qb_dev_log_compact at the leader   (trigger mode) past node 1's next
  qb_dev_leader_propose              accepted; node 2 gets a MsgApp, node 1 is paused
  qb_dev_follower_log_step at node 2 stops with QB_FFLAG_LOG_RUNS
  qb_dev_log_compact at node 2       (trigger mode)
  qb_dev_follower_log_step           the same records again: accepted
  qb_dev_leader_step                 node 2's MsgAppResp commits the entry and
                                     the commit goes out to it as a MsgApp; node
                                     1's heartbeat response (even groups) or
                                     rejected MsgAppResp (odd groups) gets a
                                     QB_MSG_SNAP with the new snap_index /
                                     snap_term

Each stage is compared bit-exact with its own restatement (propose_ref.py,
compact_ref.py, append_ref.py, oracle/leader_ref.py over the same nodes), and
every array of the node's table after it."""
import numpy as np
import pytest
import torch

from etcd_amd.quorum import compact as qcm, follower as qf, leader as ql, propose as qp
from etcd_amd.quorum.ready import ReadyState
from oracle import leader_ref as L
from tests import append_pack as AP, append_ref as A, compact_dev as D, compact_pack as CP
from tests import compact_ref as C, follower_ref as F, propose_pack as P, propose_ref as PR
from tests import request_pack as Q, request_ref as R
from tests.test_gpu_requests import DEV, DeviceRun
from tests.test_gpu_requests_loop import CFG, FCFG, G, Cluster

pytestmark = pytest.mark.gpu
TERM = 8          # the leader's term: one above the last term of every log
CATCH_UP = 2      # SnapshotCatchUpEntries
LAG = 6           # entries node 1 lacks


def make_logs(rng):
    """The dummy entry and terms 1..7, one to three entries each: 8 runs."""
    return [[0] + [t for t in range(1, 8) for _ in range(int(rng.integers(1, 4)))] for _ in range(G)]


class Loop(Cluster):
    def __init__(self, logs):
        pr = P.progress
        self.nodes = []
        for j in range(3):
            row = []
            for g in range(G):
                last = len(logs[g]) - 1
                terms = logs[g][:last + 1 - LAG] if j == 1 else logs[g]
                prs = None
                if j == 0:   # node 1 probes, paused (a MsgApp is out), and is known to be alive
                    prs = [pr(last, last + 1, L.STATE_REPLICATE, True),
                           pr(last - LAG, last - LAG + 1, L.STATE_PROBE, True, True),
                           pr(last, last + 1, L.STATE_REPLICATE, True)]
                n = Q.make_node(3, 0b111, 0, j, terms=terms, term=TERM, self_id=j + 1,
                                role=R.LEADER if j == 0 else R.FOLLOWER, lead=1,
                                committed=len(terms) - 1, prs=prs, ee=g % 3,
                                applied=len(terms) - 1)
                n.camp.vote = 1
                row.append(n)
            self.nodes.append(row)
        self.runs = [DeviceRun(self.nodes[j], CFG) for j in range(3)]
        z = np.zeros(G, np.uint64)
        applied = [np.array([n.prop.applied for n in self.nodes[j]], np.uint64) for j in range(3)]
        self.ps = qp.ProposeState.from_numpy(applied[0], z, z, device=DEV)
        self.applied = [self.ps.applied] + [ql._to_dev(applied[j], np.uint64, DEV) for j in (1, 2)]

    def compact(self, j, where):
        """etcdserver's trigger at node j: every group is SnapshotCount behind,
        snapshots at applied and compacts CATCH_UP entries below it."""
        run = self.runs[j]
        t, ft = run.lg.t, run.es.follower.t
        nodes = [C.Node([(n.prop.first - 1 + i, tm) for i, tm in enumerate(n.prop.terms)],
                        n.prop.last + 1, n.prop.applied, n.group.log.snap_index,
                        n.group.log.snap_term) for n in run.nodes]
        req = C.Request(C.CM_TRIGGER, snapshot_count=3, catch_up_entries=CATCH_UP)
        ready = ReadyState(G, {"last_index": ft["last_index"], "applied": self.applied[j],
                               "unstable_offset": ft["last_index"] + 1,   # every entry is stable
                               "usnap_index": torch.zeros_like(ft["last_index"])})
        ds = D.DeviceState.over(qcm.leader_log(run.lg), ready, t["snap_index"], t["snap_term"])
        before = ds.numpy()
        stats = C.new_stats()
        ref = C.log_compact(nodes, req, G, stats)
        res = ds.compact(D.device_request(req, G), G)
        torch.cuda.synchronize()
        D.assert_state(ds.numpy(), CP.pack_nodes(nodes, base=before), where)
        D.assert_result(res, CP.pack_result(ref, G, D.POISON), stats, where)
        assert ref.flags == [C.SNAPPED | C.COMPACTED] * G and stats["runs_dropped"] >= 5 * G
        # the step calls' restatement follows, and the rows the compaction left
        # behind the count (nobody's) get the zeros back that its packer keeps there
        for n, cn in zip(run.nodes, nodes):
            n.prop.terms = [tm for _, tm in cn.ents]
            n.group.log.first = cn.first_index
            n.group.log.snap_index, n.group.log.snap_term = cn.snap_index, cn.snap_term
            n.sync()
        dead = torch.arange(C.MAX_RUNS, device=DEV)[:, None] >= ((t["meta"] >> 16) & 0xF)[None, :]
        for k in ("run_start", "run_term"):
            t[k].view(C.MAX_RUNS, G)[dead] = 0
        self.check(j, where)
        return ref

    def propose_one(self, where):
        """One entry at every leader; returns (pflags, the messages per group)."""
        run = self.runs[0]
        inp = P.inputs([PR.PROP_ENTRIES] * G, [1] * G, [8] * G)
        ib = qp.ProposeInbox.from_numpy(inp["action"], inp["n_ents"], inp["payload"], device=DEV)
        res = qp.leader_propose(run.lg, run.es, self.ps, ib)
        pf, _, sent = P.ref_propose([n.prop for n in run.nodes], inp, PR.Config(), run.off,
                                    P.new_msg(run.lg.S))
        assert np.array_equal(res.pflags.cpu().numpy()[:G], pf), where
        self.check(0, where)
        return pf, sent

    def log_step(self, j, recs, where):
        """(group, A.AppRec) through qb_dev_follower_log_step at node j, stops
        allowed; returns the reference's outputs."""
        run = self.runs[j]
        lognodes = []
        for n in run.nodes:
            c, g_ = n.camp, n.group
            lognodes.append(A.new_node(n.prop.terms, n.prop.first, term=g_.term, vote=c.vote,
                                       lead=c.lead, committed=g_.log.committed, role=c.role,
                                       election_elapsed=c.election_elapsed,
                                       heartbeat_elapsed=c.heartbeat_elapsed))
        want = A.step_batch(lognodes, recs, FCFG)
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
        res = qf.follower_log_step(run.es.follower, qcm.leader_log(run.lg), ib, app)
        M = len(recs)
        assert np.array_equal(res.resp_type.cpu().numpy()[:M], np.array(want["resp_type"], np.uint8))
        for key in ("resp_term", "resp_index", "app_from"):
            assert np.array_equal(ql._to_np(getattr(res, key), np.uint64, M),
                                  np.array(want[key], np.uint64)), (where, key)
        assert np.array_equal(ql._to_np(res.stop_at, np.uint32, G), np.array(want["stop_at"], np.uint32))
        assert np.array_equal(res.gflags.cpu().numpy()[:G], np.array(want["gflags"], np.uint8))
        self.check(j, where)
        return want


def test_the_ninth_term_round_trip():
    rng = np.random.default_rng(33)
    logs = make_logs(rng)
    c = Loop(logs)
    lead = c.nodes[0]
    last0 = [n.prop.last for n in lead]
    assert all(len(n.group.log.runs) == C.MAX_RUNS for j in (0, 2) for n in c.nodes[j])

    # ---- the leader: refused, compacted, accepted ---------------------------
    pf, sent = c.propose_one("propose at a full table")
    assert (pf == PR.PFLAG_LOG_RUNS).all() and not any(sent)
    c.compact(0, "compact at the leader")
    assert all(n.prop.first == last0[g] - CATCH_UP + 1 for g, n in enumerate(lead))
    assert all(n.prop.first > n.group.prs[1].next for n in lead)          # past node 1's next
    assert all((n.group.log.snap_index, n.group.log.snap_term) == (last0[g], 7)
               for g, n in enumerate(lead))
    pf, sent = c.propose_one("propose behind the compaction")
    assert all(f & PR.PFLAG_APPENDED and not f & PR.PFLAG_LOG_RUNS for f in pf)
    for g, msgs in enumerate(sent):   # node 2 gets the entry; node 1 is paused
        assert [(m[0], m[1], m[2], m[3], m[5]) for m in msgs] == [(L.MSG_APP, 2, last0[g], 7, 1)], g

    # ---- node 2: stopped, compacted, accepted ---------------------------------
    recs = [(g, AP.app(1, TERM, last0[g], 7, [TERM], lead[g].group.log.committed)) for g in range(G)]
    want = c.log_step(2, recs, "MsgApp at a full table")
    assert all(f & A.FFLAG_LOG_RUNS for f in want["gflags"]) and want["stop_at"] == list(range(G))
    assert not any(want["resp_type"])
    c.compact(2, "compact at node 2")
    want = c.log_step(2, recs, "the same MsgApp behind the compaction")
    assert all(f & A.FFLAG_APPENDED for f in want["gflags"])
    assert all(s == F.NO_STOP for s in want["stop_at"])
    assert want["resp_index"] == [x + 1 for x in last0]
    assert all(n.prop.terms[-2:] == [7, TERM] and len(n.group.log.runs) <= 4 for n in c.nodes[2])

    # ---- the responses at the leader -----------------------------------------
    resps = []
    for g in range(G):
        n = lead[g]
        resps.append((g, L.Inbound(L.IN_APP_RESP, 2, TERM, want["resp_index"][g])))
        if g % 2 == 0:
            resps.append((g, L.Inbound(L.IN_HEARTBEAT_RESP, 1, TERM, 0)))
        else:   # node 1 rejects the probe at next - 1 with its own last index as the hint
            nx = n.group.prs[1].next
            resps.append((g, L.Inbound(L.IN_APP_RESP, 1, TERM, nx - 1, True, nx - 1,
                                       c.nodes[1][g].prop.log_term(nx - 1))))
    msgs = c.leader_step(resps)
    for g, m in enumerate(msgs):
        snaps = [x for x in m if x[0] == L.MSG_SNAP]
        assert snaps == [(L.MSG_SNAP, 1, last0[g], 7, 0, 0)], (g, m)      # the new snapshot
        assert [x for x in m if x[1] == 2] and all(x[0] == L.MSG_APP for x in m if x[1] == 2), (g, m)
        assert lead[g].group.prs[1].state == L.STATE_SNAPSHOT
        assert lead[g].group.log.committed == last0[g] + 1                # the entry is committed
