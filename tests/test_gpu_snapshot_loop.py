"""The snapshot round trip on the device with no per-group host code between
the calls, for 257 three-node groups (tests/test_gpu_ready_loop.py's Loop:
node 0 leads, node 1 follows): the leader's log is compacted and its Progress
has node 1 below its first index, so

  qb_dev_leader_propose / qb_dev_leader_step   emit QB_MSG_SNAP,
  qb_dev_follower_snapshot at node 1           restores, fast-forwards or
                                               refuses it as old,
  qb_dev_ready                                 lists QB_RDF_SNAPSHOT,
  confchange.restore                           installs the ConfStates,
  qb_dev_leader_tick x election_timeout        raises no HUP at a restored group
                                               (TestRestore's last assertion),
  qb_dev_advance                               stable_snap and applied_to,
  qb_dev_leader_step on the MsgAppResps        takes the peer out of StateSnapshot.

Every call is compared bit-exact with its restatement (tests/snapshot_ref.py
beside ready_ref.py, propose_ref.py, tick_ref.py and oracle/leader_ref.py over
the same nodes), and every array after it."""
import numpy as np
import pytest
import torch

from etcd_amd.quorum import follower as qf, leader as ql, propose as qp, snapshot as qs
from etcd_amd.quorum.confchange import restore as cc_restore
from oracle import confchange_ref as CC, leader_ref as L
from tests import confchange_pack as CP, propose_pack as PP, propose_ref as PR
from tests import ready_ref as R, request_pack as Q, request_ref as RQ
from tests import snapshot_pack as SP, snapshot_ref as S, tick_ref as T
from tests.test_gpu_confchange import _render, _table
from tests.test_gpu_ready_loop import Loop, qy
from tests.test_gpu_requests import DEV, DeviceRun
from tests.test_gpu_requests_loop import CFG, ET, G, HT, TERM

pytestmark = pytest.mark.gpu
RESTORE, FAST_FORWARD, OLD = 0, 1, 2
CS = {"voters": [1, 2, 3], "learners": [], "voters_outgoing": [], "learners_next": []}


def kind_of(g):
    return g % 3


class SnapLoop(Loop):
    def __init__(self, rng):
        pr = PP.progress
        self.full, self.snap_at = [], []
        self.nodes = [[], [], []]
        for g in range(G):
            full = [0] + [1] * int(rng.integers(2, 4)) + [TERM] * int(rng.integers(3, 6))
            last = len(full) - 1
            s = last - int(rng.integers(0, 2))          # the leader compacted up to s
            self.full.append(full)
            self.snap_at.append(s)
            k = kind_of(g)
            mine = full[:2] if k == RESTORE else full   # node 1's log: far behind, or whole
            com1 = {RESTORE: 1, FAST_FORWARD: s - 1, OLD: s}[k]
            # a probe below the leader's first index; every other one has probed already
            p1 = pr(0, 1, L.STATE_PROBE, True, probe_sent=g % 2 == 0)
            prs = [pr(last, last + 1, L.STATE_REPLICATE, True), p1,
                   pr(last, last + 1, L.STATE_REPLICATE, True)]
            lead = Q.make_node(3, 0b111, 0, 0, terms=full[s:], first=s + 1, term=TERM, self_id=1,
                               role=RQ.LEADER, lead=1, committed=last, prs=prs, ee=g % 3)
            n1 = Q.make_node(3, 0b111, 0, 1, terms=mine, term=TERM, self_id=2, role=RQ.FOLLOWER,
                             lead=1, committed=com1, ee=g % 3)
            n2 = Q.make_node(3, 0b111, 0, 2, terms=full, term=TERM, self_id=3, role=RQ.FOLLOWER,
                             lead=1, committed=last, ee=g % 3)
            for j, n in enumerate((lead, n1, n2)):
                n.camp.vote = 1
                self.nodes[j].append(n)
        self.runs = [DeviceRun(self.nodes[j], CFG) for j in range(3)]
        z = np.zeros(G, np.uint64)
        self.ps = qp.ProposeState.from_numpy(z, z, z, device=DEV)
        self.first_last = [len(t) - 1 for t in self.full]
        self.state, self.rn = {}, {}
        self.rstats, self.astats, self.rstat_t, self.astat_t = {}, {}, {}, {}
        for j in (0, 1):
            run = self.runs[j]
            t, ft = run.lg.t, run.es.follower.t
            z64 = lambda: torch.zeros(G, dtype=torch.int64, device=DEV)  # noqa: E731
            shared = {"term": ft["term"], "vote": ft["vote"], "committed": ft["committed"],
                      "lead": ft["lead"], "role": run.state.role, "first_index": t["first_index"],
                      "last_index": ft["last_index"], "last_term": ft["last_term"],
                      "meta": t["meta"], "run_start": t["run_start"], "run_term": t["run_term"],
                      "pending_conf_index": self.ps.pending_conf_index if j == 0 else z64(),
                      "ext": None}
            # everything committed is applied, every entry stable
            self.state[j] = qy.ReadyState.new_raw_node(
                shared, ft["committed"].clone(), self.ps.uncommitted_size if j == 0 else z64())
            self.rn[j] = [R.Node() for _ in range(G)]
            self.sync(j)
            for r in self.rn[j]:
                r.offset, r.applied = r.last_index + 1, r.committed
                r.new_raw_node()
            self.rstats[j] = dict.fromkeys(R.RSTAT_NAMES, 0)
            self.astats[j] = dict.fromkeys(R.ASTAT_NAMES, 0)
            self.rstat_t[j] = torch.zeros(len(R.RSTAT_NAMES), dtype=torch.int64, device=DEV)
            self.astat_t[j] = torch.zeros(len(R.ASTAT_NAMES), dtype=torch.int64, device=DEV)
            self.check_ready_state(j, "NewRawNode")
        self.sstats = S.new_stats()
        self.sstat_t = torch.zeros(len(S.SSTAT_NAMES), dtype=torch.int64, device=DEV)

    # ---- the leader's two emitters ----------------------------------------
    def propose_snaps(self):
        """One entry at every leader; returns {group: (index, term)} of the
        MsgSnaps to slot 1."""
        run = self.runs[0]
        inp = PP.inputs([PR.PROP_ENTRIES] * G, [1] * G, [8] * G)
        ib = qp.ProposeInbox.from_numpy(inp["action"], inp["n_ents"], inp["payload"], device=DEV)
        res = qp.leader_propose(run.lg, run.es, self.ps, ib)
        pf, _, sent = PP.ref_propose([n.prop for n in run.nodes], inp, PR.Config(), run.off,
                                     PP.new_msg(run.lg.S))
        assert np.array_equal(res.pflags.cpu().numpy()[:G], pf)
        self.check(0, "propose")
        self.set_pending(0, [g for g, m in enumerate(sent) if m], qy.RDP_MSGS)
        return {g: (idx, lt) for g, msgs in enumerate(sent) for t, to, idx, lt, _, k in msgs
                if to == 1 and t == L.MSG_SNAP}

    # ---- the follower's call ------------------------------------------------
    def snapshot(self, snaps):
        """{group: (index, term)} through qb_dev_follower_snapshot at node 1."""
        run = self.runs[1]
        order = np.random.default_rng(3).permutation(sorted(snaps))
        recs = [(int(g), S.Snap(1, TERM, snaps[int(g)][0], snaps[int(g)][1], CS)) for g in order]
        nodes = []
        for n, r in zip(run.nodes, self.rn[1]):
            c, g_ = n.camp, n.group
            nodes.append(S.Node(
                id=c.self_id, term=g_.term, vote=c.vote, lead=c.lead, committed=g_.log.committed,
                state=c.role & 3, promotable=bool(c.role & 0x80), role_other=c.role & 0x7C,
                election_elapsed=c.election_elapsed, heartbeat_elapsed=c.heartbeat_elapsed,
                first_index=n.prop.first, terms=list(n.prop.terms), offset=r.offset, snap=r.snap,
                pending=(1 if r.msgs else 0) | (2 if r.read_states else 0)))
        want = S.snapshot_call(nodes, recs, st=self.sstats)
        t = run.lg.t
        rows_before = {k: ql._to_np(t[k], np.uint64, 8 * G).copy() for k in ("run_start", "run_term")}
        for n, r, sn in zip(run.nodes, self.rn[1], nodes):
            c, g_ = n.camp, n.group
            g_.term, c.vote, c.lead, g_.log.committed = sn.term, sn.vote, sn.lead, sn.committed
            c.role = sn.state | (0x80 if sn.promotable else 0) | sn.role_other
            c.election_elapsed, c.heartbeat_elapsed = sn.election_elapsed, sn.heartbeat_elapsed
            g_.log.first, n.prop.terms, c.last_term = sn.first_index, list(sn.terms), sn.terms[-1]
            n.sync()
            r.offset, r.snap, r.msgs = sn.offset, sn.snap, bool(sn.pending & 1)
        a = SP.pack_records(recs)
        inbox = qs.SnapshotInbox.from_numpy(a["group"], a["from"], a["term"], a["snap_index"],
                                            a["snap_term"], [m.cs for _, m in recs], device=DEV)
        flog = qf.FollowerLog(G, t["meta"], t["first_index"], t["run_start"], t["run_term"])
        out = qs.new_snapshot_result(len(recs), DEV)
        out.stats = self.sstat_t
        res = qs.follower_snapshot(run.es.follower, flog, self.state[1], run.es.self_id, inbox,
                                   out=out)
        torch.cuda.synchronize()
        Rn = len(recs)
        assert res.flags().tolist() == want["sflags"]
        assert res.resp_type.cpu().numpy()[:Rn].tolist() == want["resp_type"]
        for k in ("resp_term", "resp_index"):
            assert ql._to_np(getattr(res, k), np.uint64, Rn).tolist() == want[k], k
        assert res.stats_dict() == self.sstats
        # a restored table is one run; the rows behind it keep what they held
        # and are nobody's: compared, then given the packer's filler back
        packed = Q.pack_nodes(run.nodes, CFG.readq_cap)[0]
        live = (np.arange(8)[:, None] < ((packed["meta"] >> 16) & 0xF)[None, :]).ravel()
        for k in ("run_start", "run_term"):
            got = ql._to_np(t[k], np.uint64, 8 * G)
            assert np.array_equal(got[live], packed[k][live]), k
            assert np.array_equal(got[~live], rows_before[k][~live]), k
            t[k].copy_(ql._to_dev(np.where(live, got, packed[k]), np.uint64, DEV))
        self.sync(1)
        self.check_ready_state(1, "follower snapshot")
        self.check(1, "follower snapshot")
        return recs, want, inbox, res

    def tick_follower(self):
        """One tick at node 1; returns the tflags."""
        run = self.runs[1]
        res = run.lg.tick(run.state, ET, HT, True)
        tf = res.tflags.cpu().numpy()[:G]
        for g, n in enumerate(run.nodes):
            c = n.camp
            tn = T.TickNode(n.group, c.role, c.election_elapsed, c.heartbeat_elapsed, ET)
            assert T.tick(tn, ET, HT, True) == tf[g], g
            c.role, c.election_elapsed, c.heartbeat_elapsed = (tn.role, tn.election_elapsed,
                                                               tn.heartbeat_elapsed)
        self.check(1, "follower tick")
        return tf


def test_the_snapshot_round_trip():
    c = SnapLoop(np.random.default_rng(31))
    lead, peer = c.runs[0].nodes, c.runs[1].nodes
    # ---- the leader: the proposal's bcastAppend, then a heartbeat response ----
    snaps = c.propose_snaps()
    assert sorted(snaps) == [g for g in range(G) if g % 2 == 1]
    acks = [(g, L.Inbound(L.IN_HEARTBEAT_RESP, 1, TERM, 0)) for g in range(G) if g % 2 == 0]
    for g, msgs in enumerate(c.leader_step(acks)):
        for m in msgs:
            if m[0] == L.MSG_SNAP and m[1] == 1:
                assert g not in snaps
                snaps[g] = (m[2], m[3])
    c.set_pending(0, [g for g in range(G) if g % 2 == 0], qy.RDP_MSGS)
    assert sorted(snaps) == list(range(G))
    assert all(snaps[g] == (c.snap_at[g], c.full[g][c.snap_at[g]]) for g in range(G))
    assert all(n.group.prs[1].state == L.STATE_SNAPSHOT and
               n.group.prs[1].pending_snapshot == c.snap_at[g] for g, n in enumerate(lead))

    # ---- the follower ----------------------------------------------------------
    recs, want, inbox, res = c.snapshot(snaps)
    flag = {RESTORE: S.SNF_RESTORED, FAST_FORWARD: S.SNF_FAST_FORWARD, OLD: S.SNF_OLD}
    for (g, _), f in zip(recs, want["sflags"]):
        assert f & 0xFF == flag[kind_of(g)], (g, hex(f))
    restored = [g for g in range(G) if kind_of(g) == RESTORE]
    assert all(peer[g].prop.first == c.snap_at[g] + 1 and not peer[g].camp.role & 0x80
               for g in restored)
    rd = c.ready(1, "the follower's ready")
    by_gid = {r.gid: r for r in rd}
    assert sorted(by_gid) == list(range(G))                    # every group answers
    for g in range(G):
        r = by_gid[g]
        assert r.flags & R.RDF_MSGS
        assert bool(r.flags & R.RDF_SNAPSHOT) == (kind_of(g) == RESTORE)
        assert r.snap_index == (c.snap_at[g] if kind_of(g) == RESTORE else 0)
        assert bool(r.flags & R.RDF_HARD) == (kind_of(g) != OLD)

    # ---- the host's half: the config of the restored records -------------------
    groups, css = qs.restored_conf_states(inbox, res.sflags)
    assert sorted(groups.tolist()) == restored
    states = [dict(CS, auto_leave=False) if kind_of(g) == RESTORE else {} for g in range(G)]
    table, err, _ = cc_restore(_table([CC.Tracker.empty(5) for _ in range(G)], K=5), states,
                               [c.snap_at[g] for g in range(G)])
    assert not err.any()
    dev = CP.unpack(table.numpy(), 5)
    for g in restored:
        wantcfg = CC.restore(CC.Tracker.empty(5), c.snap_at[g], [1, 2, 3], [], [], [], False)
        assert _render(dev[g]) == _render(wantcfg), g

    # ---- it does not campaign before the snapshot is applied -------------------
    c.runs[1].state.rand_timeout.fill_(ET)
    hups = np.zeros(G, bool)
    for _ in range(ET):
        hups |= (c.tick_follower() & T.TFLAG_HUP) != 0
    assert not hups[restored].any()
    assert hups[[g for g in range(G) if kind_of(g) != RESTORE]].all()

    # ---- persist, apply, advance; the host re-arms promotable ------------------
    adv = [R.record_of(r) for r in rd]
    assert all(a.stable_snap == c.snap_at[a.gid] and a.applied_to == c.snap_at[a.gid]
               for a in adv if kind_of(a.gid) == RESTORE)
    assert not any(c.advance(1, adv, "the follower's advance"))
    assert all(c.rn[1][g].snap is None and c.rn[1][g].applied == c.snap_at[g] for g in restored)
    assert c.astats[1]["snap_stable"] == len(restored)
    assert not c.ready(1, "the follower's ready after the advance")

    # ---- the MsgAppResps at the leader -----------------------------------------
    resps = [(g, L.Inbound(L.IN_APP_RESP, 1, want["resp_term"][i], want["resp_index"][i]))
             for i, (g, _) in enumerate(recs)]
    resps.sort(key=lambda x: x[0])
    c.leader_step(resps)
    for g, n in enumerate(lead):
        p = n.group.prs[1]
        assert p.state != L.STATE_SNAPSHOT and p.pending_snapshot == 0, g
        assert p.match == (c.snap_at[g] if kind_of(g) != FAST_FORWARD else c.snap_at[g]), g
