"""The RawNode loop on the device with no per-group host code between the
calls, for 257 three-node groups (tests/test_gpu_requests_loop.py's Cluster:
node 0 leads, node 1 follows), three rounds of

  qb_dev_leader_propose -> qb_dev_ready -> qb_dev_advance        at the leader,
  qb_dev_follower_log_step -> qb_dev_unstable_truncate ->
      qb_dev_ready -> qb_dev_advance                             at the follower,
  qb_dev_leader_step on the follower's MsgAppResps.

The host's part is what INTEGRATION.md gives it: it sets the pending bits
from the step calls' flags, hands each Ready back as an Advance record, trims
a committed range (a paginated apply) and is sometimes slow — in the second
round every fifth group's follower Ready is not advanced, and in the third a
new leader's MsgApp rewrites those groups' last entry, so the late Advance
meets a truncated log: QB_AFLAG_STABLE_STALE, and the entries are listed
again.  Every call is compared bit-exact with its restatement
(tests/ready_ref.py beside propose_ref.py, append_ref.py and
oracle/leader_ref.py over the same nodes), and every array after it."""
import importlib

import numpy as np
import pytest
import torch

from etcd_amd.quorum import follower as qf, leader as ql, propose as qp
from oracle import leader_ref as L
from tests import append_pack as AP, append_ref as A, follower_ref as F
from tests import propose_pack as PP, propose_ref as PR
from tests import ready_pack as P, ready_ref as R
from tests.test_gpu_requests import DEV
from tests.test_gpu_requests_loop import FCFG, G, TERM, Cluster, make_logs

qy = importlib.import_module("etcd_amd.quorum.ready")

pytestmark = pytest.mark.gpu
PAYLOAD = 8
SHARED_CHECK = ("term", "vote", "committed", "lead", "role", "first_index", "last_index",
                "last_term")


_SIGNED = {np.uint64: np.int64, np.uint32: np.int32, np.uint16: np.int16, np.uint8: np.uint8}


def filled(n, dt):
    """A device buffer pre-filled with the marker of its width."""
    return torch.from_numpy(np.full(max(n, 1), P._FILLS[dt], dt).view(_SIGNED[dt])).to(DEV)


class Loop(Cluster):
    def __init__(self, logs):
        super().__init__(logs, [0] * G)
        self.first_last = [len(t) - 1 for t in logs]   # entries up to here carry no payload
        self.state, self.rn = {}, {}
        self.rstats, self.astats, self.rstat_t, self.astat_t = {}, {}, {}, {}
        for j in (0, 1):
            run = self.runs[j]
            t, ft = run.lg.t, run.es.follower.t
            z = lambda: torch.zeros(G, dtype=torch.int64, device=DEV)  # noqa: E731
            shared = {"term": ft["term"], "vote": ft["vote"], "committed": ft["committed"],
                      "lead": ft["lead"], "role": run.state.role, "first_index": t["first_index"],
                      "last_index": ft["last_index"], "last_term": ft["last_term"],
                      "meta": t["meta"], "run_start": t["run_start"], "run_term": t["run_term"],
                      "pending_conf_index": self.ps.pending_conf_index if j == 0 else z(),
                      "ext": None}
            # a restart: nothing applied yet, every entry stable
            self.state[j] = qy.ReadyState.new_raw_node(
                shared, self.ps.applied if j == 0 else z(),
                self.ps.uncommitted_size if j == 0 else z())
            self.rn[j] = [R.Node() for _ in range(G)]
            self.sync(j)
            for g, r in enumerate(self.rn[j]):
                r.offset = r.last_index + 1
                r.new_raw_node()
            self.rstats[j] = dict.fromkeys(R.RSTAT_NAMES, 0)
            self.astats[j] = dict.fromkeys(R.ASTAT_NAMES, 0)
            self.rstat_t[j] = torch.zeros(len(R.RSTAT_NAMES), dtype=torch.int64, device=DEV)
            self.astat_t[j] = torch.zeros(len(R.ASTAT_NAMES), dtype=torch.int64, device=DEV)
            self.check_ready_state(j, "NewRawNode")

    # ---- the Ready restatement beside the step calls' nodes --------------
    def sync(self, j):
        """What the step calls left, into the Ready nodes."""
        for n, r in zip(self.runs[j].nodes, self.rn[j]):
            c = n.camp
            r.term, r.vote, r.committed, r.lead = n.group.term, c.vote, n.group.log.committed, c.lead
            r.state, r.promotable = c.role & 0x7F, bool(c.role & 0x80)
            r.first_index, r.terms = n.prop.first, list(n.prop.terms)
            r.pending_conf_index = n.prop.pending_conf_index
            r.uncommitted_size = n.prop.uncommitted_size

    def sync_back(self, j):
        """What Advance wrote of the proposal's words, into the step calls'
        nodes (the device shares the buffers)."""
        if j == 0:
            for n, r in zip(self.runs[j].nodes, self.rn[j]):
                n.prop.applied, n.prop.uncommitted_size = r.applied, r.uncommitted_size

    def check_ready_state(self, j, where):
        want = P.pack_nodes(self.rn[j])
        got = self.state[j].numpy()
        for k in P.STATE + SHARED_CHECK:
            assert np.array_equal(got[k], want[k]), (where, j, k,
                                                     np.flatnonzero(got[k] != want[k])[:8])

    def set_pending(self, j, groups, bit):
        """The host's part: pending bits from a step call's outputs."""
        mask = np.zeros(G, np.uint8)
        mask[groups] = bit
        self.state[j].t["pending"] |= torch.from_numpy(mask).to(DEV)
        for g in groups:
            if bit & qy.RDP_MSGS:
                self.rn[j][g].msgs = True

    def ready(self, j, where):
        self.sync(j)
        rflags, records, count, st = R.ready_call(self.rn[j], True, G)
        for k, v in st.items():
            self.rstats[j][k] += v
        out = qy.ReadyResult(G, filled(G, np.uint16),
                             {k: filled(G, dt) for k, dt in P.LIST.items()}, filled(1, np.uint64),
                             self.rstat_t[j])
        qy.ready(self.state[j], accept=True, out=out)
        torch.cuda.synchronize()
        assert out.count() == count, where
        assert np.array_equal(out.rflags.cpu().numpy().view(np.uint16),
                              np.array(rflags, np.uint16)), where
        want = P.pack_records(records, G)
        for k, dt in P.LIST.items():
            assert np.array_equal(out.cols[k].cpu().numpy().view(dt), want[k]), (where, k)
        assert out.stats_dict() == self.rstats[j], where
        self.check_ready_state(j, where)
        self.check(j, where)   # the step calls' arrays are only read
        return records

    def payload(self, g, lo, hi):
        """PayloadSize over the applied entries: the proposed ones carry 8."""
        return PAYLOAD * max(0, hi - max(lo, self.first_last[g] + 1) + 1)

    def host_records(self, records, paginate):
        """Each Ready handled in full, or (paginate) applied one entry at a time."""
        out = []
        for r in records:
            cursor = None
            if r.flags & R.RDF_COMMITTED:
                cursor = r.apply[0] if paginate(r.gid) else r.apply[1]
            rec = R.record_of(r, cursor)
            if cursor is not None:
                rec.applied_payload = self.payload(r.gid, r.apply[0], cursor)
            out.append(rec)
        return out

    def advance(self, j, recs, where):
        aflags, st = R.advance_call(self.rn[j], recs)
        for k, v in st.items():
            self.astats[j][k] += v
        A_ = len(recs)
        out = qy.AdvanceResult(torch.full((max(A_, 1),), 0xA5, dtype=torch.uint8, device=DEV),
                               self.astat_t[j])
        qy.advance(self.state[j], qy.AdvanceRecords.from_numpy(P.pack_advance(recs), device=DEV),
                   out=out)
        torch.cuda.synchronize()
        assert np.array_equal(out.aflags.cpu().numpy()[:A_], np.array(aflags, np.uint8)), where
        assert out.stats_dict() == self.astats[j], where
        self.sync_back(j)
        self.check_ready_state(j, where)
        self.check(j, where)
        return aflags

    # ---- the step calls (the Cluster's, returning what the loop needs) ---
    def propose_entries(self):
        """One entry of 8 bytes at every leader; returns the MsgApps to slot 1
        as (group, index, log_term, commit, n)."""
        run = self.runs[0]
        inp = PP.inputs([PR.PROP_ENTRIES] * G, [1] * G, [PAYLOAD] * G)
        ib = qp.ProposeInbox.from_numpy(inp["action"], inp["n_ents"], inp["payload"], device=DEV)
        res = qp.leader_propose(run.lg, run.es, self.ps, ib)
        pf, _, sent = PP.ref_propose([n.prop for n in run.nodes], inp, PR.Config(), run.off,
                                     PP.new_msg(run.lg.S))
        assert np.array_equal(res.pflags.cpu().numpy()[:G], pf)
        assert all(f & PR.PFLAG_APPENDED for f in pf)
        self.check(0, "propose")
        assert np.array_equal(ql._to_np(self.ps.uncommitted_size, np.uint64, G),
                              np.array([n.prop.uncommitted_size for n in run.nodes], np.uint64))
        self.set_pending(0, [g for g, m in enumerate(sent) if m], qy.RDP_MSGS)
        return [(g, idx, lt, run.nodes[g].group.log.committed, k)
                for g, msgs in enumerate(sent) for t, to, idx, lt, _, k in msgs
                if to == 1 and t == L.MSG_APP]

    def log_step(self, recs):
        """MsgApps through qb_dev_follower_log_step at node 1, then the fold of
        app_from into the unstable offsets; returns the reference's outputs."""
        run = self.runs[1]
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
        t = run.lg.t
        flog = qf.FollowerLog(G, t["meta"], t["first_index"], t["run_start"], t["run_term"])
        res = qf.follower_log_step(run.es.follower, flog, ib, app)
        M = len(recs)
        assert np.array_equal(res.resp_type.cpu().numpy()[:M], np.array(want["resp_type"], np.uint8))
        for key in ("resp_term", "resp_index", "app_from"):
            assert np.array_equal(ql._to_np(getattr(res, key), np.uint64, M),
                                  np.array(want[key], np.uint64)), key
        assert np.array_equal(res.gflags.cpu().numpy()[:G], np.array(want["gflags"], np.uint8))
        assert all(s == F.NO_STOP for s in want["stop_at"])
        self.check(1, "follower log step")
        # unstable.truncateAndAppend on the Ready nodes, record by record, beside
        # the fold's min
        for (g, m), af in zip(recs, want["app_from"]):
            if af:
                rn = self.rn[1][g]
                before = rn.offset
                tail = list(lognodes[g].terms[af - (rn.first_index - 1):])
                R.truncate_and_append(rn, af, tail)
                assert rn.terms == lognodes[g].terms and rn.offset == min(before, af)
        qy.unstable_truncate(self.state[1], ib.group, res.app_from, M=M)
        torch.cuda.synchronize()
        self.sync(1)
        self.check_ready_state(1, "truncate fold")
        return want


def test_three_rounds_of_the_ready_loop():
    rng = np.random.default_rng(21)
    c = Loop(make_logs(rng))
    slow = [g for g in range(G) if g % 5 == 0]       # the follower's host is slow here
    rewritten = [g for g in range(G) if g % 5 in (0, 2)]  # a new leader rewrites the last entry
    paginate = lambda g: g % 4 == 1  # noqa: E731
    late = []
    saw_paginated = saw_relisted = 0
    for rnd in range(3):
        # ---- the leader -------------------------------------------------
        apps = c.propose_entries()
        assert len(apps) == G
        recs0 = c.ready(0, f"round {rnd}: leader ready")
        assert len(recs0) == G and all(r.flags & R.RDF_ENTRIES and r.flags & R.RDF_MSGS
                                       and r.flags & R.RDF_MUST_SYNC for r in recs0)
        if rnd == 0:   # the restart: everything committed is still to apply
            assert all(r.flags & R.RDF_COMMITTED and r.apply[0] == 1 for r in recs0)
        adv0 = c.host_records(recs0, paginate)
        assert not any(c.advance(0, adv0, f"round {rnd}: leader advance"))
        for r, a in zip(recs0, adv0):
            if r.flags & R.RDF_COMMITTED and a.applied_to < r.apply[1]:
                saw_paginated += 1

        # ---- the follower -----------------------------------------------
        msgs = [(g, AP.app(1, TERM, idx, lt, [TERM] * k, commit)) for g, idx, lt, commit, k in apps]
        if rnd == 2:
            for i, (g, _) in enumerate(msgs):
                if g in rewritten:   # node 3 won term 3 and overwrites the follower's last entry
                    n = c.runs[1].nodes[g]
                    last = n.prop.last
                    assert last > n.group.log.committed
                    msgs[i] = (g, AP.app(3, TERM + 1, last - 1, n.prop.log_term(last - 1),
                                         [TERM + 1], n.group.log.committed))
        offsets = [r.offset for r in c.rn[1]]
        want = c.log_step(msgs)
        # the MsgAppResps wait in r.msgs for the Ready
        c.set_pending(1, [g for i, (g, _) in enumerate(msgs) if want["resp_type"][i]], qy.RDP_MSGS)
        if rnd == 2:
            assert all(want["app_from"][i] == c.runs[1].nodes[g].prop.last
                       for i, (g, _) in enumerate(msgs) if g in rewritten)
            # the fold lowered the offset of the groups whose Ready had been advanced
            assert all(c.rn[1][g].offset < offsets[g] for g in rewritten if g not in slow)
            flags = c.advance(1, late, "the late advance")
            assert all(f == R.AFLAG_STABLE_STALE for f in flags) and len(flags) == len(slow)
        recs1 = c.ready(1, f"round {rnd}: follower ready")
        assert len(recs1) == G and all(r.flags & R.RDF_ENTRIES for r in recs1)
        if rnd == 2:
            for r in recs1:
                if r.gid in slow:    # listed again, from the old offset, with the new term
                    assert r.ent == (offsets[r.gid], offsets[r.gid], TERM + 1)
                    saw_relisted += 1
        adv1 = c.host_records(recs1, paginate)
        if rnd == 1:
            late = [a for a in adv1 if a.gid in slow]
            adv1 = [a for a in adv1 if a.gid not in slow]
        assert not any(c.advance(1, adv1[::-1], f"round {rnd}: follower advance"))

        # ---- the acks at the leader -------------------------------------
        resps = [(g, L.Inbound(L.IN_APP_RESP, 1, want["resp_term"][i], want["resp_index"][i]))
                 for i, (g, _) in enumerate(msgs) if not (rnd == 2 and g in rewritten)]
        sent = c.leader_step(resps)
        c.set_pending(0, [g for g, m in enumerate(sent) if m], qy.RDP_MSGS)
    assert saw_paginated >= G // 4 - 1 and saw_relisted == len(slow)
    # the commits the last acks brought: a HardState and entries to apply
    last = c.ready(0, "the leader's last ready")
    acked = [r for r in last if r.gid not in rewritten]
    assert all(r.flags & R.RDF_HARD and r.flags & R.RDF_COMMITTED for r in acked)
    # a paginated group is still behind, and its next range starts where it stopped
    behind = [r for r in last if paginate(r.gid) and r.flags & R.RDF_COMMITTED]
    assert behind and all(r.apply[0] == c.rn[0][r.gid].applied + 1 for r in behind)
