"""An election of N nodes over G groups as a sequence of batched calls — tick
until MsgHup, campaign, follower step on the peers, record votes, tally,
campaign (WON / LOST), one more tick — written once against a small cluster
interface and run through the restatements here (``RefCluster``: tick_ref,
campaign_ref, follower_ref and the votes oracle) and, in
tests/test_gpu_campaign.py, through the device beside them.  One table per
node: node j sits in slot j of each of its groups and has raft ID j + 1.

What the host would do between the calls is left out on both sides: no new
randomized timeout after a reset and no empty entry appended by a new leader
(neither is read by the calls that follow).  Test infrastructure."""
from __future__ import annotations

import numpy as np

from oracle import quorum_ref as Q
from tests import campaign_pack as P, campaign_ref as R, follower_ref as F, tick_ref as T
from tests.parity_checks import NONE as NO_INDEX, sequential_votes

ET, HT = 4, 1          # electionTimeout / heartbeatTimeout of the loop
LATE = ET + 3          # the randomized timeout of a node that does not campaign first


def make_cluster(seed: int, N: int, G: int):
    """nodes[j][g]: node j's CampaignNode of group g, all followers at one
    term with no leader; rand[j][g]: its randomized timeout (ET for the
    seeded candidates — one, two or all N per group — else LATE).  A third of
    the logs are stale (a shorter log or an older last term)."""
    rng = np.random.default_rng(seed)
    nodes = [[] for _ in range(N)]
    rand = [np.full(G, LATE, np.uint32) for _ in range(N)]
    full = (1 << N) - 1
    for g in range(G):
        term = int(rng.integers(3, 9))
        last, lterm = int(rng.integers(2, 50)), int(rng.integers(2, term + 1))
        r = rng.random()
        k = 1 if r < 0.6 else (2 if r < 0.85 else N)
        for j in rng.choice(N, k, replace=False):
            rand[int(j)][g] = ET
        for j in range(N):
            li, lt = last, lterm
            if rng.random() < 0.33:
                li, lt = (last - 1, lterm) if rng.random() < 0.5 else (last + 2, lterm - 1)
            nodes[j].append(P.make_node(N, full, 0, j, self_id=j + 1, term=term,
                                        role=R.FOLLOWER | R.ROLE_PROMOTABLE, last_index=li,
                                        last_term=lt, committed=int(rng.integers(0, li)),
                                        rng=np.random.default_rng(seed * 1000003 + g * 16 + j)))
    return nodes, rand


class RefCluster:
    """The cluster interface over the restatements; every method takes the
    node (table) index first and returns numpy outputs."""

    def __init__(self, nodes, rand, pre_vote: bool, check_quorum: bool = True):
        self.nodes, self.rand = nodes, rand
        self.N, self.G = len(nodes), len(nodes[0])
        self.pre_vote, self.check_quorum = pre_vote, check_quorum
        self.fcfg = F.Config(election_timeout=ET, check_quorum=check_quorum, pre_vote=pre_vote)

    def tick(self, j):
        tf = np.zeros(self.G, np.uint8)
        for g, n in enumerate(self.nodes[j]):
            t = T.TickNode(n.group, n.role, n.election_elapsed, n.heartbeat_elapsed,
                           int(self.rand[j][g]))
            tf[g] = T.tick(t, ET, HT, self.check_quorum)
            n.role, n.election_elapsed, n.heartbeat_elapsed = (t.role, t.election_elapsed,
                                                               t.heartbeat_elapsed)
        return tf

    def campaign(self, j, action):
        req_term, req_mask = np.zeros(self.G, np.uint64), np.zeros(self.G, np.uint16)
        cf, rt, _ = P.ref_campaign(self.nodes[j], action, self.pre_vote, req_term, req_mask)
        return cf, rt, req_term, req_mask

    def requests(self, j, g):
        return [{"type": r.type, "to": r.to, "term": r.term, "index": r.index,
                 "log_term": r.log_term, "transfer": r.transfer} for r in self.nodes[j][g].reqs]

    def follower_step(self, j, recs):
        """recs: (group, F.Rec) in arrival order -> (resp_type, resp_term)."""
        ns = self.nodes[j]
        fn = [F.Node(n.group.term, n.vote, n.lead, n.group.log.committed, n.group.log.last,
                     n.last_term, n.role, n.election_elapsed, n.heartbeat_elapsed) for n in ns]
        rt, rterm, stop, _, _ = F.step_batch(fn, recs, self.fcfg)
        assert all(s == F.NO_STOP for s in stop)
        for n, f in zip(ns, fn):
            n.group.term, n.vote, n.lead, n.group.log.committed = f.term, f.vote, f.lead, f.committed
            n.role, n.election_elapsed, n.heartbeat_elapsed = (f.role, f.election_elapsed,
                                                               f.heartbeat_elapsed)
        return np.array(rt, np.uint8), np.array(rterm, np.uint64)

    def record_votes(self, j, prevote, recs):
        """recs: (group, slot, reject, term) -> (stepdown_at, decided_at)."""
        ns = self.nodes[j]
        cfg = np.array([n.group.mask_in | n.group.mask_out << 16 for n in ns], np.uint32)
        votes0 = np.array([P.votes_word(n.votes) for n in ns], np.uint32)
        gterm = np.array([n.group.term for n in ns], np.uint64)
        group = np.array([r[0] for r in recs], np.uint32)
        flags = np.array([r[1] | (0x80 if r[2] else 0) for r in recs], np.uint8)
        term = np.array([r[3] for r in recs], np.uint64)
        votes, sd, dec, _ = sequential_votes(prevote, cfg, votes0, gterm, group, flags, term)
        for n, w in zip(ns, votes):
            n.votes = P.votes_dict(int(w))
        return sd, dec

    def tally(self, j):
        return np.array([Q.tally_votes_slots(n.group.mask_in, n.group.mask_out, n.votes)[2]
                         for n in self.nodes[j]], np.uint8)

    def roles(self, j):
        return np.array([n.role for n in self.nodes[j]], np.uint8)


def run_election(c, log=None):
    """The loop over a cluster (RefCluster or anything with its methods).
    Returns (rounds of vote requests, the final tick's tflags per node)."""
    N, G = c.N, c.G
    for k in range(ET):
        tf = [c.tick(j) for j in range(N)]
        hup = [(t & T.TFLAG_HUP) != 0 for t in tf]
        assert any(h.any() for h in hup) == (k == ET - 1), f"tick {k}"
    action = [np.where(h, R.CAMP_HUP, R.CAMP_NONE).astype(np.uint8) for h in hup]
    rounds = 0
    while any(a.any() for a in action):
        out = [c.campaign(j, action[j]) if action[j].any() else None for j in range(N)]
        inbox = [[] for _ in range(N)]
        asked = [None] * N
        for j in range(N):  # requests in candidate order: each peer's arrival order
            if out[j] is None:
                continue
            asked[j] = np.flatnonzero(out[j][1])
            for g in asked[j].tolist():
                for m in c.requests(j, g):
                    kind = F.VOTE if m["type"] == R.MSG_VOTE else F.PREVOTE
                    inbox[m["to"]].append((g, F.Rec(kind, j + 1, m["term"], m["index"],
                                                    m["log_term"], m["transfer"])))
        answers = [[] for _ in range(N)]
        kinds = [set() for _ in range(N)]
        for p in range(N):
            if not inbox[p]:
                continue
            rt, rterm = c.follower_step(p, inbox[p])
            for i, (g, m) in enumerate(inbox[p]):
                assert rt[i] & 0x7F in (F.MSG_VOTE_RESP, F.MSG_PREVOTE_RESP)
                answers[m.frm - 1].append((g, p, bool(rt[i] & F.REJECT), int(rterm[i])))
                kinds[m.frm - 1].add(m.kind)
        action = [np.zeros(G, np.uint8) for _ in range(N)]
        for j in range(N):
            if not answers[j]:
                continue
            assert len(kinds[j]) == 1  # the nodes move in lockstep: one kind per round
            sd, dec = c.record_votes(j, kinds[j] == {F.PREVOTE}, answers[j])
            assert (sd == NO_INDEX).all()  # nobody answers from a higher term here
            res = c.tally(j)
            a = np.select([res == Q.VOTE_WON, res == Q.VOTE_LOST], [R.CAMP_WON, R.CAMP_LOST], 0)
            action[j][asked[j]] = a[asked[j]]
        rounds += 1
        if log is not None:
            log.append([int((a != 0).sum()) for a in action])
        assert rounds <= 4
    return rounds, [c.tick(j) for j in range(N)]
