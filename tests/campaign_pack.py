"""Shared infrastructure of the campaign tests: the golden scenarios as
CampaignNodes, a seeded random batch, packing to and from the engine's arrays
(tests/leader_pack.py for the arrays the campaign shares with the leader
step), and the expected outputs of one call from tests/campaign_ref.py.
Test infrastructure."""
from __future__ import annotations

import json
import os

import numpy as np

from oracle import leader_ref as L
from oracle import quorum_ref as Q
from tests import campaign_ref as R, leader_pack
from tests.tick_ref import mark_learners

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5A5A5A5A5A5A5A5  # the outputs' pre-fill: untouched elements keep it
INFLIGHT_CAP = 2


def load_tables():
    with open(os.path.join(ROOT, "tests", "golden", "campaign_tables.json"), encoding="utf-8") as f:
        return json.load(f)


def make_node(ns, mask_in, mask_out, own, *, self_id=1, term=1, vote=0, lead=0, role=R.FOLLOWER,
              last_index=0, last_term=0, committed=0, votes=None, ee=0, he=0, rng=None,
              readq_cap=0) -> R.CampaignNode:
    """A CampaignNode over a LeaderGroup of ns slots.  With ``rng`` the
    Progress, the rings, the transferee and the read queue hold seeded junk
    (what a reset must overwrite); else a quiet probe state."""
    prs = []
    for _ in range(ns):
        infl = L.Inflights(INFLIGHT_CAP)
        if rng is None:
            prs.append(L.Progress(match=0, next=1, inflights=infl))
            continue
        infl.buffer = [int(x) for x in rng.integers(1, 1 << 40, INFLIGHT_CAP)]
        infl.start = int(rng.integers(0, INFLIGHT_CAP))
        infl.count = int(rng.integers(0, INFLIGHT_CAP + 1))
        prs.append(L.Progress(match=int(rng.integers(0, 1 << 50)), next=int(rng.integers(1, 1 << 50)),
                              state=int(rng.integers(0, 3)),
                              pending_snapshot=int(rng.integers(0, 1 << 30)),
                              recent_active=bool(rng.random() < 0.5),
                              probe_sent=bool(rng.random() < 0.5), inflights=infl))
    log = L.LogView(first=1, last=last_index, committed=committed, runs=[(0, last_term)])
    transferee, readq, pending = L.NO_SLOT, [], False
    if rng is not None:
        if ns and rng.random() < 0.4:
            transferee = int(rng.integers(0, ns))
        nq = int(rng.integers(0, readq_cap + 1))
        readq = [L.ReadIndexStatus(int(rng.integers(1, 1 << 62)), committed, set(), L.NO_SLOT)
                 for _ in range(nq)]
        pending = bool(rng.random() < 0.3)
    g = L.LeaderGroup(ns, mask_in, mask_out, term, own, log, prs, transferee=transferee,
                      readq=readq, pending_readindex=pending)
    mark_learners(g)
    return R.CampaignNode(g, self_id, role, vote, lead, last_term, ee, he, dict(votes or {}))


def build_node(sc) -> R.CampaignNode:
    """A golden scenario's node: slot j is the j-th smallest ID."""
    nd = sc["node"]
    ids = nd["ids"]
    slot = {i: s for s, i in enumerate(ids)}
    mask_in = sum(1 << slot[i] for i in nd["voters"])
    mask_out = sum(1 << slot[i] for i in nd["voters_out"])
    own = slot.get(nd["self"], L.NO_SLOT)
    return make_node(len(ids), mask_in, mask_out, own, self_id=nd["self"], term=nd["term"],
                     vote=nd["vote"], lead=nd["lead"], role=nd["state"] | R.ROLE_PROMOTABLE,
                     last_index=nd["last_index"], last_term=nd["last_term"],
                     committed=nd["committed"], votes={slot[i]: True for i in nd["votes"]})


def record_vote(n: R.CampaignNode, slot: int, granted: bool) -> int:
    """stepCandidate's poll (raft.go:1399-1401 -> 837-845): RecordVote with
    first-vote-wins, TallyVotes.  Returns the action that follows (CAMP_WON /
    CAMP_LOST / CAMP_NONE); a node that is no (pre-)candidate ignores it."""
    if n.state not in (R.CANDIDATE, R.PRE_CANDIDATE):
        return R.CAMP_NONE
    n.votes.setdefault(slot, granted)
    res = Q.tally_votes_slots(n.group.mask_in, n.group.mask_out, n.votes)[2]
    return {Q.VOTE_WON: R.CAMP_WON, Q.VOTE_LOST: R.CAMP_LOST}.get(res, R.CAMP_NONE)


def check_expect(where, exp, cflags: int, reqs, n: R.CampaignNode, ids):
    """reqs: dicts / Requests with type, to (slot), term, index, log_term,
    transfer; n: the state after."""
    def get(m, k):
        return m[k] if isinstance(m, dict) else getattr(m, k)
    if "state" in exp:
        assert n.state == exp["state"], f"{where}: state {n.state}, want {exp['state']}"
    if "term" in exp:
        assert n.group.term == exp["term"], f"{where}: term {n.group.term}, want {exp['term']}"
    if "lead" in exp:
        assert n.lead == exp["lead"], f"{where}: lead {n.lead}, want {exp['lead']}"
    if "self_vote" in exp:
        assert n.votes.get(n.own) is exp["self_vote"], f"{where}: votes {n.votes}"
    if "ignored" in exp:
        assert bool(cflags & R.CFLAG_IGNORED) == exp["ignored"], f"{where}: cflags {cflags:#x}"
    if "reqs" in exp:
        got = [[get(m, "type"), ids[get(m, "to")], get(m, "term"), get(m, "index"),
                get(m, "log_term"), get(m, "transfer")] for m in reqs]
        assert got == exp["reqs"], f"{where}: requests {got}, want {exp['reqs']}"


# ------------------------------------------------------------------ packing ---

def votes_word(votes: dict) -> int:
    voted = sum(1 << s for s in votes)
    granted = sum(1 << s for s, v in votes.items() if v)
    return voted | (granted << 16)


def votes_dict(word: int) -> dict:
    return {s: bool((word >> (16 + s)) & 1) for s in range(16) if (word >> s) & 1}


def pack_nodes(nodes, readq_cap: int = 0, inflight_cap: int = INFLIGHT_CAP):
    """(leader-step arrays, election arrays) of a batch."""
    a = leader_pack.pack([n.group for n in nodes], inflight_cap, readq_cap)
    e = {"self_id": np.array([n.self_id for n in nodes], np.uint64),
         "vote": np.array([n.vote for n in nodes], np.uint64),
         "lead": np.array([n.lead for n in nodes], np.uint64),
         "last_term": np.array([n.last_term for n in nodes], np.uint64),
         "role": np.array([n.role for n in nodes], np.uint8),
         "election_elapsed": np.array([n.election_elapsed for n in nodes], np.uint32),
         "heartbeat_elapsed": np.array([n.heartbeat_elapsed for n in nodes], np.uint32),
         "votes": np.array([votes_word(n.votes) for n in nodes], np.uint32)}
    return a, e


def unpack_into(nodes, a, e, readq_cap: int = 0, inflight_cap: int = INFLIGHT_CAP):
    """Overwrite the mutable state of ``nodes`` from engine arrays."""
    leader_pack.unpack_into([n.group for n in nodes], a, inflight_cap, readq_cap)
    for i, n in enumerate(nodes):
        meta = int(a["meta"][i])
        n.group.term = int(a["term"][i])
        n.group.transferee = (meta >> 8) & 0xFF
        n.vote, n.lead = int(e["vote"][i]), int(e["lead"][i])
        n.role = int(e["role"][i])
        n.election_elapsed = int(e["election_elapsed"][i])
        n.heartbeat_elapsed = int(e["heartbeat_elapsed"][i])
        n.votes = votes_dict(int(e["votes"][i]))


def state_key(n: R.CampaignNode):
    """Everything observable about a node after a call."""
    g = n.group
    return (leader_pack.state_key(g), g.term, g.transferee, n.vote, n.lead, n.role,
            n.election_elapsed, n.heartbeat_elapsed, tuple(sorted(n.votes.items())))


def ref_campaign(nodes, actions, pre_vote, req_term, req_mask):
    """One call through campaign_ref over ``nodes`` (in place); req_term /
    req_mask (numpy, in place) get a value only where a request goes out.
    Returns (cflags, req_type, stats of this call)."""
    G = len(nodes)
    cflags, req_type = np.zeros(G, np.uint8), np.zeros(G, np.uint8)
    st = R.new_stats()
    for i, n in enumerate(nodes):
        cflags[i] = R.step(n, int(actions[i]), bool(pre_vote), st)
        if n.reqs:
            r0 = n.reqs[0]
            assert all((r.type, r.term, r.transfer) == (r0.type, r0.term, r0.transfer) and
                       (r.index, r.log_term) == (n.group.log.last, n.last_term) for r in n.reqs)
            req_type[i] = r0.type | (R.CREQ_TRANSFER if r0.transfer else 0)
            req_term[i] = r0.term
            req_mask[i] = sum(1 << r.to for r in n.reqs)
        assert bool(n.reqs) == bool(cflags[i] & R.CFLAG_REQUESTS)
    return cflags, req_type, st


# ----------------------------------------------------------------- batches ---

def random_config(rng, ns):
    """(mask_in, mask_out) over ns slots: plain, joint, joint with an empty
    incoming half, or nobody votes."""
    vin = sum(int(x) << s for s, x in enumerate(rng.random(ns) < 0.7))
    vout = 0
    r = rng.random()
    if r < 0.25:
        vout = sum(int(x) << s for s, x in enumerate(rng.random(ns) < 0.5))
    elif r < 0.35:
        vout, vin = vin, 0
    elif r < 0.42:
        vin = 0
    return vin, vout


def _pick(rng, values):
    """One of ``values`` (kept as Python ints: rng.choice would go through
    float64 and round the 64-bit edges)."""
    return values[int(rng.integers(0, len(values)))]


def random_nodes(rng: np.random.Generator, G: int, readq_cap: int = 0):
    """Seeded ragged batch: 1..16 slots, learners, joint and empty configs,
    the own slot a voter / a learner / beyond the slots, every role with a
    random promotable bit, junk Progress, and the arithmetic's edges (term
    2^64 - 1, last_index around 2^40 and 2^63)."""
    nodes = []
    for _ in range(G):
        ns = int(rng.integers(1, 17))
        vin, vout = random_config(rng, ns)
        own = int(rng.integers(0, ns))
        r = rng.random()
        if r < 0.08:
            own = int(rng.choice([ns, 16, 0xFE, 0xFF]))
        elif r < 0.75:
            own = next((s for s in range(own, ns) if ((vin | vout) >> s) & 1), own)
        if rng.random() < 0.15:      # single voter (with or without learners)
            vin, vout = 1 << min(own, ns - 1), int(rng.choice([0, 0, 1 << min(own, ns - 1)]))
        term = _pick(rng, [1, 5, int(rng.integers(1, 1 << 40)), (1 << 64) - 1])
        last = _pick(rng, [0, 7, (1 << 40) - 1, 1 << 40, (1 << 63) - 1, 1 << 63,
                           int(rng.integers(0, 1 << 20))])
        committed = _pick(rng, [0, last, max(last - 3, 0), min(last + 1, L.M64)])
        role = int(rng.integers(0, 4)) | (R.ROLE_PROMOTABLE if rng.random() < 0.75 else 0)
        votes = {int(s): bool(rng.random() < 0.5) for s in range(ns) if rng.random() < 0.3}
        nodes.append(make_node(ns, vin, vout, own, self_id=int(rng.integers(1, 1 << 62)), term=term,
                               vote=int(rng.choice([0, 3, 9])), lead=int(rng.choice([0, 3, 9])),
                               role=role, last_index=last, last_term=int(rng.integers(0, 9)),
                               committed=committed, votes=votes, ee=int(rng.integers(0, 30)),
                               he=int(rng.integers(0, 5)), rng=rng, readq_cap=readq_cap))
    return nodes


def random_actions(rng: np.random.Generator, G: int, p_none: float = 0.2, p_bad: float = 0.03):
    a = rng.integers(1, 5, G).astype(np.uint8)
    a[rng.random(G) < 0.25] |= R.CAMP_PENDING_CONF
    a[rng.random(G) < p_none] = R.CAMP_NONE
    bad = rng.random(G) < p_bad
    a[bad] = rng.choice([5, 6, 0x7F, 0x85, 0xFF], int(bad.sum())).astype(np.uint8)
    return a
