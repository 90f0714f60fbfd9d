"""CPU restatement of etcd's campaign path — TEST INFRASTRUCTURE ONLY.

One node's Step(MsgHup) and election outcomes over
``oracle.leader_ref.LeaderGroup`` / ``Progress`` (the Progress map, the config
masks, ``term``, ``leader_slot`` = the node's own slot, ``transferee``,
``readq``, ``log.last`` / ``log.committed``) plus the election's own fields
(``CampaignNode``).  Paths are relative to the reference's ``raft/``:

  reset                                        raft.go:590-619
  appendEntry (MaybeUpdate, maybeCommit)       raft.go:621-642
  becomeFollower / becomeCandidate /
    becomePreCandidate / becomeLeader          raft.go:686-758
  Step MsgHup / hup / campaign / poll          raft.go:923-928, 760-845
  stepCandidate's decision                     raft.go:1399-1414
  stepFollower MsgTimeoutNow                   raft.go:1452-1457
  promotable                                   raft.go:1618-1621
  bcastAppend / maybeSendAppend                raft.go:515-522, 432-492
  Progress.BecomeReplicate / MaybeUpdate       tracker/progress.go:133-157
  RecordVote / TallyVotes / ResetVotes         tracker/tracker.go:246-288
  MajorityConfig.CommittedIndex / JointConfig  quorum/majority.go:126-172, joint.go:49-57

What is modelled is every field the engine's arrays hold.  The log is the
host's: becomeLeader's empty entry is not appended here (``log.last`` and
``last_term`` keep their values at entry; the entry's index, last + 1, is what
MaybeUpdate and maybeCommit see), and ``pendingConfIndex``, uncommittedSize,
the new randomized timeout and the readOnly contents beyond the queue's
length are not held.  hup's look at the unapplied entries (raft.go:770-777)
is an input, ``pending_conf``.

Pinning: tests/golden/campaign_tables.json holds the reference's own tests of
this path transcribed as data; tests/test_campaign_ref.py replays them here.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List

from oracle import leader_ref as L
from oracle import quorum_ref as Q

# raft.go:39-45 StateType
FOLLOWER, CANDIDATE, LEADER, PRE_CANDIDATE = 0, 1, 2, 3
ROLE_PROMOTABLE = 0x80
NONE = 0  # raft.go:32

# include/quorum_batch.h QB_CAMP_*
CAMP_NONE, CAMP_HUP, CAMP_TRANSFER, CAMP_WON, CAMP_LOST = 0, 1, 2, 3, 4
CAMP_PENDING_CONF = 0x80

MSG_VOTE, MSG_PREVOTE = 5, 17  # raftpb/raft.pb.go:76-94
CREQ_TRANSFER = 0x80

CFLAG_REQUESTS, CFLAG_BECAME_LEADER, CFLAG_BCAST_APPEND = 0x01, 0x02, 0x04
CFLAG_RESET, CFLAG_HARDSTATE, CFLAG_IGNORED = 0x08, 0x10, 0x20

CSTAT_NAMES = ("pre_campaigns", "campaigns", "became_leader", "became_follower", "vote_requests",
               "ignored_leader", "ignored_unpromotable", "ignored_pending_conf", "ignored_role",
               "bad_action")

PRE_ELECTION, ELECTION, TRANSFER = "CampaignPreElection", "CampaignElection", "CampaignTransfer"


@dataclass
class Request:
    """A vote request in the order the reference emits it."""
    type: int          # MSG_VOTE / MSG_PREVOTE
    to: int            # slot
    term: int
    index: int
    log_term: int
    transfer: bool     # Context == "CampaignTransfer"

    def key(self):
        return (self.type, self.to, self.term, self.index, self.log_term, self.transfer)


@dataclass
class CampaignNode:
    """A raft node as the campaign sees it.  ``group.leader_slot`` is the
    node's own slot in every role; ``votes`` is ProgressTracker.Votes by slot."""
    group: L.LeaderGroup
    self_id: int
    role: int                      # StateType | ROLE_PROMOTABLE
    vote: int = NONE
    lead: int = NONE
    last_term: int = 0
    election_elapsed: int = 0
    heartbeat_elapsed: int = 0
    votes: Dict[int, bool] = field(default_factory=dict)
    reqs: List[Request] = field(default_factory=list)

    @property
    def state(self) -> int:
        return self.role & 3

    @property
    def own(self) -> int:
        return self.group.leader_slot


def promotable(n: CampaignNode) -> bool:
    """raft.go:1618-1621; hasPendingSnapshot is the host's part of the
    ROLE_PROMOTABLE bit."""
    g = n.group
    has_progress = n.own < g.n_slots
    return bool(n.role & ROLE_PROMOTABLE) and has_progress and \
        bool(((g.mask_in | g.mask_out) >> n.own) & 1)


def _reset(n: CampaignNode, term: int) -> None:
    """raft.go:590-619."""
    g = n.group
    if g.term != term:                      # raft.go:591-594
        g.term = term
        n.vote = NONE
    n.lead = NONE                           # raft.go:595
    n.election_elapsed = 0                  # raft.go:597
    n.heartbeat_elapsed = 0                 # raft.go:598
    g.transferee = L.NO_SLOT                # raft.go:601
    n.votes = {}                            # raft.go:603
    for s, p in enumerate(g.prs):           # raft.go:604-614
        # NewInflights: an empty ring; the engine leaves the dead buffer as it is
        ring = L.Inflights(p.inflights.size, 0, 0, p.inflights.buffer)
        g.prs[s] = L.Progress(match=g.log.last if s == n.own else 0,
                              next=(g.log.last + 1) & L.M64, inflights=ring,
                              is_learner=p.is_learner)
    g.readq = []                            # raft.go:618


def _poll_self(n: CampaignNode) -> int:
    """poll(r.id, ..., true), raft.go:837-845.  The engine's votes word has 16
    slots: an own slot beyond them records nothing."""
    if n.own < 16 and n.own not in n.votes:  # tracker.go:258-263
        n.votes[n.own] = True
    g = n.group
    return Q.tally_votes_slots(g.mask_in, g.mask_out, n.votes)[2]


def _become_follower(n: CampaignNode, term: int, lead: int, st: dict) -> int:
    """raft.go:686-693."""
    _reset(n, term)
    n.lead = lead
    n.role = n.role & ~3 | FOLLOWER
    st["became_follower"] += 1
    return CFLAG_RESET


def _become_pre_candidate(n: CampaignNode, st: dict) -> None:
    """raft.go:708-722."""
    assert n.state != LEADER
    n.votes = {}                            # raft.go:717
    n.lead = NONE                           # raft.go:719
    n.role = n.role & ~3 | PRE_CANDIDATE
    st["pre_campaigns"] += 1


def _become_candidate(n: CampaignNode, st: dict) -> int:
    """raft.go:695-706."""
    assert n.state != LEADER
    _reset(n, (n.group.term + 1) & L.M64)
    n.vote = n.self_id
    n.role = n.role & ~3 | CANDIDATE
    st["campaigns"] += 1
    return CFLAG_RESET


def _committed_with_new_entry(n: CampaignNode, li: int) -> int:
    """ProgressTracker.Committed (tracker.go:177-180) over the fresh Progress
    map with the own slot at li: majority.go:126-172 per half, joint.go:49-57."""
    g = n.group

    def half(mask):
        ids = [s for s in range(16) if (mask >> s) & 1]
        if not ids:
            return L.MAX_U64                # majority.go:128-132
        srt = sorted(g.prs[s].match if s < g.n_slots else 0 for s in ids)
        return srt[len(ids) - (len(ids) // 2 + 1)]
    return min(half(g.mask_in), half(g.mask_out))


def _become_leader(n: CampaignNode, st: dict) -> int:
    """raft.go:724-758 with appendEntry (raft.go:621-642)."""
    assert n.state != FOLLOWER
    g = n.group
    _reset(n, g.term)
    n.lead = n.self_id
    n.role = n.role & ~3 | LEADER
    li = (g.log.last + 1) & L.M64           # the empty entry's index, raft.go:625
    if n.own < g.n_slots:
        g.prs[n.own].become_replicate()     # raft.go:738
        g.prs[n.own].maybe_update(li)       # raft.go:638
    mci = _committed_with_new_entry(n, li)  # raft.go:640 -> 585-588
    # log.go:328-334: the entry at li carries r.Term; no other index does for
    # sure, and MaxUint64 (no voter at all) has no term
    if mci == li and mci > g.log.committed:
        g.log.committed = mci
    st["became_leader"] += 1
    return CFLAG_RESET | CFLAG_BECAME_LEADER


def _bcast_append(n: CampaignNode) -> int:
    """raft.go:515-522 -> maybeSendAppend (raft.go:432-492): a fresh Progress
    probes and is not paused; the one entry goes out and ProbeSent is set."""
    for s, p in enumerate(n.group.prs):
        if s == n.own:
            continue
        assert p.state == L.STATE_PROBE and not p.is_paused()
        p.probe_sent = True                 # raft.go:486-487
    return CFLAG_BCAST_APPEND


def _campaign(n: CampaignNode, t: str, st: dict) -> int:
    """raft.go:785-835."""
    g = n.group
    cf = 0
    if t == PRE_ELECTION:
        _become_pre_candidate(n, st)
        vote_msg, term = MSG_PREVOTE, (g.term + 1) & L.M64   # raft.go:797
    else:
        cf |= _become_candidate(n, st)
        vote_msg, term = MSG_VOTE, g.term
    if _poll_self(n) == Q.VOTE_WON:         # raft.go:803-812
        if t == PRE_ELECTION:
            return cf | _campaign(n, ELECTION, st)
        return cf | _become_leader(n, st)
    voters = g.mask_in | g.mask_out
    for s in range(16):                     # raft.go:813-834: ascending IDs
        if not (voters >> s) & 1 or s == n.own:
            continue
        n.reqs.append(Request(vote_msg, s, term, g.log.last, n.last_term, t == TRANSFER))
        st["vote_requests"] += 1
    return cf | CFLAG_REQUESTS


def _hup(n: CampaignNode, t: str, pending_conf: bool, st: dict) -> int:
    """raft.go:760-781."""
    if n.state == LEADER:                   # raft.go:761-764
        st["ignored_leader"] += 1
        return CFLAG_IGNORED
    if not promotable(n):                   # raft.go:766-769
        st["ignored_unpromotable"] += 1
        return CFLAG_IGNORED
    if pending_conf:                        # raft.go:770-777
        st["ignored_pending_conf"] += 1
        return CFLAG_IGNORED
    return _campaign(n, t, st)


def new_stats() -> dict:
    return {k: 0 for k in CSTAT_NAMES}


def step(n: CampaignNode, action: int, pre_vote: bool, st: dict) -> int:
    """One action byte on one node; the requests go to ``n.reqs`` (cleared
    first).  Returns the CFLAG_* of the call."""
    g = n.group
    n.reqs = []
    code, pending = action & 0x7F, bool(action & CAMP_PENDING_CONF)
    if code > CAMP_LOST:
        st["bad_action"] += 1
        return 0
    if code == CAMP_NONE:
        return 0
    hard0 = (g.term, n.vote, g.log.committed)
    if code == CAMP_HUP:                    # raft.go:923-928
        cf = _hup(n, PRE_ELECTION if pre_vote else ELECTION, pending, st)
    elif code == CAMP_TRANSFER:             # raft.go:1452-1457
        cf = _hup(n, TRANSFER, pending, st)
    elif n.state not in (CANDIDATE, PRE_CANDIDATE):
        st["ignored_role"] += 1
        cf = CFLAG_IGNORED
    elif code == CAMP_WON:                  # raft.go:1402-1409
        if n.state == PRE_CANDIDATE:
            cf = _campaign(n, ELECTION, st)
        else:
            cf = _become_leader(n, st)
            cf |= _bcast_append(n)
    else:                                   # raft.go:1410-1413
        cf = _become_follower(n, g.term, NONE, st)
    if (g.term, n.vote, g.log.committed) != hard0:
        cf |= CFLAG_HARDSTATE
    return cf
