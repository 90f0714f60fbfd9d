"""CPU restatement of etcd's raft.tick() — TEST INFRASTRUCTURE ONLY.

One node's tick over ``oracle.leader_ref.LeaderGroup`` / ``Progress`` (the
group's Progress map with ``is_learner`` / ``recent_active``, ``transferee``,
``readq``, ``log.committed``, ``leader_slot``) plus the tick's own fields
(``TickNode``).  Paths are relative to the reference's ``raft/``:

  tickElection / tickHeartbeat                 raft.go:645-684
  stepLeader MsgBeat / MsgCheckQuorum          raft.go:994-1018
  sendHeartbeat / bcastHeartbeat[WithCtx]      raft.go:495-541
  becomeFollower -> reset (the tick's fields)  raft.go:590-619, 686-693
  promotable                                   raft.go:1618-1621
  pastElectionTimeout / abortLeaderTransfer    raft.go:1714-1728
  ProgressTracker.Visit / QuorumActive         tracker/tracker.go:191-225
  MajorityConfig.VoteResult / JointConfig      quorum/majority.go:178-210, joint.go:61-75
  readOnly.lastPendingRequestCtx               read_only.go:116-121

What is modelled of ``reset`` is its effect on the fields the engine's tick
owns — state, the two elapsed counters, leadTransferee and the RecentActive
flag of every Progress — and nothing else: Match / Next / Inflights, readOnly,
the votes, lead and the new randomized timeout stay the host's (as
``stepdown_at`` is for the leader step).  The campaign of an election timeout
(Step MsgHup, raft.go:650) is the host's too: the tick reports it as a flag.

Pinning: tests/golden/tick_tables.json holds the reference's own tests of
this path transcribed as data; tests/test_tick_ref.py replays them here.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List

from oracle import leader_ref as L

# raft.go:39-45 StateType
FOLLOWER, CANDIDATE, LEADER, PRE_CANDIDATE = 0, 1, 2, 3
ROLE_PROMOTABLE = 0x80

MSG_HEARTBEAT = 8  # raftpb/raft.pb.go:84

TFLAG_HUP, TFLAG_BEAT, TFLAG_STEPPED_DOWN = 0x01, 0x02, 0x04
TFLAG_CHECK_QUORUM, TFLAG_TRANSFER_ABORTED = 0x08, 0x10

TSTAT_NAMES = ("leaders", "non_leaders", "beats", "heartbeats", "check_quorum", "stepped_down",
               "transfer_aborted", "hups")

M32 = (1 << 32) - 1  # the engine's counters are uint32


@dataclass
class TickNode:
    """A raft node as the tick sees it."""
    group: L.LeaderGroup
    role: int                  # StateType | ROLE_PROMOTABLE
    election_elapsed: int = 0
    heartbeat_elapsed: int = 0
    rand_timeout: int = 0      # randomizedElectionTimeout (set by the host)
    msgs: List[L.Msg] = field(default_factory=list)

    @property
    def state(self) -> int:
        return self.role & 3


def mark_learners(g: L.LeaderGroup) -> None:
    """Progress.IsLearner from the config: a slot in neither voter half."""
    for s, p in enumerate(g.prs):
        p.is_learner = not (((g.mask_in | g.mask_out) >> s) & 1)


def _vote_result(mask: int, votes: dict) -> int:
    """majority.go:178-210 over the slots of ``mask``."""
    ids = [s for s in range(16) if (mask >> s) & 1]
    if not ids:
        return 3  # an empty config wins, majority.go:179-184
    yes = sum(1 for s in ids if votes.get(s) is True)
    missing = sum(1 for s in ids if s not in votes)
    q = len(ids) // 2 + 1
    if yes >= q:
        return 3
    if yes + missing >= q:
        return 1
    return 2


def quorum_active(g: L.LeaderGroup) -> bool:
    """tracker.go:215-225."""
    votes = {}
    for s, p in enumerate(g.prs):          # Visit, tracker.go:191-212
        if p.is_learner:                   # tracker.go:218-220
            continue
        votes[s] = p.recent_active
    r1, r2 = _vote_result(g.mask_in, votes), _vote_result(g.mask_out, votes)
    if r1 == r2:                           # joint.go:61-75
        return r1 == 3
    return False


def _become_follower(n: TickNode) -> None:
    """becomeFollower(r.Term, None) -> reset(r.Term) (raft.go:686-693,
    590-619), the tick's fields only."""
    n.role = n.role & ~3 | FOLLOWER        # raft.go:691
    n.election_elapsed = 0                 # raft.go:597
    n.heartbeat_elapsed = 0                # raft.go:598
    n.group.transferee = L.NO_SLOT         # raft.go:601 abortLeaderTransfer
    for p in n.group.prs:                  # raft.go:604-614: a fresh Progress
        p.recent_active = False


def _bcast_heartbeat(n: TickNode) -> None:
    """raft.go:524-541, 495-511."""
    g = n.group
    ctx = g.readq[-1].ctx if g.readq else 0     # read_only.go:116-121
    for s, p in enumerate(g.prs):               # Visit: ascending IDs
        if s == g.leader_slot:                  # raft.go:535-537
            continue
        commit = min(p.match, g.log.committed)  # raft.go:502
        n.msgs.append(L.Msg(MSG_HEARTBEAT, s, commit=commit, aux=ctx))


def _check_quorum(n: TickNode) -> None:
    """stepLeader MsgCheckQuorum, raft.go:997-1018."""
    g = n.group
    if g.leader_slot < g.n_slots:               # raft.go:1004-1006
        g.prs[g.leader_slot].recent_active = True
    if not quorum_active(g):                    # raft.go:1007-1010
        _become_follower(n)
    for s, p in enumerate(g.prs):               # raft.go:1013-1017
        if s != g.leader_slot:
            p.recent_active = False


def tick(n: TickNode, election_timeout: int, heartbeat_timeout: int, check_quorum: bool) -> int:
    """One raft.tick(); appends the heartbeats to ``n.msgs`` and returns the
    TFLAG_* of what fired."""
    g = n.group
    mark_learners(g)
    tf = 0
    if n.state != LEADER:                       # tickElection, raft.go:645-654
        n.election_elapsed = (n.election_elapsed + 1) & M32
        if (n.role & ROLE_PROMOTABLE) and n.election_elapsed >= n.rand_timeout:  # raft.go:648
            n.election_elapsed = 0
            tf |= TFLAG_HUP                     # raft.go:650: Step(MsgHup) is the host's
        return tf
    n.heartbeat_elapsed = (n.heartbeat_elapsed + 1) & M32   # raft.go:658
    n.election_elapsed = (n.election_elapsed + 1) & M32     # raft.go:659
    if n.election_elapsed >= election_timeout:  # raft.go:661
        n.election_elapsed = 0
        if check_quorum:                        # raft.go:663-667
            tf |= TFLAG_CHECK_QUORUM
            _check_quorum(n)
            if n.state != LEADER:
                tf |= TFLAG_STEPPED_DOWN
        if n.state == LEADER and g.transferee != L.NO_SLOT:  # raft.go:669-671
            g.transferee = L.NO_SLOT
            tf |= TFLAG_TRANSFER_ABORTED
    if n.state != LEADER:                       # raft.go:674-676
        return tf
    if n.heartbeat_elapsed >= heartbeat_timeout:  # raft.go:678
        n.heartbeat_elapsed = 0
        tf |= TFLAG_BEAT
        _bcast_heartbeat(n)                     # raft.go:680 -> 994-996
    return tf


def stats_of(tflags, roles_before, n_msgs) -> dict:
    """The engine's QB_TSTAT_* counters of one tick over a batch."""
    lead = sum(1 for r in roles_before if (r & 3) == LEADER)
    return {"leaders": lead, "non_leaders": len(roles_before) - lead,
            "beats": sum(1 for f in tflags if f & TFLAG_BEAT), "heartbeats": n_msgs,
            "check_quorum": sum(1 for f in tflags if f & TFLAG_CHECK_QUORUM),
            "stepped_down": sum(1 for f in tflags if f & TFLAG_STEPPED_DOWN),
            "transfer_aborted": sum(1 for f in tflags if f & TFLAG_TRANSFER_ABORTED),
            "hups": sum(1 for f in tflags if f & TFLAG_HUP)}
