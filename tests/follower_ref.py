"""CPU restatement of etcd's raft.Step for the non-leader inbox — TEST
INFRASTRUCTURE ONLY.

One node, one message at a time, over the fields qb_dev_follower_step owns.
Paths are relative to the reference's ``raft/``:

  Step: term filter                            raft.go:847-920
  Step: MsgVote / MsgPreVote                   raft.go:930-978
  stepLeader (no case for MsgHeartbeat / MsgTimeoutNow)  raft.go:991-1370
  stepCandidate MsgHeartbeat / MsgTimeoutNow   raft.go:1393-1395, 1415-1416
  stepFollower MsgHeartbeat / MsgTimeoutNow    raft.go:1437-1440, 1452-1457
  handleHeartbeat                              raft.go:1513-1516
  becomeFollower -> reset                      raft.go:686-693, 590-619
  hup (leader / unpromotable ignore it)        raft.go:760-768
  send (stamps Term on non-vote messages)      raft.go:386-418
  raftLog.commitTo / isUpToDate                log.go:236-244, 316-318

What is modelled of ``reset`` is its effect on the fields the engine's call
owns — Term, Vote, lead, state and the two elapsed counters; Progress, the
votes, readOnly, the transferee and the new randomized timeout stay the
host's.  Three records stop a group (the rest of its batch is not applied):
a message the host steps itself (HOST), the MsgTimeoutNow of a promotable
follower (the campaign is the host's; the term filter's effect is kept) and
a heartbeat whose commitTo would panic (nothing of it is applied).

Pinning: tests/golden/follower_tables.json holds the reference's own tests of
these paths transcribed as data; tests/test_follower_ref.py replays them here.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

# raft.go:39-45 StateType
FOLLOWER, CANDIDATE, LEADER, PRE_CANDIDATE = 0, 1, 2, 3
ROLE_PROMOTABLE = 0x80
NONE = 0  # raft.go:32

# record kinds / flags (include/quorum_batch.h QB_FIN_*, QB_FREC_FORCE)
HEARTBEAT, VOTE, PREVOTE, TIMEOUT_NOW, HOST = 0, 1, 2, 3, 4
FORCE = 0x80

# raftpb/raft.pb.go:76-94 MessageType
MSG_APP_RESP, MSG_VOTE_RESP, MSG_HEARTBEAT_RESP, MSG_PREVOTE_RESP = 4, 6, 9, 18
REJECT = 0x80

FFLAG_HOST_MSG, FFLAG_CAMPAIGN, FFLAG_COMMIT_RANGE = 0x01, 0x02, 0x04
FFLAG_RESET, FFLAG_HARDSTATE = 0x08, 0x10
FFLAG_STOPS = FFLAG_HOST_MSG | FFLAG_CAMPAIGN | FFLAG_COMMIT_RANGE

FSTAT_NAMES = ("heartbeats", "granted", "rejected", "lease_dropped", "stale_ignored",
               "stale_answered", "role_ignored", "became_follower", "after_stop", "bad_group",
               "bad_kind")
NO_STOP = 0xFFFFFFFF


@dataclass
class Node:
    """A raft node as the follower step sees it."""
    term: int = 0
    vote: int = NONE
    lead: int = NONE
    committed: int = 0
    last_index: int = 0
    last_term: int = 0
    role: int = FOLLOWER           # StateType | ROLE_PROMOTABLE
    election_elapsed: int = 0
    heartbeat_elapsed: int = 0

    @property
    def state(self) -> int:
        return self.role & 3


@dataclass
class Rec:
    kind: int
    frm: int = 0
    term: int = 0
    index: int = 0     # votes: Index; heartbeat: Commit
    aux: int = 0       # votes: LogTerm; heartbeat: context id
    force: bool = False


@dataclass
class Config:
    election_timeout: int = 10
    check_quorum: bool = False
    pre_vote: bool = False


def _become_follower(n: Node, term: int, lead: int, st: dict) -> int:
    """becomeFollower(term, lead) -> reset(term), raft.go:686-693, 590-619."""
    if n.term != term:                     # raft.go:591-594
        n.term = term
        n.vote = NONE
    n.lead = NONE                          # raft.go:595
    n.election_elapsed = 0                 # raft.go:597
    n.heartbeat_elapsed = 0                # raft.go:598
    n.lead = lead                          # raft.go:690
    n.role = n.role & ~3 | FOLLOWER        # raft.go:691
    st["became_follower"] += 1
    return FFLAG_RESET


def _is_up_to_date(n: Node, lasti: int, term: int) -> bool:
    """log.go:316-318."""
    return term > n.last_term or (term == n.last_term and lasti >= n.last_index)


def step(n: Node, m: Rec, cfg: Config, st: dict) -> Tuple[int, int, int]:
    """One raft.Step(m).  Returns (resp_type, resp_term, flags): resp_type 0 =
    no message; flags = FFLAG_RESET and / or the stop reason.  A record that
    stops with HOST_MSG or COMMIT_RANGE leaves the node untouched."""
    if m.kind == HOST:
        return 0, 0, FFLAG_HOST_MSG
    is_vote = m.kind in (VOTE, PREVOTE)
    gf = 0
    if m.term == 0:                                      # raft.go:850-851: local message
        pass
    elif m.term > n.term:                                # raft.go:852
        if is_vote:                                      # raft.go:853-863
            in_lease = (cfg.check_quorum and n.lead != NONE
                        and n.election_elapsed < cfg.election_timeout)
            if not m.force and in_lease:
                st["lease_dropped"] += 1
                return 0, 0, 0
        if m.kind == HEARTBEAT and n.committed < m.index and n.last_index < m.index:
            return 0, 0, FFLAG_COMMIT_RANGE              # log.go:236-244 would panic
        if m.kind == PREVOTE:                            # raft.go:865-866
            pass
        elif m.kind == HEARTBEAT:                        # raft.go:876-877
            gf |= _become_follower(n, m.term, m.frm, st)
        else:                                            # raft.go:878-880
            gf |= _become_follower(n, m.term, NONE, st)
    elif m.term < n.term:                                # raft.go:883-919
        if (cfg.check_quorum or cfg.pre_vote) and m.kind == HEARTBEAT:
            st["stale_answered"] += 1
            return MSG_APP_RESP, n.term, 0               # raft.go:906; send: Term = r.Term
        if m.kind == PREVOTE:                            # raft.go:907-913
            st["stale_answered"] += 1
            return MSG_PREVOTE_RESP | REJECT, n.term, 0
        st["stale_ignored"] += 1
        return 0, 0, 0

    if is_vote:                                          # raft.go:930-978
        can_vote = (n.vote == m.frm or (n.vote == NONE and n.lead == NONE)
                    or (m.kind == PREVOTE and m.term > n.term))
        rt = MSG_VOTE_RESP if m.kind == VOTE else MSG_PREVOTE_RESP
        if can_vote and _is_up_to_date(n, m.index, m.aux):
            if m.kind == VOTE:                           # raft.go:969-973
                n.election_elapsed = 0
                n.vote = m.frm
            st["granted"] += 1
            return rt, m.term, gf                        # raft.go:968
        st["rejected"] += 1
        return rt | REJECT, n.term, gf                   # raft.go:977

    if m.kind == HEARTBEAT:
        if n.state == LEADER:                            # stepLeader: no case
            st["role_ignored"] += 1
            return 0, 0, gf
        if n.committed < m.index and n.last_index < m.index:
            assert gf == 0
            return 0, 0, FFLAG_COMMIT_RANGE              # log.go:236-244 would panic
        if n.state in (CANDIDATE, PRE_CANDIDATE):        # raft.go:1393-1395
            gf |= _become_follower(n, m.term, m.frm, st)
        else:                                            # raft.go:1437-1440
            n.election_elapsed = 0
            n.lead = m.frm
        if n.committed < m.index:                        # commitTo, log.go:236-244
            n.committed = m.index
        st["heartbeats"] += 1
        return MSG_HEARTBEAT_RESP, n.term, gf            # raft.go:1515; send: Term = r.Term

    assert m.kind == TIMEOUT_NOW
    if n.state == FOLLOWER and (n.role & ROLE_PROMOTABLE):   # raft.go:1452-1457 -> 760-768
        return 0, 0, gf | FFLAG_CAMPAIGN                 # hup(campaignTransfer) is the host's
    st["role_ignored"] += 1                              # raft.go:1415-1416; stepLeader: no case
    return 0, 0, gf


def new_stats() -> dict:
    return {k: 0 for k in FSTAT_NAMES}


def step_batch(nodes: List[Node], recs: List[Tuple[int, Optional[Rec]]], cfg: Config,
               st: Optional[dict] = None):
    """A batch of (group, Rec) in arrival order over ``nodes`` (in place).  A
    record with group >= len(nodes) is a bad group; a Rec whose kind is above
    HOST a bad kind (both dropped).  Returns (resp_type [M], resp_term [M],
    stop_at [G], gflags [G], stats)."""
    st = new_stats() if st is None else st
    G = len(nodes)
    resp_type, resp_term = [0] * len(recs), [0] * len(recs)
    stop_at, gflags = [NO_STOP] * G, [0] * G
    hard0 = [(n.term, n.vote, n.committed) for n in nodes]
    for i, (g, m) in enumerate(recs):
        if not 0 <= g < G:
            st["bad_group"] += 1
            continue
        if m.kind > HOST:
            st["bad_kind"] += 1
            continue
        if stop_at[g] != NO_STOP:
            st["after_stop"] += 1
            continue
        rt, rterm, gf = step(nodes[g], m, cfg, st)
        resp_type[i], resp_term[i] = rt, rterm
        gflags[g] |= gf
        if gf & FFLAG_STOPS:
            stop_at[g] = i
    for g, n in enumerate(nodes):
        if (n.term, n.vote, n.committed) != hard0[g]:
            gflags[g] |= FFLAG_HARDSTATE
    return resp_type, resp_term, stop_at, gflags, st
