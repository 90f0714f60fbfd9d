"""CPU restatement of etcd's proposal path — TEST INFRASTRUCTURE ONLY.

One node's Step(MsgProp) and the log's share of becomeLeader, statement by
statement as Go has them, on top of tests/campaign_ref.py's ``CampaignNode``
(role, lead, the Progress map, the config masks, the transferee).  Paths are
relative to the reference's ``raft/``:

  stepLeader MsgProp                           raft.go:1019-1077
  stepCandidate / stepFollower MsgProp         raft.go:1387-1389, 1423-1430
  appendEntry                                  raft.go:621-642
  increaseUncommittedSize                      raft.go:1761-1779
  becomeLeader's log share                     raft.go:745-756
  maybeSendAppend / bcastAppend                raft.go:432-492, 515-522
  maybeCommit                                  raft.go:585-588, log.go:328-334
  raftLog.term / entries                       log.go:268-299
  Progress / Inflights                         tracker/progress.go, inflights.go
  MajorityConfig.CommittedIndex / JointConfig  quorum/majority.go:126-172, joint.go:49-57

The log is a plain list of terms, one per entry: ``terms[k]`` is the term of
index ``first - 1 + k`` (``terms[0]`` the dummy entry's), as in
tests/append_ref.py.  The engine's run table appears only at the edges
(``sync`` derives ``log.runs`` for packing), so nothing here shares the
kernel's run arithmetic.

A proposal is tried on the node directly; the two stops (an empty MsgProp,
where Go panics, and a log that would need a 9th term run) are found before
anything is applied, as the engine reports them.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Tuple

from oracle import leader_ref as L
from tests import campaign_ref as CR
from tests.append_ref import runs_of

U64 = (1 << 64) - 1
MAX_RUNS = 8
FOLLOWER, CANDIDATE, LEADER, PRE_CANDIDATE = 0, 1, 2, 3

PROP_NONE, PROP_ENTRIES, PROP_LEADER_ENTRY = 0, 1, 2
PROP_CONF_CHANGE, PROP_CC_LEAVE_JOINT = 0x40, 0x80
MSG_APP, MSG_SNAP = 3, 7
PFLAG_APPENDED, PFLAG_BCAST, PFLAG_COMMITTED, PFLAG_DROPPED = 0x01, 0x02, 0x04, 0x08
PFLAG_FORWARD, PFLAG_CC_REFUSED, PFLAG_LOG_RUNS, PFLAG_BAD = 0x10, 0x20, 0x40, 0x80
PSTAT_NAMES = ("proposals", "entries", "drop_no_progress", "drop_transfer", "drop_size",
               "drop_no_leader", "drop_forwarding", "drop_candidate", "forwarded", "cc_accepted",
               "cc_refused", "msg_app", "msg_snap", "commits", "leader_entries", "log_runs",
               "empty", "ignored_role", "bad_action")


@dataclass
class Config:
    max_uncommitted_size: int = 0          # 0: noLimit (Config.validate)
    disable_proposal_forwarding: bool = False


@dataclass
class ProposeNode:
    """A raft node as a proposal sees it: the campaign's node (``camp.group``
    holds the Progress map, masks, term, own slot, transferee and the log
    view's first / committed / snapshot / max_ents) plus the log's terms and
    the three words of the proposal path."""
    camp: CR.CampaignNode
    terms: List[int] = field(default_factory=lambda: [0])   # [first - 1 .. last]
    applied: int = 0
    uncommitted_size: int = 0
    pending_conf_index: int = 0

    @property
    def group(self) -> L.LeaderGroup:
        return self.camp.group

    @property
    def first(self) -> int:
        return self.camp.group.log.first

    @property
    def last(self) -> int:
        return (self.first - 1 + len(self.terms) - 1) & U64

    def sync(self) -> None:
        """The derived words the engine's arrays hold: last_index, last_term
        and the run table."""
        log = self.camp.group.log
        log.last = self.last
        self.camp.last_term = self.terms[-1]
        starts, rterms = runs_of(self.terms, log.first)
        log.runs = list(zip(starts, rterms))

    # raftLog.term, log.go:268-288 (+ zeroTermOnErrCompacted)
    def log_term(self, i: int) -> int:
        dummy = self.first - 1
        if i < dummy or i > self.last:
            return 0
        return self.terms[i - dummy]

    # raftLog.entries, log.go:290-299 -> slice: (count, compacted)
    def entries(self, lo: int) -> Tuple[int, bool]:
        if lo > self.last:
            return 0, False
        if lo < self.first:
            return 0, True
        return min(self.camp.group.log.max_ents, self.last - lo + 1), False


def new_node(camp: CR.CampaignNode, terms: List[int], **kw) -> ProposeNode:
    n = ProposeNode(camp, list(terms), **kw)
    n.sync()
    return n


def new_stats() -> dict:
    return {k: 0 for k in PSTAT_NAMES}


def _committed_index(g: L.LeaderGroup) -> int:
    """tracker.go:177-179 -> joint.go:49-57 -> majority.go:126-172."""
    def half(mask):
        ids = [s for s in range(g.n_slots) if (mask >> s) & 1]
        if not ids:
            return U64
        srt = sorted(g.prs[s].match for s in ids)
        return srt[len(ids) - (len(ids) // 2 + 1)]
    return min(half(g.mask_in), half(g.mask_out))


def _maybe_commit(n: ProposeNode) -> bool:
    """raft.go:585-588, log.go:328-334."""
    log = n.group.log
    mci = _committed_index(n.group)
    if mci > log.committed and n.log_term(mci) == n.group.term:
        log.committed = mci
        return True
    return False


def _maybe_send_append(n: ProposeNode, to: int, msgs: list, st: dict) -> bool:
    """raft.go:432-492 with sendIfEmpty = true."""
    g = n.group
    pr = g.prs[to]
    if pr.is_paused():
        return False
    term = n.log_term((pr.next - 1) & U64)
    cnt, compacted = n.entries(pr.next)
    if compacted:
        if not pr.recent_active:
            return False
        if g.log.snap_index == 0:            # ErrSnapshotTemporarilyUnavailable
            return False
        msgs.append((MSG_SNAP, to, g.log.snap_index, g.log.snap_term, 0, 0))
        pr.become_snapshot(g.log.snap_index)
        st["msg_snap"] += 1
        return True
    msgs.append((MSG_APP, to, (pr.next - 1) & U64, term, None, cnt))   # Commit: filled in below
    if cnt != 0:
        if pr.state == L.STATE_REPLICATE:
            last = (pr.next + cnt - 1) & U64
            pr.optimistic_update(last)
            pr.inflights.add(last)
        elif pr.state == L.STATE_PROBE:
            pr.probe_sent = True
        else:
            raise AssertionError("sending append in unhandled state")
    st["msg_app"] += 1
    return True


def _append(n: ProposeNode, cnt: int) -> None:
    """raftLog.append: cnt entries of the leader's term."""
    n.terms += [n.group.term] * cnt
    n.sync()


def _needs_ninth_run(n: ProposeNode) -> bool:
    return n.terms[-1] != n.group.term and len(n.group.log.runs) >= MAX_RUNS


def step(n: ProposeNode, action: int, n_ents: int, payload: int, cc_at: int, cc_payload: int,
         cfg: Config, st: dict):
    """One action byte on one node.  Returns (pflags, msgs): msgs are (type,
    to, index, log_term, commit, n) in the order bcastAppend emits them."""
    c, g = n.camp, n.group
    code = action & 0x3F
    if code > PROP_LEADER_ENTRY:
        st["bad_action"] += 1
        return 0, []
    if code == PROP_NONE:
        return 0, []
    if code == PROP_LEADER_ENTRY:                                # raft.go:745-756
        if c.state != LEADER:
            st["ignored_role"] += 1
            return 0, []
        if _needs_ninth_run(n):
            st["log_runs"] += 1
            return PFLAG_LOG_RUNS, []
        n.pending_conf_index = n.last                            # raft.go:745
        _append(n, 1)                                            # raft.go:748 (s == 0: never refused)
        n.uncommitted_size = 0                                   # raft.go:756 behind reset
        st["leader_entries"] += 1
        st["entries"] += 1
        return PFLAG_APPENDED, []
    # Step(MsgProp): local, Term 0, so the term filter passes it
    if c.state == FOLLOWER:                                      # raft.go:1423-1430
        if c.lead == CR.NONE:
            st["drop_no_leader"] += 1
            return PFLAG_DROPPED, []
        if cfg.disable_proposal_forwarding:
            st["drop_forwarding"] += 1
            return PFLAG_DROPPED, []
        st["forwarded"] += 1
        return PFLAG_FORWARD, []
    if c.state in (CANDIDATE, PRE_CANDIDATE):                    # raft.go:1387-1389
        st["drop_candidate"] += 1
        return PFLAG_DROPPED, []
    if n_ents == 0:                                              # raft.go:1020-1022: panic
        st["empty"] += 1
        return PFLAG_BAD, []
    if c.own >= g.n_slots:                                       # raft.go:1023-1028
        st["drop_no_progress"] += 1
        return PFLAG_DROPPED, []
    if g.transferee != L.NO_SLOT:                                # raft.go:1029-1032
        st["drop_transfer"] += 1
        return PFLAG_DROPPED, []
    if _needs_ninth_run(n):
        st["log_runs"] += 1
        return PFLAG_LOG_RUNS, []
    pf = 0
    s = payload
    for i in range(n_ents) if (action & PROP_CONF_CHANGE) and cc_at < n_ents else ():
        if i != cc_at:                                           # the one conf-change entry
            continue
        already_pending = n.pending_conf_index > n.applied      # raft.go:1051
        already_joint = g.mask_out != 0                          # raft.go:1052
        wants_leave_joint = bool(action & PROP_CC_LEAVE_JOINT)   # raft.go:1053
        refused = already_pending or (already_joint and not wants_leave_joint) or \
            (not already_joint and wants_leave_joint)
        if refused:                                              # raft.go:1064-1066
            pf |= PFLAG_CC_REFUSED
            s = (payload - cc_payload) & U64
            st["cc_refused"] += 1
        else:                                                    # raft.go:1068
            n.pending_conf_index = (n.last + i + 1) & U64
            st["cc_accepted"] += 1
    # appendEntry -> increaseUncommittedSize, raft.go:1761-1779
    limit = cfg.max_uncommitted_size or U64
    if n.uncommitted_size > 0 and s > 0 and ((n.uncommitted_size + s) & U64) > limit:
        st["drop_size"] += 1
        return pf | PFLAG_DROPPED, []
    n.uncommitted_size = (n.uncommitted_size + s) & U64
    _append(n, n_ents)                                           # raft.go:637
    pf |= PFLAG_APPENDED
    st["proposals"] += 1
    st["entries"] += n_ents
    g.prs[c.own].maybe_update(n.last)                            # raft.go:638
    if _maybe_commit(n):                                         # raft.go:640
        pf |= PFLAG_COMMITTED
        st["commits"] += 1
    msgs: list = []
    for to in range(g.n_slots):                                  # bcastAppend, raft.go:515-522
        if to != c.own:
            _maybe_send_append(n, to, msgs, st)
    commit = g.log.committed
    msgs = [(t, to, i, lt, commit if t == MSG_APP else 0, k) for t, to, i, lt, _, k in msgs]
    return pf | PFLAG_BCAST, msgs
