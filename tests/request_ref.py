"""CPU restatement of etcd's MsgReadIndex and MsgTransferLeader paths — TEST
INFRASTRUCTURE ONLY.

One node's Step(MsgReadIndex) and Step(MsgTransferLeader), statement by
statement as Go has them, on top of tests/propose_ref.py's ``ProposeNode``
(the campaign's node, the log as a list of terms, maybeSendAppend).  Paths are
relative to the reference's ``raft/``:

  Step's term filter                           raft.go:847-921
  stepLeader MsgReadIndex                      raft.go:1078-1097
  stepLeader MsgTransferLeader                 raft.go:1099-1104, 1339-1370
  stepFollower MsgTransferLeader / ReadIndex   raft.go:1445-1451, 1458-1464
  committedEntryInCurrentTerm                  raft.go:1731-1733
  responseToReadIndexReq                       raft.go:1737-1752
  sendMsgReadIndexResponse                     raft.go:1827-1843
  readOnly.addRequest / recvAck                read_only.go:56-76
  bcastHeartbeatWithCtx / sendHeartbeat        raft.go:495-541
  ProgressTracker.IsSingleton                  tracker/tracker.go:228-230

``readOnly`` is what Go has: ``pending`` is the map pendingReadIndex (context
-> status) and ``queue`` the slice readIndexQueue; the engine's queue rows
appear only at the edges (``sync`` lays them out for packing).  The log is the
ProposeNode's list of terms, one per entry, so nothing here shares the
kernel's run arithmetic.

Three things are the engine's, not Go's, and are found before anything is
applied: a context of 0 (its empty context), a requesting slot that names no
Progress (the queue row can only hold a slot), and a queue of ``readq_cap``
rows (a new context against a full queue is handed back).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

from oracle import leader_ref as L
from tests import campaign_ref as CR, propose_ref as PR

U64 = (1 << 64) - 1
FOLLOWER, CANDIDATE, LEADER, PRE_CANDIDATE = 0, 1, 2, 3
NO_SLOT = L.NO_SLOT
SAFE, LEASE = 0, 1
MSG_APP, MSG_SNAP, MSG_TIMEOUT_NOW = 3, 7, 14

RD_READ_STATE, RD_RESP, RD_BCAST, RD_BCAST_DUP, RD_POSTPONED = 1, 2, 3, 4, 5
RD_FORWARD, RD_DROPPED, RD_IGNORED, RD_QUEUE_FULL, RD_HOST, RD_BAD = 6, 7, 8, 9, 10, 11
QFLAG_HEARTBEATS, QFLAG_POSTPONED, QFLAG_TRANSFER_STARTED = 0x01, 0x02, 0x04
QFLAG_TRANSFER_ABORTED, QFLAG_FORWARD, QFLAG_HOST, QFLAG_BAD = 0x08, 0x10, 0x20, 0x40
QSTAT_NAMES = ("read_states", "read_resps", "bcast", "bcast_dup", "postponed", "rd_forward",
               "rd_dropped", "rd_ignored", "queue_full", "rd_host", "bad_ctx", "bad_count",
               "bcast_groups", "xf_started", "xf_timeout_now", "xf_msg_app", "xf_msg_snap",
               "xf_aborted", "xf_ign_term", "xf_ign_no_progress", "xf_ign_learner", "xf_ign_same",
               "xf_ign_self", "xf_ign_role", "xf_forward", "xf_dropped", "xf_host")
_RD_STAT = {RD_READ_STATE: "read_states", RD_RESP: "read_resps", RD_BCAST: "bcast",
            RD_BCAST_DUP: "bcast_dup", RD_POSTPONED: "postponed", RD_FORWARD: "rd_forward",
            RD_DROPPED: "rd_dropped", RD_IGNORED: "rd_ignored", RD_QUEUE_FULL: "queue_full",
            RD_HOST: "rd_host", RD_BAD: "bad_ctx"}


@dataclass
class Config:
    read_only: int = SAFE
    readq_cap: int = 4
    max_reads: int = 1


@dataclass
class RequestNode:
    """A raft node as the two requests see it: the proposal's node (role, lead,
    Progress, masks, transferee, the log's terms) plus readOnly."""
    prop: PR.ProposeNode
    pending: Dict[int, L.ReadIndexStatus] = field(default_factory=dict)  # pendingReadIndex
    queue: List[int] = field(default_factory=list)                       # readIndexQueue

    @property
    def camp(self) -> CR.CampaignNode:
        return self.prop.camp

    @property
    def group(self) -> L.LeaderGroup:
        return self.prop.camp.group

    def sync(self) -> None:
        """The words the engine's arrays hold: the log's, and the queue rows."""
        self.prop.sync()
        self.group.readq = [self.pending[c] for c in self.queue]


def new_node(prop: PR.ProposeNode) -> RequestNode:
    """Takes over the LeaderGroup's queue rows, oldest first."""
    n = RequestNode(prop)
    for rs in prop.group.readq:
        n.pending[rs.ctx] = rs
        n.queue.append(rs.ctx)
    n.sync()
    return n


def new_stats() -> dict:
    return {k: 0 for k in QSTAT_NAMES}


@dataclass
class Result:
    qflags: int = 0
    reads: List[Tuple[int, Optional[int]]] = field(default_factory=list)  # (status, index)
    heartbeats: Optional[List[Tuple[int, int]]] = None   # (to slot, commit) of one broadcast
    xf: Tuple[int, int, int, int] = (0, 0, 0, 0)          # (type, index, log_term, n)


def _is_singleton(g: L.LeaderGroup) -> bool:
    """tracker.go:228-230."""
    return bin(g.mask_in).count("1") == 1 and g.mask_out == 0


def _committed_entry_in_current_term(n: RequestNode) -> bool:
    """raft.go:1731-1733."""
    return n.prop.log_term(n.group.log.committed) == n.group.term


def _response_to_read_index_req(n: RequestNode, frm: int) -> Tuple[int, int]:
    """raft.go:1737-1752 at readIndex = committed."""
    if frm == NO_SLOT or frm == n.camp.own:
        return RD_READ_STATE, n.group.log.committed
    return RD_RESP, n.group.log.committed


def _bcast_heartbeat_with_ctx(n: RequestNode) -> List[Tuple[int, int]]:
    """raft.go:534-541 -> sendHeartbeat raft.go:495-511: every Progress but the
    own, learners included, commit = min(match, committed)."""
    g = n.group
    return [(s, min(g.prs[s].match, g.log.committed)) for s in range(g.n_slots) if s != n.camp.own]


def _step_read(n: RequestNode, ctx: int, frm: int, cfg: Config, res: Result) -> Tuple[int, Optional[int]]:
    c, g = n.camp, n.group
    if c.state == FOLLOWER:                                       # raft.go:1458-1464
        if c.lead == CR.NONE:
            return RD_DROPPED, None
        res.qflags |= QFLAG_FORWARD
        return RD_FORWARD, None
    if c.state != LEADER:                                         # stepCandidate: no case
        return RD_IGNORED, None
    if ctx == 0:
        res.qflags |= QFLAG_BAD
        return RD_BAD, None
    if frm != NO_SLOT and frm >= g.n_slots:
        res.qflags |= QFLAG_HOST
        return RD_HOST, None
    if _is_singleton(g):                                          # raft.go:1080-1085
        return _response_to_read_index_req(n, frm)
    if not _committed_entry_in_current_term(n):                   # raft.go:1089-1092
        g.pending_readindex = True
        res.qflags |= QFLAG_POSTPONED
        return RD_POSTPONED, None
    # sendMsgReadIndexResponse, raft.go:1827-1843
    if cfg.read_only == LEASE:
        return _response_to_read_index_req(n, frm)
    new = ctx not in n.pending
    if new and len(n.queue) >= cfg.readq_cap:                     # the engine's bound
        return RD_QUEUE_FULL, None
    if new:                                                       # addRequest, read_only.go:56-63
        n.pending[ctx] = L.ReadIndexStatus(ctx, g.log.committed, set(), frm)
        n.queue.append(ctx)
    if c.own < 16:                                                # recvAck(r.id), read_only.go:68-76
        n.pending[ctx].acks.add(c.own)
    res.heartbeats = _bcast_heartbeat_with_ctx(n)
    res.qflags |= QFLAG_HEARTBEATS
    return (RD_BCAST if new else RD_BCAST_DUP), None


def _step_transfer(n: RequestNode, frm: int, mterm: int, res: Result, st: dict) -> None:
    c, g = n.camp, n.group
    if mterm != 0 and mterm < g.term:                             # raft.go:878-921
        st["xf_ign_term"] += 1
        return
    if mterm > g.term:                                            # raft.go:851-877: the host's
        st["xf_host"] += 1
        res.qflags |= QFLAG_HOST
        return
    if c.state == FOLLOWER:                                       # raft.go:1445-1451
        if c.lead == CR.NONE:
            st["xf_dropped"] += 1
            return
        st["xf_forward"] += 1
        res.qflags |= QFLAG_FORWARD
        return
    if c.state != LEADER:
        st["xf_ign_role"] += 1
        return
    if frm >= g.n_slots:                                          # raft.go:1100-1104
        st["xf_ign_no_progress"] += 1
        return
    pr = g.prs[frm]
    if not (((g.mask_in | g.mask_out) >> frm) & 1):               # raft.go:1340-1343
        st["xf_ign_learner"] += 1
        return
    lead_transferee = frm
    last_lead_transferee = g.transferee
    if last_lead_transferee != NO_SLOT:                           # raft.go:1346-1354
        if last_lead_transferee == lead_transferee:
            st["xf_ign_same"] += 1
            return
        g.transferee = NO_SLOT
        st["xf_aborted"] += 1
        res.qflags |= QFLAG_TRANSFER_ABORTED
    if lead_transferee == c.own:                                  # raft.go:1355-1358
        st["xf_ign_self"] += 1
        return
    c.election_elapsed = 0                                        # raft.go:1362
    g.transferee = lead_transferee
    st["xf_started"] += 1
    res.qflags |= QFLAG_TRANSFER_STARTED
    if pr.match == n.prop.last:                                   # raft.go:1364-1369
        res.xf = (MSG_TIMEOUT_NOW, 0, 0, 0)
        st["xf_timeout_now"] += 1
        return
    msgs: list = []
    PR._maybe_send_append(n.prop, frm, msgs, {"msg_app": 0, "msg_snap": 0})
    if msgs:
        t, _, idx, lt, _, k = msgs[0]
        res.xf = (t, idx, lt, k)
        st["xf_msg_app" if t == MSG_APP else "xf_msg_snap"] += 1


def step(n: RequestNode, reads, xf_from: int, xf_term: int, cfg: Config, st: dict) -> Result:
    """One group's requests of one call: ``reads`` is [(ctx, from slot)] (more
    than cfg.max_reads are cut there and counted), then the transfer
    (xf_from == NO_SLOT: none)."""
    res = Result()
    if len(reads) > cfg.max_reads:
        reads = reads[:cfg.max_reads]
        st["bad_count"] += 1
        res.qflags |= QFLAG_BAD
    for ctx, frm in reads:
        s = _step_read(n, ctx, frm, cfg, res)
        st[_RD_STAT[s[0]]] += 1
        res.reads.append(s)
    if res.heartbeats is not None:
        st["bcast_groups"] += 1
    if xf_from != NO_SLOT:
        _step_transfer(n, xf_from, xf_term, res, st)
    n.sync()
    return res
