"""CPU restatement of raft.switchToConfig and of the slot renumbering that
qb_dev_switch_config puts in front of it — TEST INFRASTRUCTURE ONLY.

One group at a time, statement by statement as Go has them, on the packed
arrays the engine takes (tests/switch_pack.py).  A group is unpacked into a
node keyed by raft ID, as Go holds it (Progress map, Votes map, the pending
reads' From IDs, the transferee's ID), switchToConfig runs on that, and the
node is packed again under the new slots; the engine's renumbering therefore
falls out of the IDs here and shares no arithmetic with the kernel's slot map.
Paths are relative to the reference's ``raft/``:

  switchToConfig                               raft.go:1651-1700
  restore's tail                               raft.go:1606-1609
  maybeCommit                                  raft.go:585-588, log.go:328-334
  maybeSendAppend(to, sendIfEmpty)             raft.go:432-492
  bcastAppend                                  raft.go:515-522
  raftLog.term / entries                       log.go:268-299
  Progress.MaybeUpdate / IsPaused / BecomeSnapshot   tracker/progress.go
  Inflights.Add                                tracker/inflights.go:55-70
  JointConfig / MajorityConfig.CommittedIndex  quorum/joint.go:49-57, majority.go:126-172

The two stops (a pending read from an ID the new config lacks; a removed or
demoted leader whose transferee's ID the new config lacks) are found before
anything is applied, as the engine reports them.
"""
from __future__ import annotations

import numpy as np

U64 = (1 << 64) - 1
MAX_SLOTS, MAX_RUNS = 16, 8
NONE_SLOT = 0xFF
LEADER = 2
SW_NONE, SW_SWITCH, SW_RESTORE = 0, 1, 2
MSG_APP, MSG_SNAP = 3, 7
PROBE, REPLICATE, SNAPSHOT = 0, 1, 2
PROBE_SENT, RECENT_ACTIVE = 0x04, 0x08
SWFLAG_SWITCHED, SWFLAG_COMMITTED, SWFLAG_SENT, SWFLAG_TRANSFER_ABORTED = 0x01, 0x02, 0x04, 0x08
SWFLAG_SELF_REMOVED, SWFLAG_SELF_LEARNER, SWFLAG_VOTE_DROPPED, SWFLAG_HOST = 0x10, 0x20, 0x40, 0x80
SWSTAT_NAMES = ("switched", "restores", "commits", "bcast", "probed", "msg_app", "msg_snap",
                "transfer_aborted", "self_removed", "self_learner", "vote_dropped", "host",
                "bad_action")
FILL, FILL8 = 0xA5A5A5A5A5A5A5A5, 0xA5


def new_stats() -> dict:
    return {k: 0 for k in SWSTAT_NAMES}


def _slots(off, g):
    lo, hi = int(off[g]), int(off[g + 1])
    return lo, min(max(hi - lo, 0), MAX_SLOTS)


class _Log:
    """raftLog as the arrays describe it."""

    def __init__(self, a, g, G):
        self.first, self.last = int(a["first_index"][g]), int(a["last_index"][g])
        nr = (int(a["meta"][g]) >> 16) & 0xF
        nr = min(max(nr, 1), MAX_RUNS)
        self.runs = [(int(a["run_start"][r * G + g]), int(a["run_term"][r * G + g]))
                     for r in range(nr)]
        self.max_ents = int(a["max_ents"][g])
        self.snap_index, self.snap_term = int(a["snap_index"][g]), int(a["snap_term"][g])

    def term(self, i):  # log.go:268-288 (+ zeroTermOnErrCompacted)
        if i < ((self.first - 1) & U64) or i > self.last:
            return 0
        t = 0
        for start, rt in self.runs:
            if start <= i:
                t = rt
        return t

    def entries(self, lo):  # log.go:290-299: (count, ErrCompacted)
        if lo > self.last:
            return 0, False
        if lo < self.first:
            return 0, True
        return min(self.max_ents, self.last - lo + 1), False


def _is_paused(a, i, K):  # progress.go:193-212
    st = int(a["pstate"][i])
    if st & 3 == PROBE:
        return bool(st & PROBE_SENT)
    if st & 3 == REPLICATE:
        return (int(a["infl_pos"][i]) >> 16) == K
    return True


def _maybe_send_append(a, log, i, send_if_empty, K, to, msgs, st):
    """raft.go:432-492 on the Progress at slot index i."""
    if _is_paused(a, i, K):
        return False
    nxt = int(a["next"][i])
    term = log.term((nxt - 1) & U64)
    cnt, compacted = log.entries(nxt)
    if cnt == 0 and not send_if_empty:
        return False
    ps = int(a["pstate"][i])
    if compacted:
        if not ps & RECENT_ACTIVE:
            return False
        if log.snap_index == 0:               # ErrSnapshotTemporarilyUnavailable
            return False
        msgs.append((MSG_SNAP, to, log.snap_index, log.snap_term, cnt))
        a["pstate"][i] = (ps & RECENT_ACTIVE) | SNAPSHOT      # BecomeSnapshot
        a["pending_snapshot"][i] = log.snap_index
        a["infl_pos"][i] = 0
        st["msg_snap"] += 1
        return True
    msgs.append((MSG_APP, to, (nxt - 1) & U64, term, cnt))
    if cnt != 0:
        if ps & 3 == REPLICATE:
            last = (nxt + cnt - 1) & U64
            a["next"][i] = (last + 1) & U64                   # OptimisticUpdate
            pos = int(a["infl_pos"][i])                       # Inflights.Add
            start, count = pos & 0xFFFF, pos >> 16
            nx = start + count
            if nx >= K:
                nx -= K
            a["infl_buf"][i * K + nx] = last
            a["infl_pos"][i] = start | ((count + 1) << 16)
        elif ps & 3 == PROBE:
            a["pstate"][i] = ps | PROBE_SENT
        else:
            raise AssertionError("sending append in unhandled state")
    st["msg_app"] += 1
    return True


def _committed_index(a, s0, ns, mask_in, mask_out):
    def half(mask):
        ms = sorted(int(a["match"][s0 + k]) for k in range(ns) if (mask >> k) & 1)
        if not ms:
            return U64
        return ms[len(ms) - (len(ms) // 2 + 1)]
    return min(half(mask_in), half(mask_out))


def _maybe_update_to_next(a, i):
    """pr.MaybeUpdate(pr.Next - 1), progress.go:144-153."""
    n = (int(a["next"][i]) - 1) & U64
    if int(a["match"][i]) < n:
        a["match"][i] = n
        a["pstate"][i] = int(a["pstate"][i]) & ~PROBE_SENT & 0xFF
    a["next"][i] = max(int(a["next"][i]), (n + 1) & U64)


def switch_group(a, g, action, K, Q, out, st):
    """One action byte on group g of the arrays ``a`` (in place).  ``out``:
    swflags / slot_map / msg_* (numpy, in place), written as the engine writes
    them.  Returns (swflags, msgs): msgs are (type, to slot, index, log_term,
    commit, n) in the order Visit emits them."""
    G = len(a["cfg"])
    if action > SW_RESTORE:
        st["bad_action"] += 1
        out["swflags"][g] = 0
        return 0, []
    if action == SW_NONE:
        out["swflags"][g] = 0
        return 0, []
    o0, no = _slots(a["old_off"], g)
    s0, ns = _slots(a["off"], g)
    old_ids = [int(x) for x in a["old_ids"][o0:o0 + no]]
    ids = [int(x) for x in a["ids"][s0:s0 + ns]]
    new_slot = {i: k for k, i in enumerate(ids)}
    cfg, meta = int(a["cfg"][g]), int(a["meta"][g])
    mask_in, mask_out = cfg & 0xFFFF, cfg >> 16
    voters = {i for k, i in enumerate(ids) if ((mask_in | mask_out) >> k) & 1}
    self_id = int(a["self_id"][g])
    leader = int(a["role"][g]) & 3 == LEADER

    # the node by ID, as Go holds it
    def id_of(slot):           # an old slot's ID; None: the slot names no member
        return old_ids[slot] if slot < no else None
    xf_slot = (meta >> 8) & 0xFF
    transferee = None if xf_slot == NONE_SLOT else (id_of(xf_slot), )   # (id,) / (None,)
    nrq = min((meta >> 20) & 0x1F, Q)
    reads = []
    for k in range(nrq):
        q = int(a["rq_meta"][g * Q + k])
        frm = (q >> 16) & 0xFF
        reads.append((q & 0xFF000000, [id_of(b) for b in range(16) if (q >> b) & 1],
                      None if frm == NONE_SLOT else (id_of(frm), )))
    ok = self_id in new_slot
    is_learner = ok and self_id not in voters

    # the stops
    stop = any(r[2] is not None and r[2][0] not in new_slot for r in reads)
    if leader and (not ok or is_learner) and transferee is not None and \
            transferee[0] not in new_slot:
        stop = True
    if stop:
        st["host"] += 1
        out["swflags"][g] = SWFLAG_HOST
        return SWFLAG_HOST, []

    sf = SWFLAG_SWITCHED
    st["switched"] += 1
    st["restores"] += action == SW_RESTORE
    # the renumbering: every slot-encoded word packed again under the new slots
    if out.get("slot_map") is not None:
        for k, i in enumerate(old_ids):
            out["slot_map"][o0 + k] = new_slot.get(i, NONE_SLOT)
    for k, (hi, acks, frm) in enumerate(reads):
        q = hi | sum(1 << new_slot[i] for i in acks if i in new_slot)
        q |= (NONE_SLOT if frm is None else new_slot[frm[0]]) << 16
        a["rq_meta"][g * Q + k] = q
    if a.get("votes") is not None:
        w = int(a["votes"][g])
        voted = [id_of(b) for b in range(16) if (w >> b) & 1]
        granted = [id_of(b) for b in range(16) if (w >> (16 + b)) & 1]
        if any(i not in new_slot for i in voted):
            sf |= SWFLAG_VOTE_DROPPED
            st["vote_dropped"] += 1
        a["votes"][g] = sum(1 << new_slot[i] for i in voted if i in new_slot) | \
            sum(1 << new_slot[i] for i in granted if i in new_slot) << 16
    own = new_slot.get(self_id, NONE_SLOT)
    xf = NONE_SLOT if transferee is None else new_slot.get(transferee[0], NONE_SLOT)

    msgs = []
    log = _Log(a, g, G)

    def switch_to_config():                                    # raft.go:1651-1700
        nonlocal sf, xf
        if (not ok or is_learner) and leader:                  # raft.go:1663-1674
            if not ok:
                sf |= SWFLAG_SELF_REMOVED
                st["self_removed"] += 1
            else:
                sf |= SWFLAG_SELF_LEARNER
                st["self_learner"] += 1
            return
        if not leader or mask_in == 0:                         # raft.go:1678
            return
        sf |= SWFLAG_SENT
        mci = _committed_index(a, s0, ns, mask_in, mask_out)   # maybeCommit, raft.go:585-588
        if mci > int(a["committed"][g]) and log.term(mci) == int(a["term"][g]):
            a["committed"][g] = mci
            sf |= SWFLAG_COMMITTED
            st["commits"] += 1
            st["bcast"] += 1
            for k in range(ns):                                # bcastAppend
                if ids[k] != self_id:
                    _maybe_send_append(a, log, s0 + k, True, K, k, msgs, st)
        else:
            st["probed"] += 1
            for k in range(ns):                                # raft.go:1690-1692
                _maybe_send_append(a, log, s0 + k, False, K, k, msgs, st)
        if transferee is not None and transferee[0] not in voters:   # raft.go:1695-1697
            xf = NONE_SLOT
            sf |= SWFLAG_TRANSFER_ABORTED
            st["transfer_aborted"] += 1

    switch_to_config()
    if action == SW_RESTORE and ok:                            # raft.go:1608-1609
        _maybe_update_to_next(a, s0 + own)
    a["meta"][g] = (meta & ~0xFFFF & 0xFFFFFFFF) | own | (xf << 8)
    out["swflags"][g] = sf
    commit = int(a["committed"][g])
    if sf & SWFLAG_SENT:
        out["msg_type"][s0:s0 + ns] = 0
        for t, to, idx, lt, n in msgs:
            out["msg_type"][s0 + to] = t
            out["msg_index"][s0 + to] = idx
            out["msg_log_term"][s0 + to] = lt
            out["msg_n"][s0 + to] = n
    return sf, [(t, to, idx, lt, commit if t == MSG_APP else 0, n) for t, to, idx, lt, n in msgs]


def new_out(G, S_old, S):
    return {"swflags": np.full(max(G, 1), FILL8, np.uint8),
            "slot_map": np.full(max(S_old, 1), FILL8, np.uint8),
            "msg_type": np.full(max(S, 1), FILL8, np.uint8),
            "msg_index": np.full(max(S, 1), FILL, np.uint64),
            "msg_log_term": np.full(max(S, 1), FILL, np.uint64),
            "msg_n": np.full(max(S, 1), FILL, np.uint64)}


def switch_config(a, action, K, Q, out, st):
    """One call over every group of ``a`` (in place).  Returns the messages
    per group."""
    return [switch_group(a, g, int(action[g]), K, Q, out, st)[1] for g in range(len(a["cfg"]))]
