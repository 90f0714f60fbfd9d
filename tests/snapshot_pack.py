"""Packing between tests/snapshot_ref.py's nodes / records and the arrays of
qb_snapshot_groups / qb_snapshot_inbox / qb_snapshot_out, the seeded cases the
GPU tests and the benchmark's parity check share, and the layout of K copies
of a base end to end (tests/replicate.py's per-kind functions) — TEST
INFRASTRUCTURE ONLY."""
from __future__ import annotations

import copy
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests import replicate as X, snapshot_ref as S

MAX_RUNS = 8
U64 = S.U64
FILL = 0xA5A5A5A5A5A5A5A5   # pre-fill of u64 outputs and of unused run rows
FILL32, FILL16, FILL8 = 0xA5A5A5A5, 0xA5A5, 0xA5
_FILLS = {np.uint64: FILL, np.uint32: FILL32, np.uint16: FILL16, np.uint8: FILL8}
PROMOTABLE = 0x80
META_KEEP = 0xA5F0FF00      # the meta word's other fields: bits 16-19 are the run count

STATE = {"self_id": np.uint64, "term": np.uint64, "vote": np.uint64, "lead": np.uint64,
         "committed": np.uint64, "role": np.uint8, "election_elapsed": np.uint32,
         "heartbeat_elapsed": np.uint32, "first_index": np.uint64, "last_index": np.uint64,
         "last_term": np.uint64, "meta": np.uint32, "run_start": np.uint64, "run_term": np.uint64,
         "unstable_offset": np.uint64, "usnap_index": np.uint64, "usnap_term": np.uint64,
         "pending": np.uint8}
ROWS = ("run_start", "run_term")
REC = {"group": np.uint32, "from": np.uint64, "term": np.uint64, "snap_index": np.uint64,
       "snap_term": np.uint64}
OUT = {"sflags": np.uint16, "resp_type": np.uint8, "resp_term": np.uint64, "resp_index": np.uint64}
# per-kind layout, as tests/replicate.py names the kinds
STATE_KINDS = {k: (X.ROWS if k in ROWS else X.GROUP) for k in STATE}
REC_KINDS = {"group": X.REC_GROUP, "from": X.REC, "term": X.REC, "snap_index": X.REC,
             "snap_term": X.REC, "cs_off": X.ENT_OFF, "cs_id": X.ENT, "cs_set": X.ENT}


def runs_of(n: S.Node):
    """The node's log as (start, term) runs: run 0 starts at first_index - 1."""
    runs = []
    for k, t in enumerate(n.terms):
        if not runs or runs[-1][1] != t:
            runs.append(((n.first_index - 1 + k) & U64, t))
    return runs


def pack_nodes(nodes: Sequence[S.Node], base: Optional[Dict[str, np.ndarray]] = None):
    """The state arrays of ``nodes``.  Run rows a node's table does not use,
    and the meta word's other fields, hold what ``base`` holds (the arrays
    before a call: the call must leave them), else the fill."""
    G = len(nodes)
    a = {k: np.zeros(G * (MAX_RUNS if k in ROWS else 1), dt) for k, dt in STATE.items()}
    for k in ROWS:
        a[k][:] = base[k] if base is not None else FILL
    for g, n in enumerate(nodes):
        runs = runs_of(n)
        assert 1 <= len(runs) <= MAX_RUNS, len(runs)
        for q, (s, t) in enumerate(runs):
            a["run_start"][q * G + g] = s
            a["run_term"][q * G + g] = t
        keep = (int(base["meta"][g]) & ~0xF0000) if base is not None else META_KEEP
        a["meta"][g] = keep | (len(runs) << 16)
        a["self_id"][g] = n.id
        a["term"][g], a["vote"][g], a["lead"][g], a["committed"][g] = n.term, n.vote, n.lead, n.committed
        a["role"][g] = n.state | (PROMOTABLE if n.promotable else 0) | n.role_other
        a["election_elapsed"][g], a["heartbeat_elapsed"][g] = n.election_elapsed, n.heartbeat_elapsed
        a["first_index"][g], a["last_index"][g] = n.first_index, n.last_index
        a["last_term"][g] = n.last_term
        a["unstable_offset"][g] = n.offset
        a["usnap_index"][g], a["usnap_term"][g] = n.snap if n.snap is not None else (0, 0)
        a["pending"][g] = n.pending
    return a


def nodes_from_arrays(a: Dict[str, np.ndarray], groups: Optional[Sequence[int]] = None) -> List[S.Node]:
    """The inverse of pack_nodes, for ``groups`` (default: all)."""
    G = len(a["term"])
    out = []
    for g in (range(G) if groups is None else groups):
        nr = (int(a["meta"][g]) >> 16) & 0xF
        last = int(a["last_index"][g])
        starts = [int(a["run_start"][q * G + g]) for q in range(nr)] + [(last + 1) & U64]
        terms: List[int] = []
        for q in range(nr):
            terms += [int(a["run_term"][q * G + g])] * ((starts[q + 1] - starts[q]) & U64)
        role = int(a["role"][g])
        si = int(a["usnap_index"][g])
        out.append(S.Node(
            id=int(a["self_id"][g]), term=int(a["term"][g]), vote=int(a["vote"][g]),
            lead=int(a["lead"][g]), committed=int(a["committed"][g]), state=role & 3,
            promotable=bool(role & PROMOTABLE), role_other=role & ~(3 | PROMOTABLE),
            election_elapsed=int(a["election_elapsed"][g]),
            heartbeat_elapsed=int(a["heartbeat_elapsed"][g]),
            first_index=int(a["first_index"][g]), terms=terms,
            offset=int(a["unstable_offset"][g]),
            snap=(si, int(a["usnap_term"][g])) if si else None, pending=int(a["pending"][g])))
    return out


def flat_cs(cs) -> Tuple[List[int], List[int]]:
    ids, sets = [], []
    for s, name in enumerate(S.CS_LISTS):
        for v in cs.get(name, ()):
            ids.append(int(v))
            sets.append(s)
    return ids, sets


def pack_records(recs: Sequence[Tuple[int, S.Snap]]) -> Dict[str, np.ndarray]:
    R = len(recs)
    a = {k: np.zeros(R, dt) for k, dt in REC.items()}
    off = np.zeros(R + 1, np.uint32)
    ids: List[int] = []
    sets: List[int] = []
    for i, (g, m) in enumerate(recs):
        a["group"][i], a["from"][i], a["term"][i] = g, m.frm, m.term
        a["snap_index"][i], a["snap_term"][i] = m.index, m.sterm
        i_, s_ = flat_cs(m.cs)
        ids += i_
        sets += s_
        off[i + 1] = len(ids)
    a["cs_off"], a["cs_id"], a["cs_set"] = off, np.array(ids, np.uint64), np.array(sets, np.uint8)
    return a


def clamped(recs: Sequence[Tuple[int, S.Snap]], C: int) -> List[Tuple[int, S.Snap]]:
    """The records as a call with a ConfState total of ``C`` reads them:
    offsets above C read as C, so the IDs past it are in no record."""
    out, pos = [], 0
    for g, m in recs:
        ids, sets = flat_cs(m.cs)
        keep = max(0, min(len(ids), C - pos))
        cs = {name: [i for i, s in zip(ids[:keep], sets[:keep]) if s == k]
              for k, name in enumerate(S.CS_LISTS)}
        pos += len(ids)
        out.append((g, S.Snap(m.frm, m.term, m.index, m.sterm, cs)))
    return out


def filled_out(R: int) -> Dict[str, np.ndarray]:
    return {k: np.full(max(R, 1), _FILLS[dt], dt) for k, dt in OUT.items()}


def pack_out(ref: dict, R_buf: int) -> Dict[str, np.ndarray]:
    """The output columns a call leaves in buffers of R_buf >= R elements
    pre-filled by filled_out: every record written, nothing behind them."""
    a = filled_out(R_buf)
    R = len(ref["sflags"])
    for k in OUT:
        a[k][:R] = np.array(ref[k], OUT[k]) if R else []
    return a


# ------------------------------------------------------------ seeded cases ---
INDEX_KINDS = ("at_committed", "below_committed", "inside_match", "inside_mismatch",
               "last_match", "last_mismatch", "boundary_match", "boundary_mismatch",
               "past_nonzero", "past_zero", "huge")
CS_KINDS = ("voter", "learner", "outgoing", "next_only", "absent")
CS_SPANS = (0, 1, 16, 40)
TERM_KINDS = ("zero", "lower", "equal", "higher")


def seeded_node(rng: np.random.Generator, nruns: Optional[int] = None) -> S.Node:
    """A well-formed node in any role: 1 to 8 runs, the commit low enough that
    most of the log lies behind it."""
    first = int(rng.choice([1, 1, 6, 1000, 1 << 40]))
    nruns = int(rng.integers(1, MAX_RUNS + 1)) if nruns is None else nruns
    t = 0 if first == 1 else int(rng.integers(1, 5))
    terms: List[int] = []
    for q in range(nruns):
        terms += [t] * int(rng.integers(1, 4) + (1 if q == 0 else 0))
        t += int(rng.integers(1, 4))
    last = first - 1 + len(terms) - 1
    committed = int(rng.integers(first - 1, min(first + 1, last) + 1))
    snap = None
    offset = int(rng.integers(committed + 1, last + 2))
    if first > 1 and rng.integers(0, 4) == 0:   # an earlier snapshot still unstable
        snap, offset = (first - 1, terms[0]), first
    return S.Node(id=int(rng.integers(1, 8)), term=terms[-1] + int(rng.integers(1, 4)),
                  vote=int(rng.integers(0, 4)), lead=int(rng.integers(0, 4)), committed=committed,
                  state=int(rng.choice([0, 0, 0, 1, 2, 3])), promotable=bool(rng.integers(0, 2)),
                  role_other=int(rng.choice([0, 0x40])), election_elapsed=int(rng.integers(0, 10)),
                  heartbeat_elapsed=int(rng.integers(0, 3)), first_index=first, terms=terms,
                  offset=offset, snap=snap, pending=int(rng.integers(0, 4)))


def conf_state(rng: np.random.Generator, own: int, kind: str, span: int) -> Dict[str, List[int]]:
    """``span`` IDs over the four lists, the node's own ID as ``kind`` says
    (with a span of 0 it is absent whatever the kind)."""
    cs: Dict[str, List[int]] = {name: [] for name in S.CS_LISTS}
    others = [i for i in range(100, 100 + span + 1)]
    where = {"voter": "voters", "learner": "learners", "outgoing": "voters_outgoing",
             "next_only": "learners_next"}.get(kind)
    n_other = span - (1 if where and span else 0)
    for j in range(n_other):
        cs[S.CS_LISTS[int(rng.integers(0, 4))]].append(others[j])
    if where and span:
        at = int(rng.integers(0, len(cs[where]) + 1))
        cs[where].insert(at, own)
    return cs


def seeded_record(rng: np.random.Generator, n: S.Node, index_kind: str, term_kind: str,
                  cs_kind: str, span: int) -> S.Snap:
    first, last = n.first_index, n.last_index
    dummy = first - 1
    runs = runs_of(n)

    def term_of(i):
        return S.log_term(n, i)

    if index_kind == "at_committed":
        si, st = n.committed, term_of(n.committed)
    elif index_kind == "below_committed":
        si, st = max(n.committed - 1, 0), 1
    elif index_kind in ("inside_match", "inside_mismatch"):
        si = int(rng.integers(n.committed + 1, last + 1)) if last > n.committed else last
        st = term_of(si) + (index_kind == "inside_mismatch")
    elif index_kind in ("last_match", "last_mismatch"):
        si, st = last, n.last_term + (index_kind == "last_mismatch")
    elif index_kind in ("boundary_match", "boundary_mismatch"):
        q = int(rng.integers(0, len(runs)))
        si = runs[q][0]
        if si <= n.committed:                      # keep the boundary behind the commit
            n.committed = max(dummy, si - 1)
            n.offset = max(n.offset, n.committed + 1) if n.snap is None else n.offset
        st = runs[q][1] + (index_kind == "boundary_mismatch")
    elif index_kind == "past_nonzero":
        si, st = last + int(rng.integers(1, 50)), int(rng.integers(1, 9))
    elif index_kind == "past_zero":
        si, st = last + int(rng.integers(1, 50)), 0
    elif index_kind == "huge":
        si, st = U64 - int(rng.integers(0, 2)), U64 - int(rng.integers(0, 2))
    else:
        raise ValueError(index_kind)
    mt = {"zero": 0, "lower": max(n.term - 1, 1) if n.term > 1 else 0, "equal": n.term,
          "higher": (n.term + 1, n.term + 7, U64)[int(rng.integers(0, 3))]}[term_kind]
    return S.Snap(frm=int(rng.integers(1, 8)), term=mt, index=si, sterm=st,
                  cs=conf_state(rng, n.id, cs_kind, span))


def seeded_cases(G: int, seed: int) -> Tuple[List[S.Node], List[S.Snap], List[Tuple[str, str, str, int]]]:
    """One node and one MsgSnap per group; the kinds cycle with different
    periods so a few hundred groups meet every combination that matters.
    Table sizes cycle through 1..8 runs.  Returns (nodes, msgs, kinds)."""
    rng = np.random.default_rng(seed)
    nodes, msgs, kinds = [], [], []
    for g in range(G):
        n = seeded_node(rng, nruns=1 + g % MAX_RUNS)
        ik = INDEX_KINDS[g % len(INDEX_KINDS)]
        tk = TERM_KINDS[(g // 3) % 4] if g % 5 else "equal"
        ck = CS_KINDS[(g // 2) % len(CS_KINDS)] if g % 3 else "voter"
        span = CS_SPANS[(g // 7) % len(CS_SPANS)] if g % 4 == 0 else int(rng.integers(1, 8))
        n.state = (g // 11) % 4 if g % 2 else n.state
        msgs.append(seeded_record(rng, n, ik, tk, ck, span))
        nodes.append(n)
        kinds.append((ik, tk, ck, span))
    return nodes, msgs, kinds


def restoring_case(rng: np.random.Generator, voters: int = 5) -> Tuple[S.Node, S.Snap]:
    """A follower behind the compaction point and the snapshot that restores
    it: a ``voters``-voter ConfState that holds the node."""
    n = seeded_node(rng)
    n.state = S.FOLLOWER
    ids = list(range(1, voters + 1))
    n.id = int(rng.integers(1, voters + 1))
    m = S.Snap(frm=int(rng.integers(1, voters + 1)), term=n.term, index=n.last_index + 100,
               sterm=n.last_term + 1, cs={"voters": ids})
    return n, m


# ------------------------------------------------- K copies laid end to end ---
def lay_state(a: Dict[str, np.ndarray], K: int, G0: int) -> Dict[str, np.ndarray]:
    out = {}
    for k, kind in STATE_KINDS.items():
        out[k] = (X.rep_rows([a[k]], [0] * K, G0).reshape(-1) if kind == X.ROWS
                  else X.rep_group([a[k]], [0] * K))
    return out


def lay_records(r: Dict[str, np.ndarray], K: int, G0: int) -> Dict[str, np.ndarray]:
    """Copy c's records behind copy c - 1's (copy-major), their groups + c *
    G0 (a group outside the base stays outside the result) and their spans
    behind the earlier copies'."""
    out = {}
    g = r["group"].astype(np.int64)
    c = np.repeat(np.arange(K, dtype=np.int64), len(g))
    gg = np.tile(g, K)
    out["group"] = np.where(gg < G0, gg + c * G0, np.minimum(gg - G0 + K * G0, 0xFFFFFFFF)).astype(np.uint32)
    for k in ("from", "term", "snap_index", "snap_term", "cs_id", "cs_set"):
        out[k] = np.tile(r[k], K)
    out["cs_off"] = X.rep_off(r["cs_off"], K)
    return out


def lay_out(o: Dict[str, np.ndarray], K: int) -> Dict[str, np.ndarray]:
    return {k: np.tile(v, K) for k, v in o.items()}


class DeviceState:
    """State arrays on the device as the dataclasses ``follower_snapshot``
    takes (built field by field: the mirror's host-side table check is for
    well-formed logs, and these hold wrapped and extreme ones too)."""

    def __init__(self, a: Dict[str, np.ndarray], device="cuda", pending: bool = True,
                 election_timeout: int = 10):
        import importlib

        import torch

        from etcd_amd.quorum import follower as qf, tick as qt
        qy = importlib.import_module("etcd_amd.quorum.ready")
        from etcd_amd.quorum._dev import to_dev
        self.G = G = len(a["term"])
        d = {k: to_dev(a[k], dt, device) for k, dt in STATE.items()}
        self.d = d
        tstate = qt.TickState(d["role"], d["election_elapsed"], d["heartbeat_elapsed"],
                              torch.zeros(max(G, 1), dtype=torch.int32, device=device))
        self.groups = qf.FollowerGroups(G, election_timeout, True, True,
                                        {k: d[k] for k in qf._U64_FIELDS}, tstate)
        self.log = qf.FollowerLog(G, d["meta"], d["first_index"], d["run_start"], d["run_term"])
        self.ready = qy.ReadyState(G, {"unstable_offset": d["unstable_offset"],
                                       "usnap_index": d["usnap_index"],
                                       "usnap_term": d["usnap_term"],
                                       "pending": d["pending"] if pending else None})
        self.self_id = d["self_id"]

    def numpy(self) -> Dict[str, np.ndarray]:
        n = {k: self.G * (MAX_RUNS if k in ROWS else 1) for k in STATE}
        return {k: self.d[k].cpu().numpy().view(dt)[:n[k]] for k, dt in STATE.items()}


def device_inbox(r: Dict[str, np.ndarray], device="cuda", C: Optional[int] = None):
    """A SnapshotInbox over packed record arrays (``C``: a ConfState total
    below the arrays' — offsets above it read as C)."""
    from etcd_amd.quorum import snapshot as qs
    from etcd_amd.quorum._dev import to_dev
    dts = dict(REC, cs_off=np.uint32, cs_id=np.uint64, cs_set=np.uint8)
    t = {k: to_dev(r[k], dts[k], device) for k in dts}
    return qs.SnapshotInbox(len(r["group"]), len(r["cs_id"]) if C is None else C, t,
                            groups_host=r["group"])


def run_reference(nodes: List[S.Node], recs, pending: bool = True, stats=None):
    """snapshot_call on a deep copy: (nodes after, the call's outputs)."""
    after = copy.deepcopy(nodes)
    return after, S.snapshot_call(after, recs, st=stats, pending=pending)
