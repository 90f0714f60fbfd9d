"""Packing between tests/ready_ref.py's nodes and the arrays of
qb_ready_groups / qb_ready_out / qb_advance_in, and the seeded nodes the GPU
tests and the benchmark's parity check share — TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

from tests import ready_ref as R

MAX_RUNS = 8
U64 = R.U64
FILL = 0xA5A5A5A5A5A5A5A5   # pre-fill of u64 outputs and of unused run rows
FILL32, FILL16, FILL8 = 0xA5A5A5A5, 0xA5A5, 0xA5
PROMOTABLE = 0x80

DTYPES = {"term": np.uint64, "vote": np.uint64, "committed": np.uint64, "lead": np.uint64,
          "role": np.uint8, "first_index": np.uint64, "last_index": np.uint64,
          "last_term": np.uint64, "meta": np.uint32, "run_start": np.uint64,
          "run_term": np.uint64, "pending_conf_index": np.uint64, "ext": np.uint32,
          "applied": np.uint64, "unstable_offset": np.uint64, "usnap_index": np.uint64,
          "usnap_term": np.uint64, "prev_term": np.uint64, "prev_vote": np.uint64,
          "prev_commit": np.uint64, "prev_lead": np.uint64, "prev_role": np.uint8,
          "pending": np.uint8, "uncommitted_size": np.uint64}
# what qb_dev_ready / qb_dev_advance / qb_dev_unstable_truncate may write
STATE = ("applied", "unstable_offset", "usnap_index", "usnap_term", "prev_term", "prev_vote",
         "prev_commit", "prev_lead", "prev_role", "pending", "uncommitted_size")
LIST = {"ready_gid": np.uint32, "rd_flags": np.uint16, "hs_term": np.uint64, "hs_vote": np.uint64,
        "hs_commit": np.uint64, "ent_lo": np.uint64, "ent_hi": np.uint64,
        "ent_last_term": np.uint64, "apply_lo": np.uint64, "apply_hi": np.uint64,
        "snap_index": np.uint64, "lead": np.uint64, "role": np.uint8}
ADV = {"adv_gid": np.uint32, "hs_term": np.uint64, "hs_vote": np.uint64, "hs_commit": np.uint64,
       "applied_to": np.uint64, "applied_payload": np.uint64, "stable_index": np.uint64,
       "stable_term": np.uint64, "stable_snap": np.uint64}
_FILLS = {np.uint64: FILL, np.uint32: FILL32, np.uint16: FILL16, np.uint8: FILL8}


def runs_of(n: R.Node):
    """The node's log as (start, term) runs: run 0 starts at first_index - 1."""
    runs = []
    for k, t in enumerate(n.terms):
        if not runs or runs[-1][1] != t:
            runs.append((n.first_index - 1 + k, t))
    return runs


def pack_nodes(nodes: Sequence[R.Node]) -> Dict[str, np.ndarray]:
    G = len(nodes)
    a = {k: np.zeros(G * (MAX_RUNS if k.startswith("run_") else 1), dt) for k, dt in DTYPES.items()}
    a["run_start"][:] = FILL
    a["run_term"][:] = FILL
    for g, n in enumerate(nodes):
        runs = runs_of(n)
        assert 1 <= len(runs) <= MAX_RUNS, len(runs)
        for q, (s, t) in enumerate(runs):
            a["run_start"][q * G + g] = s
            a["run_term"][q * G + g] = t
        a["meta"][g] = 0xFF00 | (len(runs) << 16)
        a["term"][g], a["vote"][g], a["committed"][g] = n.term, n.vote, n.committed
        a["lead"][g] = n.lead
        a["role"][g] = n.state | (PROMOTABLE if n.promotable else 0)
        a["first_index"][g], a["last_index"][g] = n.first_index, n.last_index
        a["last_term"][g] = n.last_term
        a["pending_conf_index"][g] = n.pending_conf_index
        a["ext"][g] = (1 << 16) if n.auto_leave else 0
        a["applied"][g], a["unstable_offset"][g] = n.applied, n.offset
        a["usnap_index"][g], a["usnap_term"][g] = n.snap if n.snap is not None else (0, 0)
        a["prev_term"][g], a["prev_vote"][g], a["prev_commit"][g] = n.prev_hard
        a["prev_lead"][g], a["prev_role"][g] = n.prev_soft
        a["pending"][g] = (1 if n.msgs else 0) | (2 if n.read_states else 0)
        a["uncommitted_size"][g] = n.uncommitted_size
    return a


def nodes_from_arrays(a: Dict[str, np.ndarray]) -> List[R.Node]:
    """The inverse of pack_nodes (a snapshot index of 0 is no snapshot)."""
    G = len(a["term"])
    out = []
    for g in range(G):
        nr = (int(a["meta"][g]) >> 16) & 0xF
        last = int(a["last_index"][g])
        starts = [int(a["run_start"][q * G + g]) for q in range(nr)] + [last + 1]
        terms: List[int] = []
        for q in range(nr):
            terms += [int(a["run_term"][q * G + g])] * (starts[q + 1] - starts[q])
        role = int(a["role"][g])
        si = int(a["usnap_index"][g])
        out.append(R.Node(
            term=int(a["term"][g]), vote=int(a["vote"][g]), committed=int(a["committed"][g]),
            lead=int(a["lead"][g]), state=role & 0x7F, promotable=bool(role & PROMOTABLE),
            first_index=int(a["first_index"][g]), terms=terms, applied=int(a["applied"][g]),
            offset=int(a["unstable_offset"][g]),
            snap=(si, int(a["usnap_term"][g])) if si else None,
            msgs=bool(a["pending"][g] & 1), read_states=bool(a["pending"][g] & 2),
            uncommitted_size=int(a["uncommitted_size"][g]),
            pending_conf_index=int(a["pending_conf_index"][g]),
            auto_leave=bool((int(a["ext"][g]) >> 16) & 1) if "ext" in a else False,
            prev_soft=(int(a["prev_lead"][g]), int(a["prev_role"][g])),
            prev_hard=(int(a["prev_term"][g]), int(a["prev_vote"][g]), int(a["prev_commit"][g]))))
    return out


def filled_list(cap: int) -> Dict[str, np.ndarray]:
    return {k: np.full(max(cap, 1), _FILLS[dt], dt) for k, dt in LIST.items()}


def pack_records(records: Sequence[R.ReadyRecord], cap: int) -> Dict[str, np.ndarray]:
    """The list columns a call leaves in buffers pre-filled by filled_list."""
    a = filled_list(cap)
    for p, r in enumerate(records):
        a["ready_gid"][p], a["rd_flags"][p] = r.gid, r.flags
        a["hs_term"][p], a["hs_vote"][p], a["hs_commit"][p] = r.hs
        a["ent_lo"][p], a["ent_hi"][p], a["ent_last_term"][p] = r.ent
        a["apply_lo"][p], a["apply_hi"][p] = r.apply
        a["snap_index"][p], a["lead"][p], a["role"][p] = r.snap_index, r.lead, r.role
    return a


def pack_advance(recs: Sequence[R.AdvanceRecord]) -> Dict[str, np.ndarray]:
    a = {k: np.zeros(len(recs), dt) for k, dt in ADV.items()}
    for i, r in enumerate(recs):
        a["adv_gid"][i] = r.gid
        a["hs_term"][i], a["hs_vote"][i], a["hs_commit"][i] = r.hs
        a["applied_to"][i], a["applied_payload"][i] = r.applied_to, r.applied_payload
        a["stable_index"][i], a["stable_term"][i] = r.stable_index, r.stable_term
        a["stable_snap"][i] = r.stable_snap
    return a


# ------------------------------------------------------------ seeded nodes ---
def idle_node(rng: np.random.Generator) -> R.Node:
    """A node with nothing to do: every entry stable and applied, the prevs
    current, nothing pending."""
    first = int(rng.choice([1, 1, 6, 1000]))
    nruns = int(rng.integers(1, MAX_RUNS + 1))
    t = 0 if first == 1 else int(rng.integers(1, 5))
    terms: List[int] = []
    for q in range(nruns):
        terms += [t] * int(rng.integers(1, 5) + (1 if q == 0 else 0))
        t += int(rng.integers(1, 4))
    last = first - 1 + len(terms) - 1
    committed = int(rng.integers(first - 1, last + 1))
    n = R.Node(term=terms[-1] + int(rng.integers(0, 3)), vote=int(rng.integers(0, 4)),
               committed=committed, lead=int(rng.integers(0, 4)), state=int(rng.integers(0, 4)),
               promotable=bool(rng.integers(0, 2)), first_index=first, terms=terms,
               applied=committed, offset=last + 1,
               uncommitted_size=int(rng.choice([0, 0, 7, 1000])),
               pending_conf_index=int(rng.integers(0, last + 2)),
               auto_leave=bool(rng.integers(0, 4) == 0)).new_raw_node()
    k = int(rng.integers(0, 8))
    if k == 0:
        n.promotable = not n.promotable  # not part of the SoftState
    elif k == 1 and first == 1:
        # an empty HardState that differs from the prev: MustSync alone, not ready
        n.term = n.vote = n.committed = n.applied = 0
        n.terms, n.offset = [0], 1
        n.pending_conf_index = 0
        n.prev_hard = (0, 3, 0)
    return n


MUTATIONS = ("soft_lead", "soft_role", "hard_term", "hard_vote", "hard_commit", "entries",
             "snapshot", "committed", "msgs", "read_states", "bad_commit", "bad_offset",
             "wrap_applied", "wrap_committed")


def mutate(n: R.Node, rng: np.random.Generator, what: str) -> None:
    first, last = n.first_index, n.last_index
    if what == "soft_lead":
        n.lead += 1
    elif what == "soft_role":
        n.state = (n.state + 1 + int(rng.integers(0, 3))) % 4
    elif what == "hard_term":
        n.term += 1 + int(rng.integers(0, 2))
    elif what == "hard_vote":
        n.vote += 1
    elif what == "hard_commit":
        n.prev_hard = (n.prev_hard[0], n.prev_hard[1], (n.committed + 1) & U64)
    elif what == "entries":
        n.offset = int(rng.integers(first, last + 1))
    elif what == "snapshot":
        n.snap = (int(rng.integers(1, 50)), int(rng.integers(1, 9)))
    elif what == "committed":
        if not first <= n.committed <= last:
            n.committed = int(rng.integers(first, last + 1))
        n.applied = int(rng.integers(max(first - 4, 0), n.committed))
    elif what == "msgs":
        n.msgs = True
    elif what == "read_states":
        n.read_states = True
    elif what == "bad_commit":
        n.committed = last + 1 + int(rng.integers(0, 3))
        n.applied = min(n.applied, last)
    elif what == "bad_offset":
        n.offset = last + 2 + int(rng.integers(0, 3))
    elif what == "wrap_applied":
        n.applied = U64  # applied + 1 wraps to 0: everything from first_index on
        n.committed = max(n.committed, first)
    elif what == "wrap_committed":
        n.committed = U64  # committed + 1 wraps to 0: nothing to apply
    else:
        raise ValueError(what)


def ready_node(rng: np.random.Generator, g: Optional[int] = None) -> R.Node:
    """A node with work: one to three mutations of an idle one (entries need a
    log of at least one entry).  With ``g`` the first mutation cycles through
    MUTATIONS, so a few groups reach every flag."""
    while True:
        n = idle_node(rng)
        if n.last_index >= n.first_index and n.terms != [0]:
            break
    k = int(rng.integers(1, 4))
    picks = [str(w) for w in rng.choice(MUTATIONS[:10], size=k, replace=False)]
    if g is not None:
        picks[0] = MUTATIONS[g % len(MUTATIONS)]
    for w in picks:
        mutate(n, rng, w)
    return n


def seeded_nodes(G: int, frac: str, seed: int) -> List[R.Node]:
    """frac: "none" (no group ready), "some" (about 1 %) or "all"."""
    rng = np.random.default_rng(seed)
    nodes = []
    for g in range(G):
        if frac == "all" or (frac == "some" and (rng.random() < 0.01 or g == G // 2)):
            nodes.append(ready_node(rng, g if frac == "all" else None))
        else:
            nodes.append(idle_node(rng))
    return nodes


def advance_records(nodes: Sequence[R.Node], records: Sequence[R.ReadyRecord],
                    rng: np.random.Generator) -> List[R.AdvanceRecord]:
    """One AdvanceRecord per Ready record: the Ready handled in full, or with
    one of the departures a host can make (a paginated apply, a payload above
    or below uncommitted_size, a stable index whose term no longer matches, a
    cursor outside [applied, committed], a group that does not exist)."""
    out = []
    G = len(nodes)
    for i, r in enumerate(records):
        rec = R.record_of(r, payload=int(rng.choice([0, 3, 7, 5000])))
        n = nodes[r.gid]
        k = i % 12
        if k == 1 and r.flags & R.RDF_COMMITTED and r.apply[1] > r.apply[0]:
            rec.applied_to = int(rng.integers(r.apply[0], r.apply[1]))  # paginated
        elif k == 2 and r.flags & R.RDF_ENTRIES:
            rec.stable_term += 1                                        # truncated since
        elif k == 3 and r.flags & R.RDF_ENTRIES:
            rec.stable_index += 1                                       # past the log
        elif k == 4:
            rec.applied_to = (n.committed + 1) & U64 or 1               # appliedTo's panic
        elif k == 5 and n.applied > 1:
            rec.applied_to = n.applied - 1                              # appliedTo's panic
        elif k == 6:
            rec.gid = G + int(rng.integers(0, 3))                       # no such group
        elif k == 7 and r.flags & R.RDF_ENTRIES and r.ent[1] > r.ent[0]:
            si = int(rng.integers(r.ent[0], r.ent[1]))                  # a prefix persisted:
            rec.stable_index = si                                       # its term from the runs
            rec.stable_term = n.terms[si - (n.first_index - 1)]
        elif k == 8 and r.flags & R.RDF_SNAPSHOT:
            rec.stable_snap += 1                                        # another snapshot
        elif k == 9 and r.flags & R.RDF_ENTRIES and n.offset > n.first_index:
            rec.stable_index = n.offset - 1                             # below the offset
            rec.stable_term = n.terms[rec.stable_index - (n.first_index - 1)]
        out.append(rec)
    return out


def auto_leave_nodes(rng: np.random.Generator, count: int) -> List[R.Node]:
    """Leaders in a joint config with AutoLeave whose pending conf change lies
    in what is about to be applied (raft.go:554), and near misses."""
    out = []
    for i in range(count):
        n = ready_node(rng)
        n.committed = n.last_index
        n.applied = max(n.first_index - 1, n.last_index - 2)
        n.auto_leave = i % 4 != 3
        n.state = R.LEADER if i % 4 != 2 else R.FOLLOWER
        n.pending_conf_index = max(0, n.last_index - (0 if i % 4 != 1 else 5))
        n.offset = min(n.offset, n.last_index + 1)
        out.append(n)
    return out
