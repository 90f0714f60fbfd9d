"""tests/compact_ref.py's nodes and requests <-> the device columns of
qb_dev_log_compact (struct qb_compact_groups / qb_compact_in / qb_compact_out),
and the seeded batches the GPU tests, the smoke run and the stride test share.
Test infrastructure."""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np

from tests import compact_ref as R

MAX_RUNS = R.MAX_RUNS
FILL = 0x5A5A5A5A5A5A5A5A          # rows of a table no run has reached
STATE = {"first_index": np.uint64, "snap_index": np.uint64, "snap_term": np.uint64,
         "meta": np.uint32, "run_start": np.uint64, "run_term": np.uint64,
         "last_index": np.uint64, "applied": np.uint64, "unstable_offset": np.uint64,
         "usnap_index": np.uint64}
LIST = {"gid": np.uint32, "flags": np.uint16, "snap_index": np.uint64, "snap_term": np.uint64,
        "compact_index": np.uint64, "first_before": np.uint64}


def pack_nodes(nodes: List[R.Node], base: Optional[Dict[str, np.ndarray]] = None,
               meta_rest: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
    """The state columns (run tables [MAX_RUNS, G]).  Rows at or above a
    group's run count, and the meta bits outside 16-19, keep what ``base``
    holds (FILL / ``meta_rest`` without one): the call leaves them alone."""
    G = len(nodes)
    a = {k: np.zeros(G, dt) for k, dt in STATE.items() if not k.startswith("run_")}
    if base is not None:
        rs, rt = base["run_start"].reshape(MAX_RUNS, G).copy(), base["run_term"].reshape(MAX_RUNS, G).copy()
        rest = base["meta"] & np.uint32(~0xF0000 & 0xFFFFFFFF)
    else:
        rs, rt = np.full((MAX_RUNS, G), FILL, np.uint64), np.full((MAX_RUNS, G), FILL, np.uint64)
        rest = np.zeros(G, np.uint32) if meta_rest is None else (
            np.asarray(meta_rest, np.uint32) & np.uint32(~0xF0000 & 0xFFFFFFFF))
    for g, n in enumerate(nodes):
        rr = R.runs(n.ents)
        assert 1 <= len(rr) <= MAX_RUNS, (g, len(rr))
        for q, (start, term) in enumerate(rr):
            rs[q, g], rt[q, g] = start, term
        a["meta"][g] = int(rest[g]) | (len(rr) << 16)
        a["first_index"][g] = n.first_index
        a["last_index"][g] = n.last_index
        a["snap_index"][g], a["snap_term"][g] = n.snap_index, n.snap_term
        a["applied"][g] = n.applied
        a["unstable_offset"][g] = n.unstable_offset & R.M64
        a["usnap_index"][g] = n.usnap_index
    a["run_start"], a["run_term"] = rs, rt
    return a


def unpack_nodes(a: Dict[str, np.ndarray]) -> List[R.Node]:
    """The nodes of well-formed columns: each run expanded to its entries."""
    G = len(a["first_index"])
    rs, rt = a["run_start"].reshape(MAX_RUNS, G), a["run_term"].reshape(MAX_RUNS, G)
    out = []
    for g in range(G):
        n = (int(a["meta"][g]) >> 16) & 0xF
        last = int(a["last_index"][g])
        ents = []
        for q in range(n):
            end = int(rs[q + 1, g]) if q + 1 < n else last + 1
            ents += [(i, int(rt[q, g])) for i in range(int(rs[q, g]), end)]
        out.append(R.Node(ents, int(a["unstable_offset"][g]), int(a["applied"][g]),
                          int(a["snap_index"][g]), int(a["snap_term"][g]), int(a["usnap_index"][g]),
                          first_zero=int(a["first_index"][g]) == 0))
    return out


def pack_request(req: R.Request, G: int) -> Dict[str, Optional[np.ndarray]]:
    col = lambda c, dt: None if c is None else np.asarray(c, dt)  # noqa: E731
    return {"snap_at": col(req.snap_at, np.uint64), "compact_at": col(req.compact_at, np.uint64),
            "force": col(req.force, np.uint8), "hold": col(req.hold, np.uint8)}


def pack_result(res: R.Result, list_cap: int, fill: int = 0x5A) -> Dict[str, np.ndarray]:
    """cmflags [G], list_count, and the list columns [list_cap]: records below
    the listed count, the pre-fill behind them."""
    out = {"cmflags": np.asarray(res.flags, np.uint16), "list_count": np.uint64(res.count)}
    for k, dt in LIST.items():
        col = np.full(max(list_cap, 1), fill, dt)     # torch's fill_(0x5A): the value, per element
        for p, rec in enumerate(res.records):
            col[p] = rec[k]
        out[k] = col
    return out


# ------------------------------------------------------------ seeded batches ---

def seeded_node(rng: np.random.Generator, nruns: int) -> R.Node:
    """A log of ``nruns`` runs of 1..6 entries each behind a random offset
    (some past 2^32), with the cursors in Go's order: off <= snap_index's
    floor, applied <= stable_last <= last_index."""
    off = int(rng.choice([0, 1, 7, 1000, (1 << 32) - 3, (1 << 40) + 5]))
    term = int(rng.integers(0 if off == 0 else 1, 5))
    ents, i = [], off
    for _ in range(nruns):
        for _ in range(int(rng.integers(1, 7))):
            ents.append((i, term))
            i += 1
        term += int(rng.integers(1, 4))
    last = ents[-1][0]
    stable_last = int(rng.integers(off, last + 1))
    applied = int(rng.integers(off, stable_last + 1))
    snap_index = int(rng.integers(0, off + 1)) if rng.random() < 0.7 else int(
        rng.integers(off, applied + 1))
    snap_term = int(rng.integers(1, 9)) if snap_index else 0
    return R.Node(ents, stable_last + 1, applied, snap_index, snap_term)


def seeded_nodes(G: int, seed: int, spoil: bool = True) -> List[R.Node]:
    """Run counts 1..8 drawn evenly; with ``spoil`` a few groups hold a
    pending snapshot or cursors that contradict each other."""
    rng = np.random.default_rng(seed)
    nodes = [seeded_node(rng, 1 + (g + int(rng.integers(0, 2)) * 3) % MAX_RUNS) for g in range(G)]
    if spoil:
        for g in range(G):
            r = rng.random()
            n = nodes[g]
            if r < 0.03:
                n.usnap_index = n.last_index + 1
            elif r < 0.04:
                n.first_zero = True
            elif r < 0.05:
                n.unstable_offset = n.last_index + 2 + int(rng.integers(0, 3))   # stable_last > last
            elif r < 0.06:
                n.unstable_offset = n.ents[0][0]                                 # stable_last < off
            elif r < 0.09:
                n.snap_index = n.applied + 1 + int(rng.integers(0, 3))           # applied < snap_index
    return nodes


def _targets(rng, n: R.Node) -> List[int]:
    """Indexes that land on every path: each run's start and the index before
    it, stable_last, off, applied and its neighbours, past the end."""
    off, sl = n.ents[0][0], n.unstable_offset - 1
    rr = R.runs(n.ents)
    q = int(rng.integers(0, len(rr)))
    t = [rr[q][0], max(rr[q][0] - 1, 0), sl, off, off + 1, n.applied, n.applied + 1,
         n.last_index, n.last_index + 1, max(off - 1, 0), int(rng.integers(off, n.last_index + 2))]
    return [max(0, min(x, R.M64)) for x in t]


def seeded_explicit(nodes: List[R.Node], seed: int, idle: float = 0.2) -> R.Request:
    rng = np.random.default_rng(seed)
    G = len(nodes)
    s, c = [0] * G, [0] * G
    for g, n in enumerate(nodes):
        if rng.random() < idle:
            continue
        t = _targets(rng, n)
        kind = int(rng.integers(0, 3))
        if kind != 1:
            s[g] = int(rng.choice(t))
        if kind != 0:
            c[g] = int(rng.choice(t))
    return R.Request(R.CM_EXPLICIT, snap_at=s, compact_at=c)


def seeded_trigger(nodes: List[R.Node], seed: int, snapshot_count: int = 3,
                   catch_up_entries: int = 2) -> R.Request:
    rng = np.random.default_rng(seed)
    G = len(nodes)
    return R.Request(R.CM_TRIGGER, snapshot_count=snapshot_count, catch_up_entries=catch_up_entries,
                     force=[int(rng.random() < 0.3) * int(rng.integers(1, 256)) for _ in range(G)],
                     hold=[int(rng.random() < 0.2) for _ in range(G)])
