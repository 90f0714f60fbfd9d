"""Large batches for the step kernels from a small base batch: K copies of a
packed base of G0 groups laid end to end (G = K * G0), with the expected
outputs replicated the same way, so that a test at half a million groups costs
one run of the Python reference at G0 and a few numpy calls.

Every array of a call has a kind (how it is indexed), and one function here
replicates each kind.  ``Case`` holds one entry point's call over a base batch
as {name: (kind, array)} dicts: the arrays before, and per call the arrays
after, the outputs (elements a call must not touch keep their pre-fill) and
the accumulated stats; the ``*_case`` functions build it from the reference's
objects with the packers the small tests use.  ``replicate`` turns an active
and an idle Case over the same table shape into the Case of K copies, each
copy the one or the other.  tests/test_replicate.py holds it to the slow
path (3 * G0 objects packed and stepped) for every entry point.

Test infrastructure."""
from __future__ import annotations

import copy
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

from tests import append_pack as AP, campaign_pack as CP, follower_pack as FP
from tests import propose_pack as PP, request_pack as QP, tick_pack as TP
from tests import campaign_ref as CR, propose_ref as PR, request_ref as QR, tick_ref as TR

# kinds
GROUP = "group"      # [G0 * c], group-major (c entries per group)
SLOT = "slot"        # [S0 * c], slot-major
OFF = "off"          # [G0 + 1] slot offsets
ROWS = "rows"        # [R * G0], row-major: row r of group g at r * G0 + g (also as [R, G0])
REC = "rec"          # [M0] per record
REC_GROUP = "rgrp"   # [M0] the records' group column
ENT_OFF = "entoff"   # [M0 + 1] offsets of the records' entry runs
ENT = "ent"          # [E0] entry runs, in record order
STOP = "stop"        # [G0] u32 batch positions, NO_STOP = none
NO_STOP = 0xFFFFFFFF

Arrays = Dict[str, Tuple[str, np.ndarray]]


@dataclass
class Case:
    """One entry point over one batch.  ``calls``: per consecutive call
    (arrays after + outputs, stats accumulated up to and including it)."""
    G: int
    inp: Arrays
    calls: List[Tuple[Arrays, Dict[str, int]]] = field(default_factory=list)
    M: int = 0          # records (REC arrays)

    def arr(self, name):
        return self.inp[name][1]


# --------------------------------------------------------- one kind each ---

def rep_group(bases, which):
    """Per-group arrays: copy c is bases[which[c]], end to end."""
    return np.concatenate([bases[w] for w in which])


rep_slot = rep_group    # per-slot arrays: the same (every base has the same off)


def rep_off(off, K):
    """Copy c's offsets shifted by c * S0; a single closing entry last."""
    off = np.asarray(off)
    S0 = int(off[-1])
    out = (off[:-1].astype(np.int64)[None, :] + S0 * np.arange(K, dtype=np.int64)[:, None]).reshape(-1)
    out = np.concatenate([out, [K * S0]])
    assert out[-1] < 1 << 32
    return out.astype(off.dtype)


def rep_rows(bases, which, G0):
    """Row-major arrays: each base as (R, G0), tiled along the group axis
    (not concatenated: row r of the result holds row r of every copy).
    Returns (R, K * G0)."""
    return np.concatenate([np.asarray(bases[w]).reshape(-1, G0) for w in which], axis=1)


def rep_rec(x, Ka):
    """Per-record arrays: the Ka copies that hold records are interleaved,
    record i of the j-th of them at i * Ka + j, which keeps each group's own
    order and spreads every group's records over the batch."""
    return np.repeat(x, Ka)


def rep_rec_group(group, act, K, G0):
    """The group column: + c * G0 for the copy c the record belongs to; a
    group outside the base (>= G0) stays outside the result (>= K * G0)."""
    g = np.repeat(np.asarray(group).astype(np.int64), len(act))
    c = np.tile(np.asarray(act, np.int64), len(group))
    out = np.where(g < G0, g + c * G0, np.minimum(g - G0 + K * G0, 0xFFFFFFFF))
    return out.astype(np.uint32)


def rep_ent_off(ent_off, Ka):
    """The entry runs follow their records: record i * Ka + j holds the runs
    of base record i, so the offsets are the prefix sums of the base's run
    counts repeated Ka times (an offset column cannot name copy-major ranges
    for interleaved records)."""
    lens = np.diff(np.asarray(ent_off).astype(np.int64))
    out = np.concatenate([[0], np.cumsum(np.repeat(lens, Ka))])
    assert out[-1] < 1 << 32
    return out.astype(np.uint32)


def rep_ent(x, ent_off, Ka):
    """An entry-run column in the order rep_ent_off lays out."""
    off = np.asarray(ent_off).astype(np.int64)
    lens = np.repeat(np.diff(off), Ka)                       # per new record
    start = np.repeat(off[:-1], Ka)                          # its runs in the base
    new0 = np.concatenate([[0], np.cumsum(lens)])[:-1]
    idx = np.repeat(start - new0, lens) + np.arange(int(lens.sum()))
    return np.asarray(x)[idx]


def rep_stop(bases, which, act):
    """stop_at: a batch position i of the j-th record-holding copy becomes
    i * Ka + j; NO_STOP stays."""
    Ka = len(act)
    rank = {c: j for j, c in enumerate(act)}
    out = []
    for c, w in enumerate(which):
        v = bases[w].astype(np.int64)
        if c in rank:
            v = np.where(v == NO_STOP, NO_STOP, v * Ka + rank[c])
        else:
            assert (v == NO_STOP).all()
        out.append(v)
    return np.concatenate(out).astype(np.uint32)


def rep_stats(stats, which):
    """Each base's counters times the number of its copies."""
    n = [sum(1 for w in which if w == b) for b in range(len(stats))]
    return {k: sum(n[b] * stats[b][k] for b in range(len(stats)) if n[b]) for k in stats[0]}


# ------------------------------------------------------------ whole cases ---

def _rep_arrays(dicts, which, act, K, G0, ent_off=None):
    """dicts[b]: base b's {name: (kind, array)}; records come from base 0."""
    out = {}
    Ka = len(act)
    for name, (kind, _) in dicts[0].items():
        xs = [d[name][1] for d in dicts]
        if kind in (GROUP, SLOT):
            v = rep_group(xs, which)
        elif kind == OFF:
            assert all(np.array_equal(x, xs[0]) for x in xs), "the bases differ in off"
            v = rep_off(xs[0], K)
        elif kind == ROWS:
            v = rep_rows(xs, which, G0)
        elif kind == REC:
            v = rep_rec(xs[0], Ka)
        elif kind == REC_GROUP:
            v = rep_rec_group(xs[0], act, K, G0)
        elif kind == ENT_OFF:
            v = rep_ent_off(xs[0], Ka)
        elif kind == ENT:
            v = rep_ent(xs[0], ent_off, Ka)
        elif kind == STOP:
            v = rep_stop(xs, which, act)
        else:
            raise ValueError(kind)
        out[name] = (kind, v)
    return out


def replicate(bases: List[Case], which) -> Case:
    """K = len(which) copies, copy c being bases[which[c]].  Base 0 is the
    active one; the others hold no records and share its table shape."""
    which = [int(w) for w in which]
    K, G0 = len(which), bases[0].G
    assert all(b.G == G0 and len(b.calls) == len(bases[0].calls) for b in bases)
    assert all(b.M == 0 for b in bases[1:]), "only base 0 may hold records"
    act = [c for c, w in enumerate(which) if w == 0]
    ent_off = bases[0].inp["ent_off"][1] if "ent_off" in bases[0].inp else None
    out = Case(K * G0, _rep_arrays([b.inp for b in bases], which, act, K, G0, ent_off),
               M=bases[0].M * len(act))
    for k in range(len(bases[0].calls)):
        out.calls.append((_rep_arrays([b.calls[k][0] for b in bases], which, act, K, G0, ent_off),
                          rep_stats([b.calls[k][1] for b in bases], which)))
    return out


def mismatches(got: Arrays, want: Arrays):
    """Names whose arrays differ (integer equality over every element)."""
    assert got.keys() == want.keys(), (sorted(got), sorted(want))
    return [k for k in want if not np.array_equal(np.asarray(got[k][1]).reshape(-1),
                                                  np.asarray(want[k][1]).reshape(-1))]


# ------------------------------------------------- the six entry points ---

LEADER_KINDS = {"off": OFF, "run_start": ROWS, "run_term": ROWS, "match": SLOT, "next": SLOT,
                "pending_snapshot": SLOT, "pstate": SLOT, "infl_pos": SLOT, "infl_buf": SLOT}


def _table(a, prefix=""):
    return {prefix + k: (LEADER_KINDS.get(k, GROUP), v) for k, v in a.items()}


def _cols(d, kind, prefix=""):
    return {prefix + k: (kind, np.array(v, copy=True)) for k, v in d.items()}


def tick_case(nodes, readq_cap, et, ht, cq, nticks=2) -> Case:
    """``nticks`` consecutive ticks (tick_ref) over a copy of ``nodes``."""
    nodes = copy.deepcopy(nodes)
    a, t = TP.pack_nodes(nodes, readq_cap)
    G, S = len(nodes), int(a["off"][-1])
    case = Case(G, {**_table(a), **_cols(t, GROUP, "t.")})
    hb_commit, hb_ctx = np.full(S, TP.FILL, np.uint64), np.full(G, TP.FILL, np.uint64)
    stats = {k: 0 for k in TR.TSTAT_NAMES}
    for _ in range(nticks):
        tf, st = TP.ref_tick(nodes, a["off"], et, ht, cq, hb_commit, hb_ctx)
        stats = {k: stats[k] + st[k] for k in stats}
        a2, t2 = TP.pack_nodes(nodes, readq_cap)
        case.calls.append(({**_table(a2), **_cols(t2, GROUP, "t."), "tflags": (GROUP, tf),
                            "hb_commit": (SLOT, hb_commit.copy()),
                            "hb_ctx": (GROUP, hb_ctx.copy())}, dict(stats)))
    return case


def tick_idle(nodes):
    """The same table with timers that cannot fire: promotable followers far
    from their randomized timeout (tflags 0, only election_elapsed moves)."""
    nodes = copy.deepcopy(nodes)
    for n in nodes:
        n.role = TR.FOLLOWER | TR.ROLE_PROMOTABLE
        n.election_elapsed, n.heartbeat_elapsed, n.rand_timeout = 0, 0, 1 << 20
    return nodes


def _election(a, e):
    """The election state as ElectionState.numpy() names it."""
    e = dict(e)
    e.update(term=a["term"], committed=a["committed"], last_index=a["last_index"])
    return _cols(e, GROUP, "e.")


def campaign_case(nodes, action, pre_vote, readq_cap) -> Case:
    nodes = copy.deepcopy(nodes)
    action = np.asarray(action, np.uint8)
    a, e = CP.pack_nodes(nodes, readq_cap)
    G = len(nodes)
    case = Case(G, {**_table(a), **_election(a, e), "action": (GROUP, action)})
    req_term, req_mask = np.full(G, CP.FILL, np.uint64), np.full(G, 0xA5A5, np.uint16)
    cf, rt, st = CP.ref_campaign(nodes, action, pre_vote, req_term, req_mask)
    a2, e2 = CP.pack_nodes(nodes, readq_cap)
    for k in ("rq_ctx", "rq_index", "rq_meta"):   # dead after a reset, never written
        a2[k] = a[k]
    case.calls.append(({**_table(a2), **_election(a2, e2), "cflags": (GROUP, cf),
                        "req_type": (GROUP, rt), "req_term": (GROUP, req_term),
                        "req_mask": (GROUP, req_mask)}, dict(st)))
    return case


def propose_case(nodes, inp, cfg: PR.Config) -> Case:
    nodes = copy.deepcopy(nodes)
    a, e, p = PP.pack_nodes(nodes)
    G, S = len(nodes), int(a["off"][-1])
    case = Case(G, {**_table(a), **_election(a, e), **_cols(p, GROUP, "p."),
                    **_cols(inp, GROUP, "in.")})
    msg = PP.new_msg(S)
    pf, st, _ = PP.ref_propose(nodes, inp, cfg, a["off"], msg)
    a2, e2, p2 = PP.pack_nodes(nodes)
    case.calls.append(({**_table(a2), **_election(a2, e2), **_cols(p2, GROUP, "p."),
                        "pflags": (GROUP, pf), **_cols(msg, SLOT)}, dict(st)))
    return case


REQ_IN_KINDS = {"n_reads": GROUP, "rd_ctx": ROWS, "rd_from": ROWS, "xf_from": GROUP,
                "xf_term": GROUP}
REQ_OUT_KINDS = {"rd_status": ROWS, "rd_index": ROWS, "hb_commit": SLOT, "xf_type": GROUP,
                 "xf_index": GROUP, "xf_log_term": GROUP, "xf_n": GROUP, "qflags": GROUP}


def requests_case(nodes, inp, cfg: QR.Config) -> Case:
    nodes = copy.deepcopy(nodes)
    a, e = QP.pack_nodes(nodes, cfg.readq_cap)
    G, S = len(nodes), int(a["off"][-1])
    case = Case(G, {**_table(a), **_election(a, e),
                    **{"in." + k: (REQ_IN_KINDS[k], v.copy()) for k, v in inp.items()}})
    out = QP.new_out(G, S, cfg.max_reads)
    st, _ = QP.ref_requests(nodes, inp, cfg, a["off"], out)
    a2, e2 = QP.pack_nodes(nodes, cfg.readq_cap)
    case.calls.append(({**_table(a2), **_election(a2, e2),
                        **{k: (REQ_OUT_KINDS[k], v) for k, v in out.items()}}, dict(st)))
    return case


def requests_idle_inputs(G, max_reads):
    return QP.inputs(G, max_reads, [[] for _ in range(G)])


def _inbox(r):
    return {"r." + k: (REC_GROUP if k == "group" else REC, v) for k, v in r.items()}


def follower_case(nodes, recs, cfg) -> Case:
    a = FP.pack_nodes(nodes)
    after, want = FP.expected(nodes, recs, cfg)
    case = Case(len(nodes), {**_cols(a, GROUP), **_inbox(FP.pack_recs(recs))}, M=len(recs))
    case.calls.append(({**_cols(after, GROUP), "resp_type": (REC, want["resp_type"]),
                        "resp_term": (REC, want["resp_term"]), "stop_at": (STOP, want["stop_at"]),
                        "gflags": (GROUP, want["gflags"])}, dict(want["stats"])))
    return case


LOG_KINDS = {"meta": GROUP, "first_index": GROUP, "run_start": ROWS, "run_term": ROWS}
APP_KINDS = {"commit": REC, "ent_off": ENT_OFF, "ent_term": ENT, "ent_len": ENT}
LOG_REC_OUT = ("resp_type", "resp_term", "resp_index", "resp_hint", "resp_log_term", "app_from")


def follower_log_case(nodes, recs, cfg) -> Case:
    a, lg = FP.pack_nodes(nodes), AP.pack_log(nodes)
    r, ap = AP.pack_recs(recs)
    after, lg2, want = AP.expected(nodes, recs, cfg)
    case = Case(len(nodes), {**_cols(a, GROUP), **{"l." + k: (LOG_KINDS[k], v) for k, v in lg.items()},
                             **_inbox(r), **{k: (APP_KINDS[k], v) for k, v in ap.items()}},
                M=len(recs))
    case.calls.append(({**_cols(after, GROUP),
                        **{"l." + k: (LOG_KINDS[k], v) for k, v in lg2.items()},
                        **{k: (REC, want[k]) for k in LOG_REC_OUT},
                        "stop_at": (STOP, want["stop_at"]), "gflags": (GROUP, want["gflags"])},
                       dict(want["stats"])))
    return case


def interleaved_records(recs, copies, K, G0):
    """The slow path's record list: ``recs`` once per copy in ``copies``,
    record i of the j-th of them at i * len(copies) + j, the group moved as
    rep_rec_group moves it."""
    out = []
    for g, m in recs:
        for c in copies:
            out.append((g + c * G0 if g < G0 else min(g - G0 + K * G0, 0xFFFFFFFF),
                        copy.deepcopy(m)))
    return out
