"""Shared infrastructure of the switch-config tests: seeded random batches in
the engine's packed arrays (the old and the new config of every group, the
group words, the new Progress), the golden cases packed the same way, and the
reference outputs of one call from tests/switch_ref.py.  Test infrastructure."""
from __future__ import annotations

import json
import os

import numpy as np

from tests import switch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFLIGHT_CAP = 2
MAX_RUNS = R.MAX_RUNS
GROUP_U64 = ("self_id", "term", "first_index", "last_index", "last_term", "snap_index", "snap_term",
             "max_ents", "committed")
SLOT_KEYS = ("match", "next", "pending_snapshot", "pstate", "infl_pos")
# what a call may change, compared bit for bit behind it
INOUT = ("meta", "committed", "votes", "rq_meta", "match", "next", "pending_snapshot", "pstate",
         "infl_pos", "infl_buf")


def load_tables():
    with open(os.path.join(ROOT, "tests", "golden", "switch_tables.json"), encoding="utf-8") as f:
        return json.load(f)


def group(old_ids, ids, voters, voters_out=(), *, self_id, role=R.LEADER, term=1, terms=(0, 1),
          first=1, committed=0, progress=None, transferee=0, votes=None, reads=(), cap=INFLIGHT_CAP,
          max_ents=1 << 62, snap_index=None, snap_term=None, own_slot=None, xf_slot=None,
          pending_readindex=False):
    """One group by raft IDs.  ``terms``: the log's terms for [first - 1 ..
    last]; ``progress``: new ID -> dict(match, next, state, recent_active,
    probe_sent, pending_snapshot, ring, start), default a quiet probe at next =
    last + 1; ``votes``: ID -> granted; ``reads``: (ack IDs, From ID or 0);
    ``own_slot`` / ``xf_slot`` override the slots derived from the IDs."""
    old_ids, ids = sorted(old_ids), sorted(ids)
    last = first - 1 + len(terms) - 1
    return dict(old_ids=old_ids, ids=ids, voters=set(voters), voters_out=set(voters_out),
                self_id=self_id, role=role, term=term, terms=list(terms), first=first,
                last=last, committed=committed, progress=progress or {}, transferee=transferee,
                votes=votes or {}, reads=list(reads), cap=cap, max_ents=max_ents,
                snap_index=first - 1 if snap_index is None else snap_index,
                snap_term=terms[0] if snap_term is None else snap_term, own_slot=own_slot,
                xf_slot=xf_slot, pending_readindex=pending_readindex)


def runs_of(terms, first):
    starts, rterms = [first - 1], [terms[0]]
    for k, t in enumerate(terms[1:], 1):
        if t != rterms[-1]:
            starts.append(first - 1 + k)
            rterms.append(t)
    return starts, rterms


def pack(groups, Q=0, cap=INFLIGHT_CAP, pad=0):
    """The engine's arrays of a batch of ``group`` dicts.  ``pad``: unused
    slot elements behind every group's new slots (a table with gaps)."""
    G = len(groups)
    a = {"old_off": np.zeros(G + 1, np.uint32), "off": np.zeros(G + 1, np.uint32),
         "cfg": np.zeros(G, np.uint32), "meta": np.zeros(G, np.uint32),
         "role": np.zeros(G, np.uint8), "votes": np.zeros(G, np.uint32),
         "run_start": np.zeros(MAX_RUNS * G, np.uint64), "run_term": np.zeros(MAX_RUNS * G, np.uint64),
         "rq_meta": np.zeros(max(G * Q, 1), np.uint32)}
    for k in GROUP_U64:
        a[k] = np.zeros(G, np.uint64)
    a["old_off"][1:] = np.cumsum([len(x["old_ids"]) for x in groups])
    a["off"][1:] = np.cumsum([len(x["ids"]) + pad for x in groups])
    S0, S = int(a["old_off"][-1]), int(a["off"][-1])
    a["old_ids"] = np.full(max(S0, 1), R.FILL, np.uint64)
    a["ids"] = np.full(max(S, 1), R.FILL, np.uint64)
    a["match"] = np.full(max(S, 1), R.FILL, np.uint64)
    a["next"] = np.full(max(S, 1), R.FILL, np.uint64)
    a["pending_snapshot"] = np.full(max(S, 1), R.FILL, np.uint64)
    a["pstate"] = np.full(max(S, 1), R.FILL8, np.uint8)
    a["infl_pos"] = np.zeros(max(S, 1), np.uint32)
    a["infl_buf"] = np.full(max(S * cap, 1), R.FILL, np.uint64)
    for g, x in enumerate(groups):
        o0, s0 = int(a["old_off"][g]), int(a["off"][g])
        old_slot = {i: k for k, i in enumerate(x["old_ids"])}
        slot = {i: k for k, i in enumerate(x["ids"])}
        a["old_ids"][o0:o0 + len(old_slot)] = x["old_ids"]
        a["ids"][s0:s0 + len(slot)] = x["ids"]
        a["cfg"][g] = sum(1 << slot[i] for i in x["voters"]) | \
            sum(1 << slot[i] for i in x["voters_out"]) << 16
        starts, rterms = runs_of(x["terms"], x["first"])
        assert len(starts) <= MAX_RUNS
        for r, (s, t) in enumerate(zip(starts, rterms)):
            a["run_start"][r * G + g], a["run_term"][r * G + g] = s, t
        own = old_slot.get(x["self_id"], 0xFF) if x["own_slot"] is None else x["own_slot"]
        xf = (old_slot[x["transferee"]] if x["transferee"] else 0xFF) if x["xf_slot"] is None \
            else x["xf_slot"]
        assert len(x["reads"]) <= Q
        a["meta"][g] = own | xf << 8 | len(starts) << 16 | len(x["reads"]) << 20 | \
            (1 << 25 if x["pending_readindex"] else 0)
        for k, (acks, frm) in enumerate(x["reads"]):
            a["rq_meta"][g * Q + k] = sum(1 << old_slot[i] for i in acks) | \
                (old_slot[frm] if frm else 0xFF) << 16
        a["votes"][g] = sum(1 << old_slot[i] for i in x["votes"]) | \
            sum(1 << old_slot[i] for i, ok in x["votes"].items() if ok) << 16
        for k, v in (("self_id", x["self_id"]), ("term", x["term"]), ("first_index", x["first"]),
                     ("last_index", x["last"]), ("last_term", x["terms"][-1]),
                     ("snap_index", x["snap_index"]), ("snap_term", x["snap_term"]),
                     ("max_ents", x["max_ents"]), ("committed", x["committed"])):
            a[k][g] = v
        a["role"][g] = x["role"]
        for i, k in slot.items():
            p = dict(match=0, next=x["last"] + 1, state=R.PROBE, recent_active=True,
                     probe_sent=False, pending_snapshot=0, ring=(), start=0)
            p.update(x["progress"].get(i, x["progress"].get(str(i), {})))
            j = s0 + k
            a["match"][j], a["next"][j] = p["match"], p["next"]
            a["pending_snapshot"][j] = p["pending_snapshot"]
            a["pstate"][j] = p["state"] | (R.PROBE_SENT if p["probe_sent"] else 0) | \
                (R.RECENT_ACTIVE if p["recent_active"] else 0)
            a["infl_pos"][j] = p["start"] | len(p["ring"]) << 16
            for q, v in enumerate(p["ring"]):
                a["infl_buf"][j * cap + (p["start"] + q) % cap] = v
    return a


def ref_call(a, action, Q, out, stats, cap=INFLIGHT_CAP):
    """One call through switch_ref over the arrays (in place); the stats
    accumulate.  Returns the messages per group."""
    return R.switch_config(a, action, cap, Q, out, stats)


def lay(a, K, Q=0):
    """The arrays (or outputs) of a batch laid end to end K times: copy c holds
    the groups [c * G, (c + 1) * G) and their slots behind the copy before."""
    G = len(a["cfg"]) if "cfg" in a else None
    out = {}
    for k, v in a.items():
        if k in ("off", "old_off"):
            n = int(v[-1])
            out[k] = np.concatenate([(v[:-1].astype(np.uint64)[None, :] +
                                      (np.arange(K, dtype=np.uint64) * n)[:, None]).reshape(-1),
                                     [K * n]]).astype(np.uint32)
        elif k in ("run_start", "run_term"):
            out[k] = np.tile(v.reshape(MAX_RUNS, G), (1, K)).reshape(-1)
        elif k == "rq_meta" and Q == 0:
            out[k] = v.copy()
        else:
            out[k] = np.tile(v, K)
    return out


def vote_patterns():
    """Every voted / granted bit pattern on a removed slot, on a moved slot
    and on a kept one: candidates of (2, 3, 4) that become (1, 2, 4) — 3 is
    removed, 1 is added in front, so slot 0 -> 1 and slot 2 -> 2.  Returns
    (arrays, action, the votes words and the VOTE_DROPPED bits expected)."""
    pats = [(v, g_) for v in range(8) for g_ in range(8)]      # 3 voted x 3 granted bits
    groups = [group([2, 3, 4], [1, 2, 4], [1, 2, 4], self_id=2, role=1, term=2) for _ in pats]
    a = pack(groups)
    move = lambda m: (m & 1) << 1 | (m & 4)                    # noqa: E731  (bit 1 is dropped)
    a["votes"][:] = [v | g_ << 16 for v, g_ in pats]
    want = np.array([move(v) | move(g_) << 16 for v, g_ in pats], np.uint32)
    dropped = np.array([bool(v & 2) for v, _ in pats])
    return a, np.full(len(pats), R.SW_SWITCH, np.uint8), want, dropped


# ----------------------------------------------------------------- batches ---

def random_terms(rng, term, max_len=24):
    """A log's terms, non-decreasing, ending at or below ``term``, in at most
    MAX_RUNS runs."""
    n = int(rng.integers(1, max_len + 1))
    last_t = term if rng.random() < 0.75 else max(1, term - int(rng.integers(1, 3)))
    k = min(int(rng.choice([1, 1, 2, 3, 8])), n, last_t)
    ts = sorted(int(x) for x in rng.choice(np.arange(1, last_t), k - 1, replace=False)) + [last_t]
    cuts = sorted(int(x) for x in rng.choice(np.arange(1, n), k - 1, replace=False)) if k > 1 else []
    bounds = [0] + cuts + [n]
    out = []
    for r in range(k):
        out += [ts[r]] * (bounds[r + 1] - bounds[r])
    return out


def random_group(rng, Q, cap=INFLIGHT_CAP, n_new=None):
    """Adds, removes, promotions and demotions, joint configs, the own slot
    first / last / removed / a learner, a transferee kept / demoted / removed,
    pending reads whose From stays or goes, votes with every bit pattern on
    removed slots, Progress in every state with rings empty to full, next
    below first_index, every role."""
    pool = np.arange(1, 41)
    n_old = int(rng.integers(1, 17))
    old_ids = sorted(int(x) for x in rng.choice(pool, n_old, replace=False))
    kind = rng.random()
    if kind < 0.15:
        ids = list(old_ids)                                        # promotions / demotions only
    else:
        keep = [i for i in old_ids if rng.random() < 0.8]
        rest = [int(x) for x in pool if x not in old_ids]
        add = [int(x) for x in rng.choice(rest, int(rng.integers(0, 4)), replace=False)]
        ids = sorted(keep + add)[:16]
        if kind > 0.97:
            ids = sorted(int(x) for x in rng.choice(rest, int(rng.integers(1, 5)), replace=False))
    if n_new is not None:                                          # a fixed new size
        rest = [int(x) for x in pool if x not in ids]
        ids = sorted((ids + rest)[:n_new])
    if not ids and rng.random() < 0.7:
        ids = [int(rng.choice(pool))]
    r = rng.random()
    if r < 0.55 and ids:
        self_id = ids[0] if r < 0.1 else ids[-1] if r < 0.2 else int(rng.choice(ids))
    elif r < 0.9:
        self_id = int(rng.choice(old_ids))
    else:
        self_id = int(rng.integers(41, 50))                        # never a member
    voters = {i for i in ids if rng.random() < 0.75}
    if rng.random() < 0.85:
        voters |= {self_id} & set(ids)
    if rng.random() < 0.04:
        voters = set()
    voters_out = {i for i in ids if rng.random() < 0.5} if rng.random() < 0.3 else set()
    term = int(rng.integers(1, 12))
    terms = random_terms(rng, term)
    first = int(rng.integers(1, 40))
    last = first - 1 + len(terms) - 1
    committed = int(rng.integers(first - 1, last + 1))
    hot = rng.random() < 0.5                                       # a quorum at the log's end
    progress = {}
    for i in ids:
        state = int(rng.choice([0, 0, 1, 1, 1, 2]))
        match = last if hot and rng.random() < 0.8 else int(rng.integers(0, last + 1))
        nxt = match + 1 + int(rng.integers(0, 3))
        if rng.random() < 0.3:
            nxt = int(rng.integers(max(1, first - 3), last + 3))   # also below first_index
        ring, start = (), 0
        if state == R.REPLICATE:
            ring = tuple(match + 1 + q for q in range(int(rng.integers(0, cap + 1))))
            start = int(rng.integers(0, cap))
        if i not in old_ids and rng.random() < 0.7:                # initProgress
            state, match, nxt, ring, start = R.PROBE, 0, last, (), 0
        progress[i] = dict(match=match, next=nxt, state=state, recent_active=bool(rng.random() < 0.7),
                           probe_sent=bool(rng.random() < 0.25),
                           pending_snapshot=int(rng.integers(0, last + 3)) if state == 2 else 0,
                           ring=ring, start=start)
    role = int(rng.choice([R.LEADER] * 7 + [0, 1, 3]))
    transferee = int(rng.choice(old_ids)) if rng.random() < 0.3 else 0
    votes = {i: bool(rng.random() < 0.5) for i in old_ids if rng.random() < 0.5}
    reads = []
    for _ in range(int(rng.integers(0, Q + 1)) if Q else 0):
        stay = [i for i in old_ids if i in ids]
        frm = 0 if rng.random() < 0.5 or not stay else int(rng.choice(stay))
        if rng.random() < 0.03:
            frm = int(rng.choice(old_ids))                         # may be gone: stop (a)
        reads.append(([i for i in old_ids if rng.random() < 0.4], frm))
    x = group(old_ids, ids, voters, voters_out, self_id=self_id, role=role, term=term, terms=terms,
              first=first, committed=committed, progress=progress, transferee=transferee,
              votes=votes, reads=reads, cap=cap, max_ents=int(rng.choice([1, 2, 5, 1 << 62])),
              snap_index=0 if rng.random() < 0.2 else first - 1,
              pending_readindex=bool(rng.random() < 0.2))
    if rng.random() < 0.03:
        x["own_slot"] = int(rng.choice([n_old, 16, 0xFE, 0xFF]))    # a stale own slot: recomputed
    if rng.random() < 0.02:
        x["xf_slot"] = int(rng.choice([n_old, 16, 0xFE]))           # a transferee that names no member
    return x


def random_batch(rng, G, Q=0, cap=INFLIGHT_CAP, p_act=1.0, n_new=None, pad=0):
    """(arrays, action) of a seeded batch; also votes / rq_meta bits beyond
    the old slots now and then."""
    groups = [random_group(rng, Q, cap, n_new) for _ in range(G)]
    a = pack(groups, Q, cap, pad)
    wild = rng.random(G) < 0.05
    a["votes"][wild] = rng.integers(0, 1 << 32, int(wild.sum()), dtype=np.uint64).astype(np.uint32)
    action = rng.choice([R.SW_SWITCH] * 3 + [R.SW_RESTORE], G).astype(np.uint8)
    action[rng.random(G) >= p_act] = R.SW_NONE
    bad = rng.random(G) < 0.02
    action[bad] = rng.choice([3, 5, 0x41, 0xFF], int(bad.sum())).astype(np.uint8)
    return a, action
