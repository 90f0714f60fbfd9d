"""Shared infrastructure of the follower-log-step tests: the golden tables as
append_ref nodes / records, packing to the engine's arrays (the run table
included), the expected arrays of one call from tests/append_ref.py, and a
seeded fuzz generator.  Test infrastructure."""
from __future__ import annotations

import copy
import json
import os

import numpy as np

from tests import append_ref as A, follower_pack as P, follower_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_RUNS = A.MAX_RUNS
FILL = 0xA5A5A5A5A5A5A5A5      # untouched output elements
STALE_START, STALE_TERM = 0xDEAD00000000DEAD, 0xBEEF00000000BEEF  # rows past the run count
META_KEEP = 0x0250_0A03        # other bits of the meta word (slots, read queue, bit 25): kept
FUZZ_SEEDS = (1, 2, 3)
FUZZ_G, FUZZ_M = 600, 2400


def load_tables():
    with open(os.path.join(ROOT, "tests", "golden", "append_tables.json"), encoding="utf-8") as f:
        return json.load(f)


def app(frm, term, index, log_term, ents, commit=0) -> A.AppRec:
    return A.AppRec(A.APP, frm, term, index, log_term, False, commit, list(ents))


def scenarios(tables=None):
    """Every row of the golden tables as (name, Config, LogNode, [AppRec]): a
    follower that is handed the row's message through raft.Step."""
    t = tables or load_tables()
    cfg = F.Config()
    out = []
    tb = t["handle_msg_app"]   # (stepped at the node's term: the test calls handleAppendEntries)
    for i, r in enumerate(tb["rows"]):
        n = A.new_node([0] + tb["log"], term=tb["term"], committed=tb["committed"])
        out.append((f"handle_msg_app#{i}", cfg, n,
                    [app(2, tb["term"], r["index"], r["log_term"], r["ents"], r["commit"])]))
    tb = t["find_conflict"]
    for i, r in enumerate(tb["rows"]):
        log = [0] + tb["log"]
        n = A.new_node(log, term=3)
        out.append((f"find_conflict#{i}", cfg, n,
                    [app(2, 3, r["first"] - 1, log[r["first"] - 1], r["ents"])]))
    tb = t["maybe_append"]
    for i, r in enumerate(tb["rows"]):
        n = A.new_node([0] + tb["log"], term=3, committed=tb["committed"])
        out.append((f"maybe_append#{i}", cfg, n,
                    [app(2, 3, r["index"], r["log_term"], r["ents"], r["commit"])]))
    for key in ("check_msg_app", "append_entries"):
        tb = t[key]
        for i, r in enumerate(tb["rows"]):
            n = A.new_node([0] + tb["log"], term=tb["term"], lead=tb["lead"],
                           committed=tb["committed"])
            out.append((f"{key}#{i}", cfg, n,
                        [app(tb["from"], tb["term"], r["index"], r["log_term"],
                             r.get("ents", []))]))
    tb = t["fast_log_rejection"]
    for i, r in enumerate(tb["rows"]):
        n = A.new_node([0] + r["follower_log"], term=0)
        lead = r["leader_log"]
        out.append((f"fast_log_rejection#{i}", cfg, n,
                    [app(tb["from"], tb["term"], len(lead), lead[-1], [tb["term"]])]))
    return out


# ---- packing -------------------------------------------------------------

def pack_log(nodes):
    """The qb_follower_log arrays of ``nodes``: meta (run count in bits 16-19
    over META_KEEP), first_index, and the run tables [MAX_RUNS, G] with the
    rows past a group's count holding STALE_* (the step must not read them as
    runs nor write them)."""
    G = len(nodes)
    meta = np.zeros(G, np.uint32)
    rs = np.full((MAX_RUNS, G), STALE_START, np.uint64)
    rt = np.full((MAX_RUNS, G), STALE_TERM, np.uint64)
    for g, n in enumerate(nodes):
        starts, terms = A.runs_of(n.terms, n.first_index)
        assert 1 <= len(starts) <= MAX_RUNS, f"group {g}: {len(starts)} runs"
        meta[g] = (META_KEEP & ~0xF0000) | (len(starts) << 16)
        rs[:len(starts), g] = np.array(starts, np.uint64)
        rt[:len(starts), g] = np.array(terms, np.uint64)
    return {"meta": meta, "first_index": np.array([n.first_index for n in nodes], np.uint64),
            "run_start": rs, "run_term": rt}


def pack_recs(recs):
    """recs: (group, Rec / AppRec) in arrival order -> (inbox arrays, app
    arrays).  A record's entries are run-length encoded; ``zero_runs`` /
    junk is left to the tests that want it."""
    inbox = P.pack_recs(recs)
    commit, off, et, el = [], [0], [], []
    for _, m in recs:
        if isinstance(m, A.AppRec):
            commit.append(m.commit)
            for t, n in A.rle(m.ents):
                et.append(t)
                el.append(n)
        else:
            commit.append(0)
        off.append(len(et))
    return inbox, {"commit": np.array(commit, np.uint64), "ent_off": np.array(off, np.uint32),
                   "ent_term": np.array(et, np.uint64), "ent_len": np.array(el, np.uint32)}


def expected(nodes, recs, cfg: F.Config, log0=None):
    """append_ref over a copy of ``nodes``: (group arrays after, log arrays
    after, outputs).  log0: the log arrays before (default pack_log(nodes));
    the table memory is modelled row by row: an append rewrites rows
    [0, new count) — equal to what was there below the first changed row — and
    leaves the others as they were."""
    after = copy.deepcopy(nodes)
    lg = copy.deepcopy(log0 if log0 is not None else pack_log(nodes))

    def on_append(g, n):
        starts, terms = A.runs_of(n.terms, n.first_index)
        lg["run_start"][:len(starts), g] = np.array(starts, np.uint64)
        lg["run_term"][:len(starts), g] = np.array(terms, np.uint64)
        lg["meta"][g] = (int(lg["meta"][g]) & ~0xF0000) | (len(starts) << 16)

    o = A.step_batch(after, recs, cfg, on_append=on_append)
    M = len(recs)

    def col(key, none):
        return np.array([none if v is None else v for v in o[key]], np.uint64).reshape(M)

    outs = {"resp_type": np.array(o["resp_type"], np.uint8),
            "resp_term": col("resp_term", 0), "resp_index": col("resp_index", 0),
            "app_from": col("app_from", 0), "resp_hint": col("resp_hint", FILL),
            "resp_log_term": col("resp_log_term", FILL),
            "stop_at": np.array(o["stop_at"], np.uint32),
            "gflags": np.array(o["gflags"], np.uint8), "stats": o["stats"]}
    return P.pack_nodes(after), lg, outs


# ---- fuzz ----------------------------------------------------------------

def _rand_log(rng, n, t0, step_p=0.3):
    out, t = [], t0
    for _ in range(n):
        if rng.random() < step_p:
            t += int(rng.integers(1, 3))
        out.append(t)
    return out


def cap_runs(terms, first_index=1, most=MAX_RUNS):
    """``terms`` cut at its end until it has at most ``most`` term runs."""
    terms = list(terms)
    while len(A.runs_of(terms, first_index)[0]) > most:
        terms.pop()
    return terms


def fuzz(seed: int, G: int = FUZZ_G, M: int = FUZZ_M):
    """(nodes, recs).  Every group has a leader-side log that shares a random
    prefix with the follower's (the follower's tail diverges, is shorter, or
    equal), first_index 1 or far up; records of every kind, the MsgApp cut
    from the leader's log at indexes below / inside / at the end of / past
    the follower's log, with a right or a wrong LogTerm, commits inside and
    past the new end, zero terms, and terms below / at / above the node's."""
    rng = np.random.default_rng(seed)
    nodes, leaders = [], []
    for _ in range(G):
        first = int(rng.choice([1, 1, 1, 7, 1 << 40]))
        dterm = int(rng.integers(0, 3)) if first > 1 else 0
        shared = _rand_log(rng, int(rng.integers(0, 12)), max(dterm, 1))
        base = shared[-1] if shared else max(dterm, 1)
        ltail = _rand_log(rng, int(rng.integers(0, 10)), base + int(rng.integers(0, 2)),
                          0.5 if rng.random() < 0.3 else 0.2)
        kind = rng.random()
        if kind < 0.4:
            ftail = []                                         # behind the leader
        elif kind < 0.6:
            ftail = ltail[:int(rng.integers(0, len(ltail) + 1))]  # a prefix of its tail
        else:                                                  # a divergent tail
            ftail = _rand_log(rng, int(rng.integers(1, 8)), base + int(rng.integers(0, 3)), 0.4)
        flog = cap_runs([dterm] + shared + ftail, first)
        llog = [dterm] + shared + ltail
        term = max(flog[-1], llog[-1]) + int(rng.integers(0, 2))
        role = int(rng.choice([F.FOLLOWER] * 7 + [F.CANDIDATE, F.LEADER, F.PRE_CANDIDATE]))
        if rng.random() < 0.7:
            role |= F.ROLE_PROMOTABLE
        n = A.new_node(flog, first, term=term, vote=int(rng.choice([0, 0, 1, 2, 3])),
                       lead=int(rng.choice([0, 1, 2, 3])), role=role,
                       election_elapsed=int(rng.choice([0, 9, 10, 13])),
                       heartbeat_elapsed=int(rng.integers(0, 4)))
        n.committed = first - 1 + int(rng.integers(0, min(len(shared), len(flog) - 1) + 1))
        nodes.append(n)
        leaders.append(llog)
    recs = []
    for _ in range(M):
        g = int(rng.integers(0, G))
        if rng.random() < 0.01:
            g = int(rng.choice([G, G + 7, 0xFFFFFFFF]))
        n, llog = (nodes[g], leaders[g]) if g < G else (nodes[0], leaders[0])
        dummy = n.first_index - 1
        kind = int(rng.choice([A.APP] * 14 + [F.HEARTBEAT] * 3 + [F.VOTE] * 2 + [F.PREVOTE] * 2 +
                              [F.TIMEOUT_NOW, F.HOST, int(rng.integers(6, 8))]))
        if kind in (F.TIMEOUT_NOW, F.HOST) and rng.random() < 0.6:
            kind = A.APP
        term = int(rng.choice([n.term] * 8 + [0, max(n.term - 1, 1), n.term + 1, n.term + 2]))
        frm = int(rng.integers(1, 4))
        if kind == A.APP:
            at = int(rng.integers(0, len(llog)))               # offset of Index in the leader's log
            if rng.random() < 0.35:
                at = min(len(llog), len(n.terms)) - 1           # around the follower's end
            k = int(rng.integers(0, 7))
            ents = llog[at + 1:at + 1 + k]
            log_term = llog[at]
            r = rng.random()
            if r < 0.06:
                log_term += 1                                    # a wrong LogTerm
            elif r < 0.10:
                ents = ents + [ents[-1] + 1 if ents else log_term + 1] * 2   # a newer term behind
            elif r < 0.13:
                at, log_term = len(n.terms) - 1, n.last_term     # zero terms past the end
                ents = [0] * int(rng.integers(1, 3))
            elif r < 0.16:
                at, log_term = len(n.terms) + int(rng.integers(0, 3)), 0   # "matches" past the end
            elif r < 0.19 and ents:
                ents = [t + 3 * j for j, t in enumerate(ents)]   # many runs
            index = dummy + at
            commit = int(rng.choice([0, dummy, index, index + len(ents), index + len(ents) + 2,
                                     dummy + int(rng.integers(0, len(n.terms) + 3))]))
            recs.append((g, A.AppRec(A.APP, frm, term, index, log_term, False, commit, ents)))
            continue
        if kind == F.HEARTBEAT:
            index = dummy + int(rng.integers(0, len(n.terms)))
            if rng.random() < 0.08:
                index = n.last_index + int(rng.integers(1, 12))
            aux = int(rng.choice([0, int(rng.integers(1, 1 << 62))]))
        else:
            index = max(0, n.last_index + int(rng.integers(-2, 4)))
            aux = max(0, n.last_term + int(rng.integers(-1, 3)))
        recs.append((g, F.Rec(kind, frm, term, index, aux, bool(rng.random() < 0.25))))
    return nodes, recs
