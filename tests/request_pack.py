"""Shared infrastructure of the request tests: RequestNodes from plain
arguments and from the golden scenarios, a seeded random batch, packing to the
engine's arrays (tests/propose_pack.py and tests/campaign_pack.py for the
arrays the call shares with the proposal and the campaign), and the expected
outputs of one call from tests/request_ref.py.  Test infrastructure."""
from __future__ import annotations

import json
import os

import numpy as np

from oracle import leader_ref as L
from tests import campaign_pack as CP, propose_pack as P, request_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = CP.FILL          # the outputs' pre-fill: untouched elements keep it
FILL8 = 0xA5
FILL32 = 0xA5A5A5A5
INFLIGHT_CAP = P.INFLIGHT_CAP
NO_SLOT = R.NO_SLOT
STATUS = {"read_state": R.RD_READ_STATE, "resp": R.RD_RESP, "bcast": R.RD_BCAST,
          "bcast_dup": R.RD_BCAST_DUP, "postponed": R.RD_POSTPONED, "forward": R.RD_FORWARD,
          "dropped": R.RD_DROPPED, "ignored": R.RD_IGNORED}
OUT_KEYS = ("rd_status", "rd_index", "hb_commit", "xf_type", "xf_index", "xf_log_term", "xf_n",
            "qflags")


def load_tables():
    with open(os.path.join(ROOT, "tests", "golden", "request_tables.json"), encoding="utf-8") as f:
        return json.load(f)


def make_node(ns, mask_in, mask_out, own, *, readq=(), pending=False, ee=0, **kw) -> R.RequestNode:
    """P.make_node plus the read queue ([(ctx, index, ack slots, from slot)],
    oldest first), the postponed-reads bit and election_elapsed."""
    prop = P.make_node(ns, mask_in, mask_out, own, **kw)
    g = prop.group
    g.readq = [L.ReadIndexStatus(c, i, set(acks), frm) for c, i, acks, frm in readq]
    g.pending_readindex = bool(pending)
    prop.camp.election_elapsed = ee
    return R.new_node(prop)


def _progress(p, cap):
    return P.progress(p["match"], p["next"], p["state"], p["recent_active"], p["probe_sent"],
                      p.get("pending_snapshot", 0), ring=tuple(p.get("ring", ())), cap=cap)


def build_node(sc) -> R.RequestNode:
    """A golden scenario's node: slot j is the j-th smallest ID."""
    nd = sc["node"]
    ids = nd["ids"]
    slot = {i: s for s, i in enumerate(ids)}
    cap = nd["inflight_cap"]
    return make_node(len(ids), sum(1 << slot[i] for i in nd["voters"]),
                     sum(1 << slot[i] for i in nd["voters_out"]), slot[nd["self"]],
                     terms=nd["terms"], term=nd["term"], first=nd["first"], role=nd["state"],
                     lead=nd["lead"], committed=nd["committed"],
                     prs=[_progress(nd["progress"][str(i)], cap) for i in ids],
                     transferee=slot[nd["transferee"]] if nd["transferee"] else NO_SLOT, cap=cap,
                     max_ents=nd["max_ents"], applied=nd["applied"], self_id=nd["self"],
                     ee=nd["election_elapsed"])


def check_expect(where, exp, res: R.Result, n: R.RequestNode, ids):
    """res: the Result of the call (or its equal read back from the device);
    n: the node behind it."""
    g = n.group
    to_id = lambda s: 0 if s == NO_SLOT else ids[s]  # noqa: E731
    if "status" in exp:
        assert res.reads[0][0] == STATUS[exp["status"]], f"{where}: status {res.reads[0][0]}"
        if exp["status"] in ("read_state", "resp"):
            assert res.reads[0][1] == exp["index"], f"{where}: read index {res.reads[0][1]}"
    if "heartbeats" in exp:
        got = [[ids[s], c] for s, c in (res.heartbeats or [])]
        assert got == exp["heartbeats"], f"{where}: heartbeats {got}, want {exp['heartbeats']}"
    if "queue" in exp:
        got = [[r.ctx, r.index, sorted(ids[s] for s in r.acks), to_id(r.from_slot)]
               for r in g.readq]
        assert got == exp["queue"], f"{where}: queue {got}, want {exp['queue']}"
        if exp["status"] in ("bcast", "bcast_dup"):
            assert got[-1][1] == exp["index"], f"{where}: queued index {got[-1][1]}"
    if "pending" in exp:
        assert g.pending_readindex == exp["pending"], f"{where}: pending {g.pending_readindex}"
    if "msg" in exp:
        t, idx, lt, k = res.xf
        got = None
        if t:
            app = t == R.MSG_APP
            got = [t, None, idx, lt, g.log.committed if app else 0, k]
        want = exp["msg"] and [exp["msg"][0], None] + exp["msg"][2:]
        assert got == want, f"{where}: message {got}, want {want}"
    if "transferee" in exp:
        assert to_id(g.transferee) == exp["transferee"], f"{where}: transferee {g.transferee}"
    for key, bit in (("started", R.QFLAG_TRANSFER_STARTED), ("aborted", R.QFLAG_TRANSFER_ABORTED),
                     ("forward", R.QFLAG_FORWARD)):
        if key in exp:
            assert bool(res.qflags & bit) == exp[key], f"{where}: {key}: qflags {res.qflags:#x}"
    if exp.get("status") == "forward":
        assert res.qflags & R.QFLAG_FORWARD, f"{where}: qflags {res.qflags:#x}"
    if "election_elapsed" in exp:
        assert n.camp.election_elapsed == exp["election_elapsed"], (where, n.camp.election_elapsed)


def replay(sc, apply):
    """Run a golden scenario.  apply(node, cfg, reads, xf_from, xf_term) makes
    one call on the node (in place) and returns its Result."""
    n = build_node(sc)
    cfg = R.Config(**sc["config"])
    ids = sc["node"]["ids"]
    slot = lambda i: NO_SLOT if i == 0 else (ids.index(i) if i in ids else len(ids))  # noqa: E731
    cap = sc["node"]["inflight_cap"]
    for si, step in enumerate(sc["steps"]):
        where = f"{sc['name']} step {si}"
        if step["op"] == "set":
            g = n.group
            if "terms" in step:
                n.prop.terms = list(step["terms"])
            if "committed" in step:
                g.log.committed = step["committed"]
            if "pending" in step:
                g.pending_readindex = step["pending"]
            if "election_elapsed" in step:
                n.camp.election_elapsed = step["election_elapsed"]
            for i, p in step.get("progress", {}).items():
                g.prs[ids.index(int(i))] = _progress(p, cap)
            n.sync()
            continue
        if step["op"] == "read":
            res = apply(n, cfg, [(step["ctx"], slot(step["from"]))], NO_SLOT, 0)
        else:
            res = apply(n, cfg, [], slot(step["from"]), step["term"])
            if "msg" in step["expect"] and step["expect"]["msg"]:
                assert step["expect"]["msg"][1] == step["from"]   # To is the request's From
        check_expect(where, step["expect"], res, n, ids)
    return n


# ------------------------------------------------------------------ packing ---

def pack_nodes(nodes, readq_cap: int, cap: int = INFLIGHT_CAP):
    """(leader-step arrays, election arrays) of a batch.  Queue rows past a
    group's count hold the marker: a call must leave them alone."""
    for n in nodes:
        n.sync()
    a, e = CP.pack_nodes([n.camp for n in nodes], readq_cap, cap)
    for i, n in enumerate(nodes):
        lo, hi = i * readq_cap + len(n.queue), (i + 1) * readq_cap
        a["rq_ctx"][lo:hi] = FILL
        a["rq_index"][lo:hi] = FILL
        a["rq_meta"][lo:hi] = FILL32
    return a, e


def nodes_from_arrays(a, e, readq_cap: int, cap: int = INFLIGHT_CAP):
    """RequestNodes of a batch held as engine arrays (pack_nodes' inverse):
    ``a`` the leader-step arrays, ``e`` the election arrays."""
    G = len(a["cfg"])
    z = np.zeros(G, np.uint64)
    props = P.nodes_from_arrays(a, e, {"applied": z, "uncommitted_size": z, "pending_conf_index": z},
                                cap)
    nodes = []
    for i, prop in enumerate(props):
        meta = int(a["meta"][i])
        g = prop.group
        g.readq = []
        for k in range(min((meta >> 20) & 0x1F, readq_cap)):
            q = i * readq_cap + k
            m = int(a["rq_meta"][q])
            g.readq.append(L.ReadIndexStatus(int(a["rq_ctx"][q]), int(a["rq_index"][q]),
                                             {s for s in range(16) if (m >> s) & 1}, m >> 16))
        g.pending_readindex = bool(meta & (1 << 25))
        nodes.append(R.new_node(prop))
    return nodes


def inputs(G: int, max_reads: int, reads, xf_from=None, xf_term=None):
    """reads: per group a list of (ctx, from slot); ``n_reads`` may be given
    larger than max_reads through ``reads[g]`` being longer (the rows keep the
    first max_reads)."""
    inp = {"n_reads": np.zeros(G, np.uint8),
           "rd_ctx": np.full(max_reads * G, 0x5A5A5A5A5A5A5A5A, np.uint64),
           "rd_from": np.full(max_reads * G, 0x5A, np.uint8),
           "xf_from": np.full(G, NO_SLOT, np.uint8) if xf_from is None else np.asarray(xf_from, np.uint8),
           "xf_term": np.zeros(G, np.uint64) if xf_term is None else np.asarray(xf_term, np.uint64)}
    for g, rs in enumerate(reads):
        inp["n_reads"][g] = len(rs)
        for k, (c, f) in enumerate(rs[:max_reads]):
            inp["rd_ctx"][k * G + g] = c
            inp["rd_from"][k * G + g] = f
    return inp


def reads_of(inp, g, G, max_reads):
    """Group g's requests as request_ref.step takes them: a count past
    max_reads shows as one extra request (cut and counted there)."""
    n = int(inp["n_reads"][g])
    rs = [(int(inp["rd_ctx"][k * G + g]), int(inp["rd_from"][k * G + g]))
          for k in range(min(n, max_reads))]
    return rs + [(0, 0)] * (n > max_reads)


def new_out(G: int, S: int, max_reads: int):
    return {"rd_status": np.full(max_reads * G, FILL8, np.uint8),
            "rd_index": np.full(max_reads * G, FILL, np.uint64),
            "hb_commit": np.full(S, FILL, np.uint64), "xf_type": np.full(G, FILL8, np.uint8),
            "xf_index": np.full(G, FILL, np.uint64), "xf_log_term": np.full(G, FILL, np.uint64),
            "xf_n": np.full(G, FILL, np.uint64), "qflags": np.full(G, FILL8, np.uint8)}


def ref_requests(nodes, inp, cfg: R.Config, off, out):
    """One call through request_ref over ``nodes`` (in place).  ``off``: the
    device table's slot offsets; ``out``: new_out's dict (in place), written as
    the engine writes it.  Returns (stats of this call, Results per group)."""
    G = len(nodes)
    st = R.new_stats()
    results = []
    for i, n in enumerate(nodes):
        res = R.step(n, reads_of(inp, i, G, cfg.max_reads), int(inp["xf_from"][i]),
                     int(inp["xf_term"][i]), cfg, st)
        results.append(res)
        for k, (s, idx) in enumerate(res.reads):
            out["rd_status"][k * G + i] = s
            if idx is not None:
                out["rd_index"][k * G + i] = idx
        if res.heartbeats is not None:
            for s, c in res.heartbeats:
                if s < 16:
                    out["hb_commit"][int(off[i]) + s] = c
        t, idx, lt, k = res.xf
        out["xf_type"][i] = t
        if t in (R.MSG_APP, R.MSG_SNAP):
            out["xf_index"][i], out["xf_log_term"][i], out["xf_n"][i] = idx, lt, k
        out["qflags"][i] = res.qflags
    return st, results


# ----------------------------------------------------------------- batches ---

def random_nodes(rng: np.random.Generator, G: int, readq_cap: int, slot_counts=None,
                 cap: int = INFLIGHT_CAP):
    """P.random_nodes (learners, joint and empty configs, every role, logs of
    1..8 runs, compacted prefixes, every Progress state) with a read queue of
    0..readq_cap rows, the postponed bit, a committed index whose term is the
    leader's more often than not, a transferee now and then."""
    props = P.random_nodes(rng, G, slot_counts, cap)
    nodes = []
    for prop in props:
        g = prop.group
        if rng.random() < 0.6 and prop.terms[-1] == g.term:      # committed at the log's end
            g.log.committed = max(prop.last - int(rng.integers(0, 2)), prop.first - 1)
        nq = int(rng.choice([0, 0, 1, readq_cap - 1, readq_cap])) if readq_cap else 0
        nq = max(nq, 0)
        g.readq = [L.ReadIndexStatus(100 + k, int(rng.integers(0, g.log.committed + 1)),
                                     {s for s in range(g.n_slots) if rng.random() < 0.3},
                                     int(rng.choice([NO_SLOT, 0, g.n_slots - 1])))
                   for k in range(nq)]
        g.pending_readindex = bool(rng.random() < 0.2)
        if rng.random() < 0.15:
            g.transferee = int(rng.integers(0, g.n_slots))
        prop.camp.election_elapsed = int(rng.integers(0, 9))
        nodes.append(R.new_node(prop))
    return nodes


def random_inputs(rng: np.random.Generator, nodes, max_reads: int, p_none: float = 0.2):
    G = len(nodes)
    reads, xf_from, xf_term = [], [], []
    for n in nodes:
        g = n.group
        nr = int(rng.integers(0, max_reads + 1)) if rng.random() > p_none else 0
        if rng.random() < 0.03:
            nr = max_reads + int(rng.integers(1, 4))
        rs = []
        for _ in range(nr):
            # contexts 100.. may be pending already; a small pool repeats within the call
            c = CP._pick(rng, [0, 100, 101, 102, 103, 200, 201, 202, 203, 204, (1 << 64) - 1])
            f = int(rng.choice([NO_SLOT, NO_SLOT, 0, g.n_slots - 1, n.camp.own & 0xFF, g.n_slots,
                                0xFE]))
            rs.append((c, f))
        reads.append(rs)
        r = rng.random()
        xf_from.append(NO_SLOT if r < 0.4 else int(rng.integers(0, g.n_slots)) if r < 0.9 else
                       int(rng.choice([g.n_slots, 16, 0xFE])))
        xf_term.append(int(rng.choice([0, 0, g.term, g.term, max(g.term - 1, 0), g.term + 1])))
    return inputs(G, max_reads, reads, xf_from, xf_term)
