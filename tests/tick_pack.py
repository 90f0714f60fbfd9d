"""Shared infrastructure of the tick tests: the golden scenarios as TickNodes,
a seeded random batch, packing to the engine's arrays (tests/leader_pack.py
for the arrays the tick shares with the leader step), the expected outputs of
one tick from tests/tick_ref.py, and a numpy-vectorised restatement of the
tick for sizes a Python loop cannot cover (checked against tick_ref in
tests/test_tick_ref.py).  Test infrastructure."""
from __future__ import annotations

import json
import os

import numpy as np

from oracle import leader_ref as L
from tests import leader_pack, tick_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5A5A5A5A5A5A5A5  # the outputs' pre-fill: untouched elements keep it
TIMEOUTS = ((10, 1, 1), (10, 1, 0), (3, 3, 1), (1, 1, 1), (5, 7, 1))


def load_tables():
    with open(os.path.join(ROOT, "tests", "golden", "tick_tables.json"), encoding="utf-8") as f:
        return json.load(f)


def make_group(ns, mask_in, mask_out, leader, committed, match, active, transferee=L.NO_SLOT,
               readq_ctx=()) -> L.LeaderGroup:
    """A LeaderGroup holding what the tick reads; the rest is a valid,
    inert leader state (one term run, Replicate, an empty one-entry ring)."""
    last = max([committed] + list(match) + [1])
    log = L.LogView(first=1, last=last, committed=committed, runs=[(0, 1)])
    prs = [L.Progress(match=m, next=(m + 1) & L.M64, state=L.STATE_REPLICATE, recent_active=bool(a),
                      inflights=L.Inflights(1)) for m, a in zip(match, active)]
    readq = [L.ReadIndexStatus(c, committed, set(), L.NO_SLOT) for c in readq_ctx]
    g = L.LeaderGroup(ns, mask_in, mask_out, 1, leader, log, prs, transferee=transferee, readq=readq)
    T.mark_learners(g)
    return g


def build_node(sc) -> T.TickNode:
    g = make_group(sc["slots"], sc["mask_in"], sc["mask_out"], sc["leader"], sc["committed"],
                   [p["match"] for p in sc["progress"]],
                   [p["recent_active"] for p in sc["progress"]], sc["transferee"], sc["readq_ctx"])
    return T.TickNode(g, sc["role"], sc["election_elapsed"], sc["heartbeat_elapsed"],
                      sc["rand_timeout"])


def check_tick_expect(where, exp, msgs, node: T.TickNode):
    """msgs: dicts with leader_scenarios.MSG_FIELDS; node: the state after."""
    from tests.leader_scenarios import MSG_FIELDS
    if "n_msgs" in exp:
        assert len(msgs) == exp["n_msgs"], f"{where}: {len(msgs)} msgs, want {exp['n_msgs']}: {msgs}"
    if "msgs_exact" in exp:
        got = [[m[k] for k in MSG_FIELDS] for m in msgs]
        assert got == exp["msgs_exact"], f"{where}: msgs {got}, want {exp['msgs_exact']}"
    for k, v in exp.get("all_msgs", {}).items():
        for j, m in enumerate(msgs):
            assert m[k] == v, f"{where}: msg {j} {k}={m[k]}, want {v}"
    if "role" in exp:
        assert node.role & 3 == exp["role"], f"{where}: role {node.role & 3}, want {exp['role']}"
    if "transferee" in exp:
        assert node.group.transferee == exp["transferee"], f"{where}: {node.group.transferee}"


def random_nodes(rng: np.random.Generator, G: int, readq_cap: int, et: int, ht: int):
    """Seeded ragged batch: 1..16 slots, learners, joint configs with either
    half empty, the leader at a random voter slot or without a Progress, mixed
    roles with a random promotable bit, read queues of 0..readq_cap, and
    counters at timeout-1 / timeout / timeout+5 / anywhere below."""
    def start(timeout):
        return int(rng.choice([max(timeout - 1, 0), timeout, timeout + 5,
                               int(rng.integers(0, timeout + 1))]))
    nodes = []
    for _ in range(G):
        ns = int(rng.integers(1, 17))
        bits = [int(x) for x in rng.random(ns) < 0.7]
        vin = sum(b << s for s, b in enumerate(bits))
        vout = 0
        r = rng.random()
        if r < 0.25:    # joint, both halves
            vout = sum(int(x) << s for s, x in enumerate(rng.random(ns) < 0.5))
        elif r < 0.35:  # joint with an empty incoming half
            vout, vin = vin, 0
        elif r < 0.40:  # nobody votes at all
            vin = 0
        leader = int(rng.integers(0, ns))
        r = rng.random()
        if r < 0.10:
            leader = int(rng.choice([ns, 16, 0xFE]))  # the leader has no Progress
        elif r < 0.80:
            leader = next((s for s in range(leader, ns) if ((vin | vout) >> s) & 1), leader)
        committed = int(rng.integers(0, 1000))
        match = [int(rng.choice([0, committed, int(rng.integers(0, 2000))])) for _ in range(ns)]
        if rng.random() < 0.02:
            match[0], committed = (1 << 64) - 1, (1 << 64) - 2   # full-range compare
        active = rng.random(ns) < 0.5
        transferee = int(rng.integers(0, ns)) if rng.random() < 0.3 else L.NO_SLOT
        nq = int(rng.integers(0, readq_cap + 1))
        ctx = [int(rng.integers(1, 1 << 62)) for _ in range(nq)]
        g = make_group(ns, vin, vout, leader, committed, match, active, transferee, ctx)
        role = int(rng.choice([T.LEADER, T.LEADER, T.LEADER, T.FOLLOWER, T.CANDIDATE,
                               T.PRE_CANDIDATE]))
        if rng.random() < 0.6:
            role |= T.ROLE_PROMOTABLE
        rt = et + int(rng.integers(0, et))
        leader_role = (role & 3) == T.LEADER
        nodes.append(T.TickNode(g, role, start(et if leader_role else rt), start(ht), rt))
    return nodes


def pack_nodes(nodes, readq_cap: int):
    """(leader-step arrays, tick arrays) of a batch."""
    arrays = leader_pack.pack([n.group for n in nodes], 1, readq_cap)
    tick = {"role": np.array([n.role for n in nodes], np.uint8),
            "election_elapsed": np.array([n.election_elapsed for n in nodes], np.uint32),
            "heartbeat_elapsed": np.array([n.heartbeat_elapsed for n in nodes], np.uint32),
            "rand_timeout": np.array([n.rand_timeout for n in nodes], np.uint32)}
    return arrays, tick


def ref_tick(nodes, off, et, ht, cq, hb_commit, hb_ctx):
    """One tick of every node through tick_ref; applies the heartbeats to the
    slot-aligned hb_commit / hb_ctx arrays (in place) and returns (tflags,
    stats of this tick)."""
    roles = [n.role for n in nodes]
    tflags = np.zeros(len(nodes), np.uint8)
    n_msgs = 0
    for i, n in enumerate(nodes):
        n.msgs = []
        tflags[i] = T.tick(n, et, ht, bool(cq))
        if tflags[i] & T.TFLAG_BEAT:
            hb_ctx[i] = n.group.readq[-1].ctx if n.group.readq else 0
        for m in n.msgs:
            assert m.type == T.MSG_HEARTBEAT and m.index == 0 and m.log_term == 0
            hb_commit[int(off[i]) + m.to] = m.commit
            assert m.aux == hb_ctx[i]
        n_msgs += len(n.msgs)
    return tflags, T.stats_of(tflags.tolist(), roles, n_msgs)


def set_recent_active(nodes, off, mask):
    """RecentActive := true where mask (per slot), on the reference side."""
    for i, n in enumerate(nodes):
        for s, p in enumerate(n.group.prs):
            if mask[int(off[i]) + s]:
                p.recent_active = True


# ------------------------------------------------- vectorised restatement ---

def np_tick(a, t, readq_cap, et, ht, cq, hb_commit, hb_ctx):
    """tick_ref over arrays, for tables of one slot count per group or ragged
    ones (numpy; in place on a["meta"], a["pstate"], t[...], hb_commit,
    hb_ctx).  Returns (tflags, stats).  The same rules as tick_ref.tick, one
    array operation per branch."""
    off = a["off"].astype(np.int64)
    G = len(a["cfg"])
    ns = np.minimum(off[1:] - off[:-1], 16)
    S = int(off[-1])
    grp = np.repeat(np.arange(G), off[1:] - off[:-1])
    k = np.arange(S) - off[grp]                      # slot within its group
    inslot = k < 16
    role = t["role"]
    leader = (role & 3) == T.LEADER
    tf = np.zeros(G, np.uint8)
    ee = t["election_elapsed"] + np.uint32(1)
    he = np.where(leader, t["heartbeat_elapsed"] + np.uint32(1), t["heartbeat_elapsed"])
    hup = ~leader & ((role & T.ROLE_PROMOTABLE) != 0) & (ee >= t["rand_timeout"])
    ee[hup] = 0
    tf[hup] |= T.TFLAG_HUP
    sweep = leader & (ee >= et)
    ee[sweep] = 0
    meta = a["meta"]
    ls = (meta & 0xFF).astype(np.int64)
    has_pr = ls < ns
    own = inslot & has_pr[grp] & (k == ls[grp])
    down = np.zeros(G, bool)
    if cq and sweep.any():
        tf[sweep] |= T.TFLAG_CHECK_QUORUM
        sel = (((a["pstate"] & 8) != 0) | own) & inslot & sweep[grp]
        bits = np.bincount(grp[sel], weights=(1 << k[sel]).astype(np.float64),
                           minlength=G).astype(np.int64)   # (sums < 2^16: exact)
        cfg = a["cfg"].astype(np.int64)

        def won(mask):
            n, y = _popc(mask), _popc(mask & bits)
            return (n == 0) | (y >= n // 2 + 1)
        down = sweep & ~(won(cfg & 0xFFFF) & won(cfg >> 16))
        clear = sweep[grp] & inslot
        st = a["pstate"]
        st[clear & ~own] &= np.uint8(0xF7)
        st[clear & own & ~down[grp]] |= np.uint8(8)
        st[clear & own & down[grp]] &= np.uint8(0xF7)
        tf[down] |= T.TFLAG_STEPPED_DOWN
        role[down] &= np.uint8(0xFC)
        he[down] = 0
        meta[down] |= np.uint32(0xFF00)
    abort = sweep & ~down & ((meta & 0xFF00) != 0xFF00)
    meta[abort] |= np.uint32(0xFF00)
    tf[abort] |= T.TFLAG_TRANSFER_ABORTED
    beat = leader & ~down & (he >= ht)
    he[beat] = 0
    tf[beat] |= T.TFLAG_BEAT
    nq = np.minimum((meta >> 20) & 0x1F, readq_cap).astype(np.int64)
    ctx = np.zeros(G, np.uint64)
    hasq = beat & (nq > 0)
    if readq_cap:
        ctx[hasq] = a["rq_ctx"][np.arange(G)[hasq] * readq_cap + nq[hasq] - 1]
    hb_ctx[beat] = ctx[beat]
    send = beat[grp] & inslot & ~own
    hb_commit[send] = np.minimum(a["match"][send], a["committed"][grp][send])
    t["election_elapsed"][:] = ee
    t["heartbeat_elapsed"][:] = he
    nl = int(leader.sum())
    stats = {"leaders": nl, "non_leaders": G - nl, "beats": int(beat.sum()),
             "heartbeats": int(send.sum()), "check_quorum": int(sweep.sum()) if cq else 0,
             "stepped_down": int(down.sum()), "transfer_aborted": int(abort.sum()),
             "hups": int(hup.sum())}
    return tf, stats


def _popc(x):
    x = x.astype(np.uint64)
    c = np.zeros(len(x), np.int64)
    for b in range(16):
        c += ((x >> np.uint64(b)) & np.uint64(1)).astype(np.int64)
    return c
