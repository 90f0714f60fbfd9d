"""Shared infrastructure of the follower-step tests: the golden scenarios as
follower_ref Nodes / Recs, packing to the engine's arrays, a seeded fuzz
generator, and the expected arrays of one call from tests/follower_ref.py.
Test infrastructure."""
from __future__ import annotations

import copy
import json
import os

import numpy as np

from tests import follower_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64_FIELDS = ("term", "vote", "lead", "committed", "last_index", "last_term")
GROUP_DTYPES = dict({k: np.uint64 for k in U64_FIELDS}, role=np.uint8,
                    election_elapsed=np.uint32, heartbeat_elapsed=np.uint32)
INBOX_DTYPES = {"group": np.uint32, "flags": np.uint8, "from": np.uint64, "term": np.uint64,
                "index": np.uint64, "aux": np.uint64}
FUZZ_SEEDS = (1, 2, 3)
FUZZ_G, FUZZ_M = 1000, 5000


def load_tables():
    with open(os.path.join(ROOT, "tests", "golden", "follower_tables.json"), encoding="utf-8") as f:
        return json.load(f)


def scenario_node(sc) -> F.Node:
    return F.Node(**sc["node"])


def scenario_recs(sc):
    return [F.Rec(r["kind"], r["from"], r["term"], r["index"], r["aux"], r["force"])
            for r in sc["recs"]]


def scenario_config(sc) -> F.Config:
    return F.Config(**sc["config"])


def check_scenario(sc, resp_type, resp_term, node: F.Node):
    """The scenario's expectations against one run's responses (per record)
    and the node after it."""
    where = sc["name"]
    for j, r in enumerate(sc["recs"]):
        exp = r["expect"]
        assert resp_type[j] & 0x7F == exp["type"], f"{where}#{j}: type {resp_type[j]}, want {exp}"
        assert bool(resp_type[j] & F.REJECT) == exp["reject"], f"{where}#{j}: reject, want {exp}"
        if "term" in exp:
            assert resp_term[j] == exp["term"], f"{where}#{j}: term {resp_term[j]}, want {exp}"
    for k, v in sc["expect_node"].items():
        got = node.state if k == "state" else getattr(node, k)
        assert got == v, f"{where}: {k} = {got}, want {v}"


def pack_nodes(nodes):
    return {k: np.array([getattr(n, k) for n in nodes], dt) for k, dt in GROUP_DTYPES.items()}


def pack_recs(recs):
    """recs: (group, Rec) in arrival order."""
    return {"group": np.array([g & 0xFFFFFFFF for g, _ in recs], np.uint32),
            "flags": np.array([m.kind | (F.FORCE if m.force else 0) for _, m in recs], np.uint8),
            "from": np.array([m.frm for _, m in recs], np.uint64),
            "term": np.array([m.term for _, m in recs], np.uint64),
            "index": np.array([m.index for _, m in recs], np.uint64),
            "aux": np.array([m.aux for _, m in recs], np.uint64)}


def expected(nodes, recs, cfg: F.Config):
    """follower_ref over a copy of ``nodes``: (group arrays after, outputs)
    with outputs = resp_type u8 / resp_term u64 [M], stop_at u32 / gflags u8
    [G], stats dict."""
    after = copy.deepcopy(nodes)
    rt, rterm, stop, gf, st = F.step_batch(after, recs, cfg)
    return pack_nodes(after), {"resp_type": np.array(rt, np.uint8),
                               "resp_term": np.array(rterm, np.uint64),
                               "stop_at": np.array(stop, np.uint32),
                               "gflags": np.array(gf, np.uint8), "stats": st}


def interleave(per_group, rng: np.random.Generator):
    """Lists of Recs per group -> one batch in which every group's records
    keep their order and the groups are interleaved at random."""
    owner = np.repeat(np.arange(len(per_group)), [len(r) for r in per_group])
    rng.shuffle(owner)
    nxt = [0] * len(per_group)
    out = []
    for g in owner.tolist():
        out.append((g, per_group[g][nxt[g]]))
        nxt[g] += 1
    return out


# every seed runs under both settings of check_quorum and of pre_vote
FUZZ_CONFIGS = ((True, False), (False, True), (True, True), (False, False))
FUZZ_ET = 10


def fuzz_config(check_quorum: bool, pre_vote: bool) -> F.Config:
    return F.Config(election_timeout=FUZZ_ET, check_quorum=check_quorum, pre_vote=pre_vote)


def fuzz(seed: int, G: int = FUZZ_G, M: int = FUZZ_M):
    """(nodes, recs): all four roles with a random promotable bit, terms
    3..6, a known leader or none, electionElapsed inside and outside the lease
    window; records of every kind with terms below / at / above the node's
    and 0, FORCE, Commit inside and past lastIndex, logs behind / equal /
    ahead of the voter's, HOST records, bad groups and bad kinds."""
    rng = np.random.default_rng(seed)
    et = FUZZ_ET
    nodes = []
    for _ in range(G):
        term = int(rng.integers(3, 7))
        last_term = int(rng.integers(1, term + 1))
        last_index = int(rng.integers(0, 50))
        role = int(rng.choice([F.FOLLOWER, F.FOLLOWER, F.FOLLOWER, F.CANDIDATE, F.LEADER,
                               F.PRE_CANDIDATE]))
        if rng.random() < 0.7:
            role |= F.ROLE_PROMOTABLE
        nodes.append(F.Node(term=term, vote=int(rng.choice([0, 0, 1, 2, 3])),
                            lead=int(rng.choice([0, 1, 2, 3])),
                            committed=int(rng.integers(0, last_index + 1)),
                            last_index=last_index, last_term=last_term, role=role,
                            election_elapsed=int(rng.choice([0, et - 1, et, et + 3])),
                            heartbeat_elapsed=int(rng.integers(0, 4))))
    recs = []
    for _ in range(M):
        g = int(rng.integers(0, G))
        r = rng.random()
        if r < 0.01:
            g = int(rng.choice([G, G + 7, 0xFFFFFFFF]))
        n = nodes[g] if g < G else nodes[0]
        kind = int(rng.choice([F.HEARTBEAT] * 8 + [F.VOTE] * 4 + [F.PREVOTE] * 4 +
                              [F.TIMEOUT_NOW] * 2 + [F.HOST] + ([int(rng.integers(5, 8))] if rng.random() < 0.2 else [])))
        term = int(rng.choice([0, max(n.term - 1, 1), n.term, n.term, n.term, n.term + 1,
                               n.term + 2, int(rng.integers(1, 9))]))
        frm = int(rng.integers(1, 4))
        if kind == F.HEARTBEAT:
            index = int(rng.integers(0, n.last_index + 1))
            if rng.random() < 0.04:
                index = n.last_index + int(rng.integers(1, 5))
            aux = int(rng.choice([0, int(rng.integers(1, 1 << 62))]))
        else:
            index = max(0, n.last_index + int(rng.integers(-2, 3)))
            aux = max(0, n.last_term + int(rng.integers(-1, 2)))
        recs.append((g, F.Rec(kind, frm, term, index, aux, bool(rng.random() < 0.25))))
    return nodes, recs
