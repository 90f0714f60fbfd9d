"""Shared infrastructure of the propose tests: ProposeNodes from plain
arguments and from the golden scenarios, a seeded random batch, packing to the
engine's arrays (tests/campaign_pack.py for the arrays the call shares with
the campaign), and the expected outputs of one call from tests/propose_ref.py.
Test infrastructure."""
from __future__ import annotations

import json
import os

import numpy as np

from oracle import leader_ref as L
from tests import campaign_pack as CP, campaign_ref as CR, propose_ref as R
from tests.tick_ref import mark_learners

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = CP.FILL          # the outputs' pre-fill: untouched elements keep it
FILL8 = 0xA5
INFLIGHT_CAP = 2
U64 = R.U64


def load_tables():
    with open(os.path.join(ROOT, "tests", "golden", "propose_tables.json"), encoding="utf-8") as f:
        return json.load(f)


def progress(match=0, next=1, state=L.STATE_PROBE, recent_active=False, probe_sent=False,
             pending_snapshot=0, ring=(), start=0, cap=INFLIGHT_CAP) -> L.Progress:
    """A Progress whose ring holds ``ring`` (oldest first) from ``start`` on."""
    infl = L.Inflights(cap)
    infl.start = start
    for v in ring:
        infl.add(v)
    return L.Progress(match=match, next=next, state=state, pending_snapshot=pending_snapshot,
                      recent_active=recent_active, probe_sent=probe_sent, inflights=infl)


def make_node(ns, mask_in, mask_out, own, *, terms, term, first=1, role=R.LEADER, lead=0,
              committed=None, prs=None, transferee=L.NO_SLOT, cap=INFLIGHT_CAP, snap_index=None,
              snap_term=None, max_ents=1 << 62, applied=0, unc=0, pci=0, self_id=1) -> R.ProposeNode:
    """A ProposeNode of ns slots over the log ``terms`` ([first - 1 .. last]).
    Without ``prs`` every peer probes quietly at next = last + 1 and the own
    slot replicates at match = last."""
    last = first - 1 + len(terms) - 1
    if prs is None:
        prs = [progress(match=last, next=last + 1, state=L.STATE_REPLICATE, recent_active=True,
                        cap=cap) if s == own else
               progress(match=0, next=last + 1, recent_active=True, cap=cap) for s in range(ns)]
    log = L.LogView(first=first, last=last, committed=first - 1 if committed is None else committed,
                    runs=[], snap_index=first - 1 if snap_index is None else snap_index,
                    snap_term=terms[0] if snap_term is None else snap_term, max_ents=max_ents)
    g = L.LeaderGroup(ns, mask_in, mask_out, term, own, log, prs, transferee=transferee)
    mark_learners(g)
    camp = CR.CampaignNode(g, self_id, role | CR.ROLE_PROMOTABLE, 0, lead, terms[-1], 0, 0, {})
    return R.new_node(camp, terms, applied=applied, uncommitted_size=unc, pending_conf_index=pci)


def build_node(sc) -> R.ProposeNode:
    """A golden scenario's node: slot j is the j-th smallest ID."""
    nd = sc["node"]
    ids = nd["ids"]
    slot = {i: s for s, i in enumerate(ids)}
    cap = nd["inflight_cap"]
    prs = []
    for i in ids:
        p = nd["progress"][str(i)]
        prs.append(progress(p["match"], p["next"], p["state"], p["recent_active"], p["probe_sent"],
                            p.get("pending_snapshot", 0), cap=cap))
    return make_node(len(ids), sum(1 << slot[i] for i in nd["voters"]),
                     sum(1 << slot[i] for i in nd["voters_out"]), slot[nd["self"]],
                     terms=nd["terms"], term=nd["term"], first=nd["first"], role=nd["state"],
                     lead=nd["lead"], committed=nd["committed"], prs=prs,
                     transferee=slot[nd["transferee"]] if nd["transferee"] else L.NO_SLOT, cap=cap,
                     max_ents=nd["max_ents"], applied=nd["applied"], unc=nd["uncommitted_size"],
                     pci=nd["pending_conf_index"], self_id=nd["self"])


def check_expect(where, exp, pf: int, msgs, n: R.ProposeNode, ids):
    """msgs: (type, to slot, index, log_term, commit, n) of the call; n: the
    node behind it."""
    for key, bit in (("dropped", R.PFLAG_DROPPED), ("forward", R.PFLAG_FORWARD),
                     ("appended", R.PFLAG_APPENDED), ("cc_refused", R.PFLAG_CC_REFUSED)):
        if key in exp:
            assert bool(pf & bit) == exp[key], f"{where}: {key}: pflags {pf:#x}"
    if "n_msgs" in exp:
        assert len(msgs) == exp["n_msgs"], f"{where}: {len(msgs)} messages, want {exp['n_msgs']}"
    if "msgs" in exp:
        got = [[t, ids[to], i, lt, c, k] for t, to, i, lt, c, k in msgs]
        assert got == exp["msgs"], f"{where}: messages {got}, want {exp['msgs']}"
    g = n.group
    for key, got in (("last_index", n.last), ("last_term", n.terms[-1]),
                     ("committed", g.log.committed), ("pending_conf_index", n.pending_conf_index),
                     ("uncommitted_size", n.uncommitted_size)):
        if key in exp:
            assert got == exp[key], f"{where}: {key} = {got}, want {exp[key]}"
    if "log" in exp:
        got = [[t, n.first + k] for k, t in enumerate(n.terms[1:])]
        assert got == exp["log"], f"{where}: log {got}, want {exp['log']}"
    for i, want in exp.get("progress", {}).items():
        p = g.prs[ids.index(int(i))]
        got = {"match": p.match, "next": p.next, "state": p.state, "probe_sent": p.probe_sent,
               "inflights_full": p.inflights.full()}
        for key, v in want.items():
            assert got[key] == v, f"{where}: progress[{i}].{key} = {got[key]}, want {v}"


def replay(sc, apply):
    """Run a golden scenario.  apply(node, cfg, inp, k, repeat) makes the k-th
    of ``repeat`` identical calls on the node (in place) and returns (pflags,
    messages); ``inp`` is (action, n_ents, payload, cc_at, cc_payload)."""
    n = build_node(sc)
    cfg = R.Config(**sc["config"])
    ids = sc["node"]["ids"]
    for si, step in enumerate(sc["steps"]):
        where = f"{sc['name']} step {si}"
        if step["op"] == "set":
            n.uncommitted_size = step["uncommitted_size"]
            continue
        if step["op"] == "check":
            check_expect(where, step["expect"], 0, [], n, ids)
            continue
        if step["op"] == "leader_entry":
            inp = (R.PROP_LEADER_ENTRY, 0, 0, 0, 0)
        else:
            cc = step.get("cc")
            act = R.PROP_ENTRIES
            if cc:
                act |= R.PROP_CONF_CHANGE | (R.PROP_CC_LEAVE_JOINT if cc["leave_joint"] else 0)
            inp = (act, step["n"], step["payload"], cc["at"] if cc else 0,
                   cc["payload"] if cc else 0)
        repeat = step.get("repeat", 1)
        for k in range(repeat):
            pf, msgs = apply(n, cfg, inp, k, repeat)
            check_expect(f"{where} #{k}", step["expect"], pf, msgs, n, ids)
    return n


def nodes_from_arrays(a, e, p, cap: int = INFLIGHT_CAP):
    """ProposeNodes of a batch held as engine arrays (pack_nodes' inverse):
    ``a`` the leader-step arrays, ``e`` the election arrays (role, lead,
    last_term, self_id at least), ``p`` the propose arrays."""
    from tests.append_ref import terms_of_runs
    G = len(a["cfg"])
    off = a["off"]
    nodes = []
    for i in range(G):
        meta, cfg = int(a["meta"][i]), int(a["cfg"][i])
        nr = (meta >> 16) & 0xF
        starts = [int(a["run_start"][r * G + i]) for r in range(nr)]
        rterms = [int(a["run_term"][r * G + i]) for r in range(nr)]
        first = int(a["first_index"][i])
        assert starts[0] == first - 1
        prs = []
        for s in range(int(off[i]), int(off[i + 1])):
            st, pos = int(a["pstate"][s]), int(a["infl_pos"][s])
            pr = progress(int(a["match"][s]), int(a["next"][s]), st & 3, bool(st & 8), bool(st & 4),
                          int(a["pending_snapshot"][s]), cap=cap)
            pr.inflights = L.Inflights(cap, pos & 0xFFFF, pos >> 16,
                                       [int(x) for x in a["infl_buf"][s * cap:(s + 1) * cap]])
            prs.append(pr)
        n = make_node(len(prs), cfg & 0xFFFF, cfg >> 16, meta & 0xFF,
                      terms=terms_of_runs(starts, rterms, int(a["last_index"][i])),
                      term=int(a["term"][i]), first=first, lead=int(e["lead"][i]),
                      committed=int(a["committed"][i]), prs=prs, transferee=(meta >> 8) & 0xFF,
                      cap=cap, snap_index=int(a["snap_index"][i]), snap_term=int(a["snap_term"][i]),
                      max_ents=int(a["max_ents"][i]), applied=int(p["applied"][i]),
                      unc=int(p["uncommitted_size"][i]), pci=int(p["pending_conf_index"][i]),
                      self_id=int(e["self_id"][i]))
        n.camp.role = int(e["role"][i])
        assert n.camp.last_term == int(e["last_term"][i])
        for k in ("vote", "election_elapsed", "heartbeat_elapsed"):
            if k in e:
                setattr(n.camp, k, int(e[k][i]))
        if "votes" in e:
            n.camp.votes = CP.votes_dict(int(e["votes"][i]))
        nodes.append(n)
    return nodes


# ------------------------------------------------------------------ packing ---

def pack_nodes(nodes, cap: int = INFLIGHT_CAP):
    """(leader-step arrays, election arrays, propose arrays) of a batch."""
    for n in nodes:
        n.sync()
    a, e = CP.pack_nodes([n.camp for n in nodes], 0, cap)
    p = {"applied": np.array([n.applied for n in nodes], np.uint64),
         "uncommitted_size": np.array([n.uncommitted_size for n in nodes], np.uint64),
         "pending_conf_index": np.array([n.pending_conf_index for n in nodes], np.uint64)}
    return a, e, p


@np.errstate(over="ignore")
def inputs(action, n_ents, payload=None, cc_at=None, cc_payload=None):
    G = len(action)
    z = lambda dt: np.zeros(G, dt)  # noqa: E731
    return {"action": np.asarray(action, np.uint8), "n_ents": np.asarray(n_ents, np.uint32),
            "payload": z(np.uint64) if payload is None else np.asarray(payload, np.uint64),
            "cc_at": z(np.uint32) if cc_at is None else np.asarray(cc_at, np.uint32),
            "cc_payload": z(np.uint64) if cc_payload is None else np.asarray(cc_payload, np.uint64)}


def ref_propose(nodes, inp, cfg: R.Config, off, msg):
    """One call through propose_ref over ``nodes`` (in place).  ``off``: the
    device table's slot offsets; ``msg``: dict of msg_type / msg_index /
    msg_log_term / msg_n (numpy, in place), written as the engine writes
    them.  Returns (pflags, stats of this call, messages per group)."""
    G = len(nodes)
    pflags = np.zeros(G, np.uint8)
    st = R.new_stats()
    sent = []
    for i, n in enumerate(nodes):
        pf, msgs = R.step(n, int(inp["action"][i]), int(inp["n_ents"][i]), int(inp["payload"][i]),
                          int(inp["cc_at"][i]), int(inp["cc_payload"][i]), cfg, st)
        pflags[i] = pf
        sent.append(msgs)
        assert bool(msgs) <= bool(pf & R.PFLAG_BCAST)
        if pf & R.PFLAG_BCAST:
            s0 = int(off[i])
            msg["msg_type"][s0:s0 + n.group.n_slots] = 0
            for t, to, idx, lt, _, k in msgs:
                msg["msg_type"][s0 + to] = t
                msg["msg_index"][s0 + to] = idx
                msg["msg_log_term"][s0 + to] = lt
                msg["msg_n"][s0 + to] = k
    return pflags, st, sent


def new_msg(S: int):
    return {"msg_type": np.full(S, FILL8, np.uint8), "msg_index": np.full(S, FILL, np.uint64),
            "msg_log_term": np.full(S, FILL, np.uint64), "msg_n": np.full(S, FILL, np.uint64)}


# ----------------------------------------------------------------- batches ---

def random_terms(rng, term, max_len=30):
    """A log's terms, non-decreasing, ending at or below ``term``, in at most
    MAX_RUNS runs (sometimes exactly that many)."""
    n = int(rng.integers(1, max_len + 1))            # entries incl. the dummy
    last_t = term if rng.random() < 0.7 else max(1, term - int(rng.integers(1, 3)))
    k = min(int(rng.choice([1, 1, 2, 3, 7, 8])), n, last_t)
    ts = sorted(int(x) for x in rng.choice(np.arange(1, last_t), k - 1, replace=False)) + [last_t]
    cuts = sorted(int(x) for x in rng.choice(np.arange(1, n), k - 1, replace=False)) if k > 1 else []
    bounds = [0] + cuts + [n]
    out = []
    for r in range(k):
        out += [ts[r]] * (bounds[r + 1] - bounds[r])
    return out


def random_nodes(rng: np.random.Generator, G: int, slot_counts=None, cap: int = INFLIGHT_CAP):
    """Seeded ragged batch: learners, joint and empty configs, every role, the
    own slot a voter / beyond the slots, logs of 1..8 term runs with the
    leader's term on top or not yet, compacted prefixes, Progress in every
    state with rings empty / part / full / wrapped, peers behind first_index
    with and without RecentActive or a snapshot, a transferee now and then,
    and the proposal words around their thresholds."""
    nodes = []
    for _ in range(G):
        ns = int(rng.choice(slot_counts)) if slot_counts else int(rng.integers(1, 17))
        vin, vout = CP.random_config(rng, ns)
        own = int(rng.integers(0, ns))
        r = rng.random()
        if r < 0.06:
            own = int(rng.choice([ns, 16, 0xFE, 0xFF]))
        elif r < 0.8:
            own = next((s for s in range(own, ns) if ((vin | vout) >> s) & 1), own)
        if rng.random() < 0.1:
            vin, vout = 1 << min(own, ns - 1), 0        # single voter: commits at once
        term = int(rng.integers(1, 12))
        terms = random_terms(rng, term)
        first = int(rng.integers(1, 40))
        last = first - 1 + len(terms) - 1
        committed = int(rng.integers(first - 1, last + 1))
        prs = []
        for s in range(ns):
            state = int(rng.choice([0, 0, 1, 1, 1, 2]))
            match = int(rng.integers(0, last + 1))
            nxt = match + 1 + int(rng.integers(0, 3))
            if rng.random() < 0.25:
                nxt = int(rng.integers(max(1, first - 3), last + 3))
            ring, start = (), 0
            if state == L.STATE_REPLICATE:
                cnt = int(rng.integers(0, cap + 1))
                start = int(rng.integers(0, cap))
                ring = tuple(match + 1 + q for q in range(cnt))
            if s == own and rng.random() < 0.8:
                state, match, nxt, ring = L.STATE_REPLICATE, last, last + 1, ()
            prs.append(progress(match, nxt, state, bool(rng.random() < 0.6),
                                bool(rng.random() < 0.3),
                                int(rng.integers(0, last + 3)) if state == 2 else 0, ring, start, cap))
        role = int(rng.choice([R.LEADER] * 7 + [R.FOLLOWER, R.CANDIDATE, R.PRE_CANDIDATE]))
        applied = int(rng.integers(0, committed + 1))
        nodes.append(make_node(
            ns, vin, vout, own, terms=terms, term=term, first=first, role=role,
            lead=int(rng.choice([0, 3])), committed=committed, prs=prs,
            transferee=int(rng.integers(0, ns)) if rng.random() < 0.05 else L.NO_SLOT, cap=cap,
            snap_index=0 if rng.random() < 0.2 else first - 1, snap_term=terms[0],
            max_ents=int(rng.choice([1, 2, 5, 1 << 62])), applied=applied,
            unc=int(rng.choice([0, 0, 10, 90, 100, 101])),
            pci=int(rng.choice([0, applied, applied + 1, max(applied - 1, 0)])),
            self_id=int(rng.integers(1, 1 << 62))))
    return nodes


def random_inputs(rng: np.random.Generator, G: int, p_none: float = 0.15, p_bad: float = 0.03):
    action = rng.choice([R.PROP_ENTRIES] * 8 + [R.PROP_LEADER_ENTRY], G).astype(np.uint8)
    cc = rng.random(G) < 0.25
    action[cc] |= R.PROP_CONF_CHANGE
    action[cc & (rng.random(G) < 0.4)] |= R.PROP_CC_LEAVE_JOINT
    action[rng.random(G) < p_none] = R.PROP_NONE
    bad = rng.random(G) < p_bad
    action[bad] = rng.choice([3, 5, 0x3F, 0x43, 0xFF], int(bad.sum())).astype(np.uint8)
    n_ents = rng.integers(1, 6, G).astype(np.uint32)
    n_ents[rng.random(G) < 0.03] = 0
    cc_payload = rng.integers(0, 8, G).astype(np.uint64)
    payload = cc_payload + rng.choice([0, 0, 1, 5, 10, 11, 200], G).astype(np.uint64)
    cc_at = rng.integers(0, 6, G).astype(np.uint32)     # (sometimes >= n_ents: the bit reads clear)
    return inputs(action, n_ents, payload, cc_at, cc_payload)
