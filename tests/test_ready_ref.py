"""tests/ready_ref.py against the reference's own tests of the Ready cycle
(tests/golden/ready_tables.json), and tests/ready_pack.py's round trip.  No
GPU."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ready_pack as P, ready_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "ready_tables.json"), encoding="utf-8") as _f:
    TABLES = json.load(_f)
LOG = {t["name"]: t for t in TABLES["log"]}
NODE = {t["name"]: t for t in TABLES["node"]}
SEQS = TABLES["sequences"]


def make_node(d) -> R.Node:
    return R.Node(term=d["term"], vote=d["vote"], committed=d["committed"], lead=d["lead"],
                  state=d["state"], first_index=d["first"], terms=list(d["terms"]),
                  applied=d["applied"], offset=d["offset"],
                  snap=tuple(d["snap"]) if d["snap"] else None, msgs=d["msgs"],
                  read_states=d["read_states"], uncommitted_size=d["uncommitted_size"],
                  prev_soft=tuple(d["prev_soft"]), prev_hard=tuple(d["prev_hard"]))


def bare_unstable(row) -> R.Node:
    """A bare unstable{entries, offset, snapshot} as a node whose log starts at
    the offset.  Row 0's unstable{offset: 0} has no raftLog counterpart (the
    offset is a last index + 1); it is held at offset 1, and its expectation —
    nothing moves — is kept."""
    off = max(row["offset"], 1)
    return R.Node(first_index=off, terms=[0] + list(row["entries"]), offset=off,
                  committed=off - 1, applied=off - 1,
                  snap=tuple(row["snap"]) if row["snap"] else None).new_raw_node()


def apply_set(n: R.Node, fields) -> None:
    for k, v in fields.items():
        setattr(n, k, list(v) if isinstance(v, list) else v)


def table_nodes(tables):
    """Every node state the tables pass through, for the device test."""
    nodes = []
    for name in ("TestHasNextEnts", "TestNextEnts"):
        for row in tables_by(tables, "log", name)["rows"]:
            n = make_node(tables_by(tables, "log", name)["node"])
            R.applied_to(n, row["applied_to"])
            nodes.append(n)
    for row in tables_by(tables, "log", "TestUnstableEnts")["rows"]:
        nodes.append(make_node(row["node"]))
    nodes.append(make_node(tables_by(tables, "log", "TestStableTo")["node"]))
    for row in tables_by(tables, "log", "TestStableToWithSnap")["rows"]:
        nodes.append(make_node(row["node"]))
    for row in tables["unstable"]["rows"]:
        nodes.append(bare_unstable(row))
    for row in tables_by(tables, "node", "TestSoftStateEqual")["rows"]:
        nodes.append(R.Node(lead=row["soft"][0], state=row["soft"][1]))
    for row in tables_by(tables, "node", "TestIsHardStateEqual")["rows"]:
        # the log is long enough for the row's Commit to be a legal one
        nodes.append(R.Node(term=row["hard"][0], vote=row["hard"][1], committed=row["hard"][2],
                            applied=row["hard"][2], terms=[0, 0], offset=2))
    for sc in tables["sequences"]:
        n = make_node(sc["node"])
        nodes.append(copy.deepcopy(n))
        for st in sc["steps"]:
            if st["op"] == "then":
                apply_set(n, st["set"])
                nodes.append(copy.deepcopy(n))
            elif st["op"] == "ready":
                _, rd = R.ready_flags(n)
                R.accept_ready(n, rd)
                n._last = rd
            elif st["op"] == "advance":
                R.advance(n, host_record(n, n._last, st))
                nodes.append(copy.deepcopy(n))
    for n in nodes:
        n.__dict__.pop("_last", None)
    return nodes


def tables_by(tables, part, name):
    return next(t for t in tables[part] if t["name"] == name)


def host_record(n: R.Node, rd: R.Ready, step) -> R.AdvanceRecord:
    """What the host hands back of ``rd``: everything, or CommittedEntries
    only up to the step's trim_to (limitSize cut them there)."""
    cursor = step.get("trim_to", rd.committed[1] if rd.committed else rd.snap_index)
    return R.AdvanceRecord(0, rd.hard, cursor, step["payload"],
                           rd.entries[1] if rd.entries else 0, rd.entries[2] if rd.entries else 0,
                           rd.snap_index)


def test_the_table_is_what_its_maker_writes(tmp_path):
    """ready_tables.json is make_ready_golden.py's output, byte for byte."""
    src = os.path.join(ROOT, "tests", "golden", "make_ready_golden.py")
    code = open(src, encoding="utf-8").read().replace(
        "os.path.dirname(os.path.abspath(__file__))", repr(str(tmp_path)))
    subprocess.run([sys.executable, "-c", code], check=True, capture_output=True)
    with open(tmp_path / "ready_tables.json", encoding="utf-8") as f:
        assert json.load(f) == TABLES


def test_every_named_test_is_transcribed():
    names = set(LOG) | set(NODE) | {TABLES["unstable"]["name"]} | {s["name"] for s in SEQS}
    assert names == {
        "TestHasNextEnts", "TestNextEnts", "TestUnstableEnts", "TestStableTo",
        "TestStableToWithSnap", "TestUnstableStableTo", "TestReadyContainUpdates",
        "TestIsHardStateEqual", "TestSoftStateEqual", "TestRawNodeStart", "TestRawNodeRestart",
        "TestRawNodeRestartFromSnapshot", "TestRawNodeCommitPaginationAfterRestart"}
    assert len(TABLES["unstable"]["rows"]) == 11


def test_has_next_ents_and_next_ents():
    for row in LOG["TestHasNextEnts"]["rows"]:
        n = make_node(LOG["TestHasNextEnts"]["node"])
        R.applied_to(n, row["applied_to"])
        assert R.has_next_ents(n) == row["has_next"], row
        assert bool(R.ready_flags(n)[0] & R.RDF_COMMITTED) == row["has_next"], row
    for row in LOG["TestNextEnts"]["rows"]:
        n = make_node(LOG["TestNextEnts"]["node"])
        R.applied_to(n, row["applied_to"])
        want = tuple(row["want"]) if row["want"] else None
        assert R.next_ents(n) == want, row


def test_unstable_ents():
    for row in LOG["TestUnstableEnts"]["rows"]:
        n = make_node(row["node"])
        ents = R.unstable_entries(n)
        assert ents == (tuple(row["want"]) if row["want"] else None), row
        if ents:
            R.stable_to(n, ents[1], ents[2])
        assert n.offset == row["woffset"], row


def test_stable_to():
    for row in LOG["TestStableTo"]["rows"]:
        n = make_node(LOG["TestStableTo"]["node"])
        R.stable_to(n, row["index"], row["term"])
        assert n.offset == row["woffset"], row
    for row in LOG["TestStableToWithSnap"]["rows"]:
        n = make_node(row["node"])
        R.stable_to(n, row["index"], row["term"])
        assert n.offset == row["woffset"], row


def test_unstable_stable_to():
    for i, row in enumerate(TABLES["unstable"]["rows"]):
        n = bare_unstable(row)
        moved = row["woffset"] - row["offset"]
        before = n.offset
        flags = R.advance(n, R.AdvanceRecord(0, stable_index=row["index"], stable_term=row["term"]))
        assert n.offset - before == moved, (i, row)
        assert n.last_index - n.offset + 1 == row["wlen"], (i, row)
        assert bool(flags & R.AFLAG_STABLE_STALE) == (moved == 0), (i, row)


def test_ready_contain_updates_and_state_equality():
    for row in NODE["TestReadyContainUpdates"]["rows"]:
        rd = R.Ready(soft=tuple(row["soft"]) if row["soft"] else None, hard=tuple(row["hard"]),
                     entries=(1, row["entries"], 1) if row["entries"] else None,
                     committed=(1, row["committed"]) if row["committed"] else None,
                     snap_index=row["snap_index"], msgs=bool(row["msgs"]))
        assert R.contains_updates(rd) == row["want"], row
    for row in NODE["TestSoftStateEqual"]["rows"]:
        assert (tuple(row["soft"]) == (0, R.FOLLOWER)) == row["equal"]
        n = R.Node(lead=row["soft"][0], state=row["soft"][1])
        assert bool(R.ready_flags(n)[0] & R.RDF_SOFT) == (not row["equal"])
    for row in NODE["TestIsHardStateEqual"]["rows"]:
        assert R.is_empty_hard_state(tuple(row["hard"])) == row["equal"]


@pytest.mark.parametrize("sc", SEQS, ids=[s["name"] for s in SEQS])
def test_rawnode_sequences(sc):
    n = make_node(sc["node"])
    rd = None
    for i, st in enumerate(sc["steps"]):
        if st["op"] == "has_ready":
            assert R.has_ready(n) == st["want"], i
            assert bool(R.ready_flags(n)[0] & ~R.RDF_MUST_SYNC) == st["want"], i
        elif st["op"] == "then":
            apply_set(n, st["set"])
        elif st["op"] == "ready":
            f, rd = R.ready_flags(n)
            names = sorted(k for b, k in enumerate(R.RDF_NAMES) if (f >> b) & 1)
            assert names == st["flags"], i
            assert rd.soft == (tuple(st["soft"]) if st["soft"] else None), i
            assert (rd.hard if f & R.RDF_HARD else R.EMPTY_HS) == tuple(st["hard"]), i
            assert rd.entries == (tuple(st["entries"]) if st["entries"] else None), i
            assert rd.committed == (tuple(st["committed"]) if st["committed"] else None), i
            assert rd.snap_index == st["snap_index"], i
            R.accept_ready(n, rd)
        elif st["op"] == "advance":
            assert R.advance(n, host_record(n, rd, st)) == 0, i
        else:
            raise AssertionError(st["op"])


def test_pagination_keeps_committed_on_the_next_ready():
    """TestRawNodeCommitPaginationAfterRestart's point: after the host applied
    only up to its trim, the next Ready starts right behind it."""
    sc = next(s for s in SEQS if s["name"] == "TestRawNodeCommitPaginationAfterRestart")
    n = make_node(sc["node"])
    f, rd = R.ready_flags(n)
    R.accept_ready(n, rd)
    R.advance(n, host_record(n, rd, sc["steps"][1]))
    f, rd = R.ready_flags(n)
    assert f & R.RDF_COMMITTED and rd.committed == (10, 10)


def test_pack_round_trip_and_truncate_fold():
    nodes = P.seeded_nodes(200, "all", 3)
    back = P.nodes_from_arrays(P.pack_nodes(nodes))
    assert back == nodes
    # truncateAndAppend's three cases leave offset = min(offset, after)
    rng = np.random.default_rng(5)
    for n in P.seeded_nodes(200, "some", 4):
        if n.last_index < n.first_index or n.offset > n.last_index + 1 or n.committed > n.last_index:
            continue
        after = int(rng.integers(max(n.committed + 1, n.first_index), n.last_index + 2))
        m = copy.deepcopy(n)
        R.truncate_and_append(m, after, [n.last_term + 1] * 2)
        R.truncate_fold([n], [0], [after])
        assert m.offset == n.offset
        assert m.last_index == after + 1
