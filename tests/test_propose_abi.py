"""qb_dev_leader_propose's host-side argument checks: every refusal by return
code and error text, with no GPU (the checks run before any HIP call), and
the binding's structs against the header's layout."""
import ctypes as C
import os
import subprocess

import pytest

from etcd_amd import _lib
from etcd_amd.quorum import propose as qp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 0x1000  # a non-NULL pointer; never dereferenced: each check fails first
PTRS = ("off", "cfg", "role", "term", "lead", "first_index", "snap_index", "snap_term",
        "max_ents", "applied", "meta", "committed", "last_index", "last_term", "run_start",
        "run_term", "uncommitted_size", "pending_conf_index", "match", "next",
        "pending_snapshot", "pstate", "infl_pos", "infl_buf")
INS = ("action", "n_ents", "payload", "cc_at", "cc_payload")
OUTS = ("pflags", "msg_type", "msg_index", "msg_log_term", "msg_n")


def groups(**kw):
    f = dict(G=16, inflight_cap=4, disable_proposal_forwarding=0, max_uncommitted_size=0)
    f.update({p: D for p in PTRS})
    f.update(kw)
    return qp.ProposeGroupsC(**f)


def call(pg, pin="default", pout="default", stats=D, **kw):
    lib = _lib.load()
    if pin == "default":
        pin = qp.ProposeInC(**{k: kw.get(k, D) for k in INS})
    if pout == "default":
        pout = qp.ProposeOutC(**{k: kw.get(k, D) for k in OUTS})
    ref = lambda s: C.byref(s) if s is not None else None  # noqa: E731
    rc = lib.qb_dev_leader_propose(ref(pg), ref(pin), ref(pout), stats, None)
    return rc, lib.qb_last_error()


def test_the_mirrors_list_the_header_pointers():
    assert tuple(n for n, _ in qp.ProposeGroupsC._fields_[4:]) == PTRS
    assert tuple(n for n, _ in qp.ProposeInC._fields_) == INS
    assert tuple(n for n, _ in qp.ProposeOutC._fields_) == OUTS


def test_null_structs_are_einval():
    rc, err = call(None)
    assert rc == _lib.QB_EINVAL and b"pg is NULL" in err
    rc, err = call(groups(), pin=None)
    assert rc == _lib.QB_EINVAL and b"in / out is NULL" in err
    rc, err = call(groups(), pout=None)
    assert rc == _lib.QB_EINVAL and b"in / out is NULL" in err


@pytest.mark.parametrize("name", PTRS)
def test_null_group_pointer_is_einval(name):
    rc, err = call(groups(**{name: None}))
    assert rc == _lib.QB_EINVAL and b"group pointer is NULL" in err


@pytest.mark.parametrize("name", INS)
def test_null_input_pointer_is_einval(name):
    rc, err = call(groups(), **{name: None})
    assert rc == _lib.QB_EINVAL and b"input pointer is NULL" in err


@pytest.mark.parametrize("name", OUTS)
def test_null_output_pointer_is_einval(name):
    rc, err = call(groups(), **{name: None})
    assert rc == _lib.QB_EINVAL and b"output pointer is NULL" in err


def test_null_stats_is_einval():
    rc, err = call(groups(), stats=None)
    assert rc == _lib.QB_EINVAL and b"output pointer is NULL" in err


@pytest.mark.parametrize("cap", [0, 4097, 0xFFFFFFFF])
def test_inflight_cap_range(cap):
    rc, err = call(groups(inflight_cap=cap))
    assert rc == _lib.QB_EINVAL and b"inflight_cap must be 1..4096" in err


def test_disable_proposal_forwarding_is_a_flag():
    rc, err = call(groups(disable_proposal_forwarding=2))
    assert rc == _lib.QB_EINVAL and b"disable_proposal_forwarding must be 0 or 1" in err


def test_no_groups_is_ok_and_touches_nothing():
    """G == 0 returns QB_OK before any array pointer is looked at."""
    pg = groups(G=0, **{p: None for p in PTRS})
    rc, _ = call(pg, stats=None, **{k: None for k in INS + OUTS})
    assert rc == _lib.QB_OK


def test_python_mirror_refuses_host_tensors():
    import importlib

    import torch
    from etcd_amd.quorum import follower as qf, tick as qt
    qc = importlib.import_module("etcd_amd.quorum.campaign")
    z8 = torch.zeros(64, dtype=torch.uint8)
    z32, z64 = torch.zeros(64, dtype=torch.int32), torch.zeros(64, dtype=torch.int64)
    st = qt.TickState(z8, z32, z32, z32)
    fg = qf.FollowerGroups(4, 10, False, True, {k: z64 for k in (
        "term", "vote", "lead", "committed", "last_index", "last_term")}, st)
    es = qc.ElectionState(z64, z32, fg)

    class FakeGroups:
        G, S, device, inflight_cap = 4, 4, torch.device("cpu"), 2
        t = {k: z64 for k in ("first_index", "snap_index", "snap_term", "max_ents", "run_start",
                              "run_term", "match", "next", "pending_snapshot", "infl_buf", "term",
                              "committed", "last_index")}
        t.update(off=z32, cfg=z32, meta=z32, infl_pos=z32, pstate=z8)
    with pytest.raises(_lib.QuorumBatchError, match="device tensor"):
        qp.leader_propose(FakeGroups, es, qp.ProposeState(z64, z64, z64),
                          qp.ProposeInbox(z8, z32, z64, z32, z64))
    FakeGroups.inflight_cap = 0
    with pytest.raises(_lib.QuorumBatchError, match="inflight_cap"):
        qp.leader_propose(FakeGroups, es, qp.ProposeState(z64, z64, z64),
                          qp.ProposeInbox(z8, z32, z64, z32, z64))


def test_binding_layout_and_constants_match_header(tmp_path):
    """The three mirrors have the header's sizes and field offsets, and the
    module's constants the header's values (gcc on the header)."""
    structs = (("qb_propose_groups", qp.ProposeGroupsC),
               ("qb_propose_in", qp.ProposeInC), ("qb_propose_out", qp.ProposeOutC))
    consts = [("QB_PROP_NONE", qp.PROP_NONE), ("QB_PROP_ENTRIES", qp.PROP_ENTRIES),
              ("QB_PROP_LEADER_ENTRY", qp.PROP_LEADER_ENTRY),
              ("QB_PROP_CONF_CHANGE", qp.PROP_CONF_CHANGE),
              ("QB_PROP_CC_LEAVE_JOINT", qp.PROP_CC_LEAVE_JOINT),
              ("QB_MSG_APP", qp.MSG_APP), ("QB_MSG_SNAP", qp.MSG_SNAP),
              ("QB_PFLAG_APPENDED", qp.PFLAG_APPENDED), ("QB_PFLAG_BCAST", qp.PFLAG_BCAST),
              ("QB_PFLAG_COMMITTED", qp.PFLAG_COMMITTED), ("QB_PFLAG_DROPPED", qp.PFLAG_DROPPED),
              ("QB_PFLAG_FORWARD", qp.PFLAG_FORWARD), ("QB_PFLAG_CC_REFUSED", qp.PFLAG_CC_REFUSED),
              ("QB_PFLAG_LOG_RUNS", qp.PFLAG_LOG_RUNS), ("QB_PFLAG_BAD", qp.PFLAG_BAD),
              ("QB_PSTAT_COUNT", len(qp.PSTAT_NAMES)), ("QB_ABI_VERSION", 1)]
    consts += [("QB_PSTAT_" + c, qp.PSTAT_NAMES.index(n)) for c, n in (
        ("PROPOSALS", "proposals"), ("ENTRIES", "entries"),
        ("DROP_NO_PROGRESS", "drop_no_progress"), ("DROP_TRANSFER", "drop_transfer"),
        ("DROP_SIZE", "drop_size"), ("DROP_NO_LEADER", "drop_no_leader"),
        ("DROP_FORWARDING", "drop_forwarding"), ("DROP_CANDIDATE", "drop_candidate"),
        ("FORWARDED", "forwarded"), ("CC_ACCEPTED", "cc_accepted"), ("CC_REFUSED", "cc_refused"),
        ("MSG_APP", "msg_app"), ("MSG_SNAP", "msg_snap"), ("COMMITS", "commits"),
        ("LEADER_ENTRIES", "leader_entries"), ("LOG_RUNS", "log_runs"), ("EMPTY", "empty"),
        ("IGNORED_ROLE", "ignored_role"), ("BAD_ACTION", "bad_action"))]
    items = []
    want = []
    for cname, cls in structs:
        items.append(f"sizeof({cname})")
        want.append(C.sizeof(cls))
        for n, _ in cls._fields_:
            items.append(f"offsetof({cname}, {n})")
            want.append(getattr(cls, n).offset)
    fmt = " ".join(["%zu"] * len(items) + ["%d"] * len(consts))
    args = ", ".join(items + [f"(int)({c})" for c, _ in consts])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quorum_batch.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", {args}); return 0; }}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert got == want + [v for _, v in consts]
