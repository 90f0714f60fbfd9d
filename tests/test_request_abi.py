"""qb_dev_leader_requests' host-side argument checks: every refusal by return
code and error text, with no GPU (the checks run before any HIP call), and
the binding's structs against the header's layout."""
import ctypes as C
import os
import subprocess

import pytest

from etcd_amd import _lib
from etcd_amd.quorum import request as qr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 0x1000  # a non-NULL pointer; never dereferenced: each check fails first
PTRS = ("off", "cfg", "meta", "role", "term", "lead", "committed", "first_index", "last_index",
        "last_term", "snap_index", "snap_term", "max_ents", "run_start", "run_term",
        "election_elapsed", "match", "next", "pending_snapshot", "pstate", "infl_pos", "infl_buf")
QUEUE = ("rq_ctx", "rq_index", "rq_meta")
INS = ("n_reads", "rd_ctx", "rd_from", "xf_from")
OUTS = ("rd_status", "rd_index", "hb_commit", "xf_type", "xf_index", "xf_log_term", "xf_n",
        "qflags")


def groups(**kw):
    f = dict(G=16, inflight_cap=4, readq_cap=4, read_only=0, max_reads=2)
    f.update({p: D for p in PTRS + QUEUE})
    f.update(kw)
    return qr.RequestGroupsC(**f)


def call(rg, rin="default", rout="default", stats=D, **kw):
    lib = _lib.load()
    if rin == "default":
        rin = qr.RequestInC(**{k: kw.get(k, D) for k in INS + ("xf_term",)})
    if rout == "default":
        rout = qr.RequestOutC(**{k: kw.get(k, D) for k in OUTS})
    ref = lambda s: C.byref(s) if s is not None else None  # noqa: E731
    rc = lib.qb_dev_leader_requests(ref(rg), ref(rin), ref(rout), stats, None)
    return rc, lib.qb_last_error()


def test_the_mirrors_list_the_header_pointers():
    assert tuple(n for n, _ in qr.RequestGroupsC._fields_[5:]) == PTRS + QUEUE
    assert tuple(n for n, _ in qr.RequestInC._fields_) == INS + ("xf_term",)
    assert tuple(n for n, _ in qr.RequestOutC._fields_) == OUTS


def test_null_structs_are_einval():
    rc, err = call(None)
    assert rc == _lib.QB_EINVAL and b"rg is NULL" in err
    rc, err = call(groups(), rin=None)
    assert rc == _lib.QB_EINVAL and b"in / out is NULL" in err
    rc, err = call(groups(), rout=None)
    assert rc == _lib.QB_EINVAL and b"in / out is NULL" in err


@pytest.mark.parametrize("name", PTRS)
def test_null_group_pointer_is_einval(name):
    rc, err = call(groups(**{name: None}))
    assert rc == _lib.QB_EINVAL and b"group pointer is NULL" in err


@pytest.mark.parametrize("name", QUEUE)
def test_null_queue_pointer_is_einval_with_a_queue(name):
    rc, err = call(groups(**{name: None}))
    assert rc == _lib.QB_EINVAL and b"read queue arrays are NULL with readq_cap 4" in err


def test_null_queue_pointers_pass_the_checks_without_a_queue():
    """readq_cap == 0: the queue arrays may be NULL; the next check (here a
    NULL input) is the one that refuses."""
    rc, err = call(groups(readq_cap=0, **{p: None for p in QUEUE}), n_reads=None)
    assert rc == _lib.QB_EINVAL and b"input pointer is NULL" in err


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


@pytest.mark.parametrize("n", [0, 17, 0xFFFFFFFF])
def test_max_reads_range(n):
    rc, err = call(groups(max_reads=n))
    assert rc == _lib.QB_EINVAL and b"max_reads must be 1..16" in err


@pytest.mark.parametrize("cap", [17, 0xFFFFFFFF])
def test_readq_cap_range(cap):
    rc, err = call(groups(readq_cap=cap))
    assert rc == _lib.QB_EINVAL and b"readq_cap" in err and b"> 16" in err


@pytest.mark.parametrize("cap", [0, 4097, 0xFFFFFFFF])
def test_inflight_cap_range(cap):
    rc, err = call(groups(inflight_cap=cap))
    assert rc == _lib.QB_EINVAL and b"inflight_cap must be 1..4096" in err


@pytest.mark.parametrize("ro", [2, 0xFFFFFFFF])
def test_read_only_is_one_of_two(ro):
    rc, err = call(groups(read_only=ro))
    assert rc == _lib.QB_EINVAL and b"read_only must be 0 or 1" in err


def test_no_groups_is_ok_and_touches_nothing():
    """G == 0 returns QB_OK before any array pointer is looked at."""
    rg = groups(G=0, **{p: None for p in PTRS + QUEUE})
    rc, _ = call(rg, stats=None, **{k: None for k in INS + OUTS + ("xf_term",)})
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
        G, S, device, inflight_cap, readq_cap, read_only = 4, 4, torch.device("cpu"), 2, 4, 0
        t = {k: z64 for k in ("first_index", "snap_index", "snap_term", "max_ents", "run_start",
                              "run_term", "match", "next", "pending_snapshot", "infl_buf", "term",
                              "committed", "last_index", "rq_ctx", "rq_index")}
        t.update(off=z32, cfg=z32, meta=z32, infl_pos=z32, pstate=z8, rq_meta=z32)
    ib = qr.RequestInbox(2, z8, z64, z8, z8)
    out = qr.RequestResult(z8, z64, z64, z8, z64, z64, z64, z8, z64)
    with pytest.raises(_lib.QuorumBatchError, match="device tensor"):
        qr.leader_requests(FakeGroups, es, ib, out=out)
    for field, bad, what in (("inflight_cap", 0, "inflight_cap"), ("readq_cap", 17, "readq_cap"),
                             ("read_only", 2, "read_only")):
        keep = getattr(FakeGroups, field)
        setattr(FakeGroups, field, bad)
        with pytest.raises(_lib.QuorumBatchError, match=what):
            qr.leader_requests(FakeGroups, es, ib, out=out)
        setattr(FakeGroups, field, keep)
    with pytest.raises(_lib.QuorumBatchError, match="max_reads"):
        qr.leader_requests(FakeGroups, es, qr.RequestInbox(17, z8, z64, z8, z8), out=out)


def test_binding_layout_and_constants_match_header(tmp_path):
    """The three mirrors have the header's sizes and field offsets, and the
    module's constants the header's values (gcc on the header)."""
    structs = (("qb_request_groups", qr.RequestGroupsC),
               ("qb_request_in", qr.RequestInC), ("qb_request_out", qr.RequestOutC))
    consts = [("QB_REQ_MAX_READS", qr.MAX_READS), ("QB_MSG_APP", qr.MSG_APP),
              ("QB_MSG_SNAP", qr.MSG_SNAP), ("QB_MSG_TIMEOUT_NOW", qr.MSG_TIMEOUT_NOW),
              ("QB_QSTAT_COUNT", len(qr.QSTAT_NAMES)), ("QB_ABI_VERSION", 1)]
    consts += [("QB_RD_" + n, getattr(qr, "RD_" + n)) for n in (
        "READ_STATE", "RESP", "BCAST", "BCAST_DUP", "POSTPONED", "FORWARD", "DROPPED", "IGNORED",
        "QUEUE_FULL", "HOST", "BAD")]
    consts += [("QB_QFLAG_" + n, getattr(qr, "QFLAG_" + n)) for n in (
        "HEARTBEATS", "POSTPONED", "TRANSFER_STARTED", "TRANSFER_ABORTED", "FORWARD", "HOST", "BAD")]
    consts += [("QB_QSTAT_" + n.upper(), i) for i, n in enumerate(qr.QSTAT_NAMES)]
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
