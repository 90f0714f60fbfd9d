"""qb_dev_campaign's host-side argument checks: every refusal by return code
and error text, with no GPU (the checks run before any HIP call), and the
binding's struct against the header's layout."""
import ctypes as C
import importlib
import os
import subprocess

import pytest

from etcd_amd import _lib

# (the package exports the function campaign() under the module's own name)
qc = importlib.import_module("etcd_amd.quorum.campaign")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 0x1000  # a non-NULL pointer; never dereferenced: each check fails first
PTRS = ("off", "cfg", "meta", "self_id", "term", "vote", "lead", "committed", "last_index",
        "last_term", "role", "election_elapsed", "heartbeat_elapsed", "votes", "match", "next",
        "pending_snapshot", "pstate", "infl_pos")
OUTS = ("action", "cflags", "req_type", "req_term", "req_mask", "stats")


def groups(**kw):
    f = dict(G=16, pre_vote=1, reserved=0)
    f.update({p: D for p in PTRS})
    f.update(kw)
    return qc.CampaignGroupsC(**f)


def call(cg, **kw):
    lib = _lib.load()
    out = {k: D for k in OUTS}
    out.update(kw)
    rc = lib.qb_dev_campaign(C.byref(cg) if cg is not None else None, *[out[k] for k in OUTS], None)
    return rc, lib.qb_last_error()


def test_the_mirror_lists_the_header_pointers():
    assert tuple(n for n, _ in qc.CampaignGroupsC._fields_[3:]) == PTRS


def test_null_struct_is_einval():
    rc, err = call(None)
    assert rc == _lib.QB_EINVAL and b"cg is NULL" in err


@pytest.mark.parametrize("name", PTRS)
def test_null_group_pointer_is_einval(name):
    rc, err = call(groups(**{name: None}))
    assert rc == _lib.QB_EINVAL and b"group pointer is NULL" in err


@pytest.mark.parametrize("name", OUTS)
def test_null_output_pointer_is_einval(name):
    rc, err = call(groups(), **{name: None})
    assert rc == _lib.QB_EINVAL and b"output pointer is NULL" in err


def test_pre_vote_is_a_flag():
    rc, err = call(groups(pre_vote=2))
    assert rc == _lib.QB_EINVAL and b"pre_vote must be 0 or 1" in err


def test_no_groups_is_ok_and_touches_nothing():
    """G == 0 returns QB_OK before any pointer is looked at."""
    cg = groups(G=0, **{p: None for p in PTRS})
    rc, _ = call(cg, **{k: None for k in OUTS})
    assert rc == _lib.QB_OK


def test_python_mirror_refuses_host_tensors():
    import torch
    from etcd_amd.quorum import follower as qf, tick as qt
    z32, z64 = torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int64)
    st = qt.TickState(torch.zeros(4, dtype=torch.uint8), z32, z32, z32)
    fg = qf.FollowerGroups(4, 10, False, True, {k: z64 for k in (
        "term", "vote", "lead", "committed", "last_index", "last_term")}, st)
    es = qc.ElectionState(z64, z32, fg)

    class FakeGroups:
        G, S, device = 4, 4, torch.device("cpu")
        t = {"off": z32, "cfg": z32, "meta": z32, "match": z64, "next": z64,
             "pending_snapshot": z64, "pstate": torch.zeros(8, dtype=torch.uint8), "infl_pos": z32}
    with pytest.raises(_lib.QuorumBatchError, match="device tensor"):
        qc.campaign(FakeGroups, es, torch.zeros(4, dtype=torch.uint8))


def test_binding_layout_and_constants_match_header(tmp_path):
    """CampaignGroupsC has the header's size and field offsets, and the
    module's constants the header's values (gcc on the header)."""
    names = ["G", "pre_vote", "reserved"] + list(PTRS)
    consts = [("QB_CAMP_NONE", qc.CAMP_NONE), ("QB_CAMP_HUP", qc.CAMP_HUP),
              ("QB_CAMP_TRANSFER", qc.CAMP_TRANSFER), ("QB_CAMP_WON", qc.CAMP_WON),
              ("QB_CAMP_LOST", qc.CAMP_LOST), ("QB_CAMP_PENDING_CONF", qc.CAMP_PENDING_CONF),
              ("QB_MSG_VOTE", qc.MSG_VOTE), ("QB_MSG_PREVOTE", qc.MSG_PREVOTE),
              ("QB_CREQ_TRANSFER", qc.CREQ_TRANSFER), ("QB_CFLAG_REQUESTS", qc.CFLAG_REQUESTS),
              ("QB_CFLAG_BECAME_LEADER", qc.CFLAG_BECAME_LEADER),
              ("QB_CFLAG_BCAST_APPEND", qc.CFLAG_BCAST_APPEND), ("QB_CFLAG_RESET", qc.CFLAG_RESET),
              ("QB_CFLAG_HARDSTATE", qc.CFLAG_HARDSTATE), ("QB_CFLAG_IGNORED", qc.CFLAG_IGNORED),
              ("QB_CSTAT_COUNT", len(qc.CSTAT_NAMES)), ("QB_CSTAT_BAD_ACTION", 9),
              ("QB_CSTAT_VOTE_REQUESTS", qc.CSTAT_NAMES.index("vote_requests")),
              ("QB_CFLAG_RESET == QB_FFLAG_RESET", 1), ("QB_CREQ_TRANSFER == QB_FREC_FORCE", 1)]
    src = tmp_path / "layout.c"
    fmt = " ".join(["%zu"] * (len(names) + 1) + ["%d"] * len(consts))
    args = ", ".join([f"offsetof(qb_campaign_groups, {n})" for n in names] +
                     [f"(int)({c})" for c, _ in consts])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quorum_batch.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", sizeof(qb_campaign_groups), {args}); '
                   'return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert got == [C.sizeof(qc.CampaignGroupsC)] + \
        [getattr(qc.CampaignGroupsC, n).offset for n in names] + [v for _, v in consts]
