"""qb_dev_follower_step's host-side argument checks: every refusal by return
code and error text, with no GPU (the checks run before any HIP call), the
binding's structs against the header's layout, and the Python mirror's tensor
checks."""
import ctypes as C
import os
import subprocess

import pytest

from etcd_amd import _lib
from etcd_amd.quorum.follower import FSTAT_NAMES, FollowerGroupsC, FollowerInboxC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 0x1000  # a non-NULL pointer; never dereferenced: each check fails first
GROUP_PTRS = ("term", "vote", "lead", "committed", "last_index", "last_term", "role",
              "election_elapsed", "heartbeat_elapsed")
INBOX_PTRS = ("group", "flags", "from", "term", "index", "aux")
OUTPUTS = ("resp_type", "resp_term", "stop_at", "gflags", "stats")


def groups(**kw):
    f = dict(G=16, election_timeout=10, check_quorum=1, pre_vote=1, reserved=0)
    f.update({p: D for p in GROUP_PTRS})
    f.update(kw)
    return FollowerGroupsC(**f)


def inbox(M=32, **kw):
    f = {p: D for p in INBOX_PTRS}
    f.update(kw)
    ib = FollowerInboxC(M=M)
    for k, v in f.items():
        setattr(ib, k, v)
    return ib


def step(fg, ib, ws=D, ws_bytes=1 << 40, **out):
    lib = _lib.load()
    o = {k: D for k in OUTPUTS}
    o.update(out)
    rc = lib.qb_dev_follower_step(C.byref(fg) if fg is not None else None,
                                  C.byref(ib) if ib is not None else None,
                                  *[o[k] for k in OUTPUTS], ws, C.c_size_t(ws_bytes), None)
    return rc, lib.qb_last_error()


def test_null_structs_are_einval():
    rc, err = step(None, inbox())
    assert rc == _lib.QB_EINVAL and b"fg is NULL" in err
    rc, err = step(groups(), None)
    assert rc == _lib.QB_EINVAL and b"in is NULL" in err


@pytest.mark.parametrize("name", GROUP_PTRS)
def test_null_group_pointer_is_einval(name):
    rc, err = step(groups(**{name: None}), inbox())
    assert rc == _lib.QB_EINVAL and b"group pointer is NULL" in err


@pytest.mark.parametrize("name", INBOX_PTRS)
def test_null_inbox_pointer_is_einval(name):
    rc, err = step(groups(), inbox(**{name: None}))
    assert rc == _lib.QB_EINVAL and b"inbox pointer is NULL" in err


@pytest.mark.parametrize("name", OUTPUTS)
def test_null_output_pointer_is_einval(name):
    rc, err = step(groups(), inbox(), **{name: None})
    assert rc == _lib.QB_EINVAL and b"output pointer is NULL" in err


def test_zero_election_timeout_is_einval():
    rc, err = step(groups(election_timeout=0), inbox())
    assert rc == _lib.QB_EINVAL and b"election_timeout must be >= 1" in err


@pytest.mark.parametrize("name", ["check_quorum", "pre_vote"])
def test_flags_are_flags(name):
    rc, err = step(groups(**{name: 2}), inbox())
    assert rc == _lib.QB_EINVAL and f"{name} must be 0 or 1".encode() in err


def test_workspace_is_required_and_sized():
    lib = _lib.load()
    need = lib.qb_follower_workspace_bytes(16, 32)
    assert need >= 4 * (16 + 1) + 4 * 32
    rc, err = step(groups(), inbox(), ws=None)
    assert rc == _lib.QB_EINVAL and b"workspace is NULL" in err
    rc, err = step(groups(), inbox(), ws_bytes=need - 1)
    assert rc == _lib.QB_EINVAL and b"workspace too small" in err
    # grows with both the groups and the records
    assert lib.qb_follower_workspace_bytes(1 << 20, 32) > need
    assert lib.qb_follower_workspace_bytes(16, 1 << 20) > need


def test_record_count_bound():
    lib = _lib.load()
    assert lib.qb_follower_workspace_bytes(16, (1 << 32) - 2) > 0
    assert lib.qb_follower_workspace_bytes(16, (1 << 32) - 1) == 0
    rc, err = step(groups(), inbox(M=(1 << 32) - 1))
    assert rc == _lib.QB_EINVAL and b"2^32 - 2" in err


def test_no_groups_is_ok_and_touches_nothing():
    """G == 0 returns QB_OK before any pointer is looked at."""
    fg = groups(G=0, **{p: None for p in GROUP_PTRS})
    rc, _ = step(fg, inbox(**{p: None for p in INBOX_PTRS}), ws=None, ws_bytes=0,
                 **{k: None for k in OUTPUTS})
    assert rc == _lib.QB_OK


def test_python_mirror_refuses_bad_tensors():
    import torch
    from etcd_amd.quorum import follower as qf, tick as qt
    z32 = torch.zeros(4, dtype=torch.int32)
    z64 = torch.zeros(4, dtype=torch.int64)
    st = qt.TickState(torch.zeros(4, dtype=torch.uint8), z32, z32, z32)
    fg = qf.FollowerGroups(4, 10, True, True, {k: z64 for k in qf._U64_FIELDS}, st)
    ib = qf.FollowerInbox(z32, torch.zeros(4, dtype=torch.uint8), z64, z64, z64, z64)
    with pytest.raises(_lib.QuorumBatchError, match="device tensor"):
        qf.follower_step(fg, ib)
    ib._m = -1
    with pytest.raises(_lib.QuorumBatchError, match="non-negative"):
        qf.follower_step(fg, ib)
    ib._m = 1 << 32
    with pytest.raises(_lib.QuorumBatchError, match="2\\^32 - 2"):
        qf.follower_step(fg, ib)
    with pytest.raises(_lib.QuorumBatchError, match="election_timeout"):
        qf.follower_step(qf.FollowerGroups(4, 0, True, True, fg.t, st), ib)
    import numpy as np
    with pytest.raises(_lib.QuorumBatchError, match="lack vote"):
        qf.FollowerGroups.from_numpy({"term": np.zeros(4, np.uint64)}, st, 10, True, True, "cpu")
    with pytest.raises(_lib.QuorumBatchError, match="entries"):
        qf.FollowerInbox.from_numpy(np.zeros(4), np.zeros(3), np.zeros(4), np.zeros(4),
                                    np.zeros(4), np.zeros(4), "cpu")


def test_binding_layout_matches_header(tmp_path):
    """FollowerGroupsC / FollowerInboxC have the header's sizes and field
    offsets (gcc on the header), and the mirror's constants its values."""
    gnames = ["G", "election_timeout", "check_quorum", "pre_vote", "reserved"] + list(GROUP_PTRS)
    inames = ["M"] + list(INBOX_PTRS)
    args = ", ".join(["sizeof(qb_follower_groups)"] +
                     [f"offsetof(qb_follower_groups, {n})" for n in gnames] +
                     ["sizeof(qb_follower_inbox)"] +
                     [f"offsetof(qb_follower_inbox, {n})" for n in inames])
    fmt = " ".join(["%zu"] * (len(gnames) + len(inames) + 2))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quorum_batch.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", {args}); '
                   f'return QB_FSTAT_COUNT == {len(FSTAT_NAMES)} && QB_FIN_HOST == 4 && '
                   'QB_FREC_FORCE == 0x80 && QB_FRESP_PREVOTE_RESP == 18 && '
                   'QB_FRESP_HEARTBEAT_RESP == 9 && QB_FRESP_VOTE_RESP == 6 && '
                   'QB_FRESP_APP_RESP == 4 && QB_FFLAG_HARDSTATE == 0x10 && '
                   'QB_FSTAT_BAD_KIND == 10 ? 0 : 1; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    want = ([C.sizeof(FollowerGroupsC)] + [getattr(FollowerGroupsC, n).offset for n in gnames] +
            [C.sizeof(FollowerInboxC)] + [getattr(FollowerInboxC, n).offset for n in inames])
    assert got == want
