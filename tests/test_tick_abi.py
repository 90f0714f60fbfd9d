"""qb_dev_leader_tick's host-side argument checks: every refusal by return
code and error text, with no GPU (the checks run before any HIP call), and
the binding's struct against the header's layout."""
import ctypes as C
import os
import subprocess

import pytest

from etcd_amd import _lib
from etcd_amd.quorum.tick import TickGroupsC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 0x1000  # a non-NULL pointer; never dereferenced: each check fails first
PTRS = ("off", "cfg", "meta", "committed", "match", "pstate", "rq_ctx", "role", "election_elapsed",
        "heartbeat_elapsed", "rand_timeout")


def groups(**kw):
    f = dict(G=16, readq_cap=4, election_timeout=10, heartbeat_timeout=1, check_quorum=1)
    f.update({p: D for p in PTRS})
    f.update(kw)
    return TickGroupsC(**f)


def tick(tg, tflags=D, hb_commit=D, hb_ctx=D, stats=D):
    lib = _lib.load()
    rc = lib.qb_dev_leader_tick(C.byref(tg) if tg is not None else None, tflags, hb_commit, hb_ctx,
                                stats, None)
    return rc, lib.qb_last_error()


def test_null_struct_is_einval():
    rc, err = tick(None)
    assert rc == _lib.QB_EINVAL and b"tg is NULL" in err


@pytest.mark.parametrize("name", [p for p in PTRS if p != "rq_ctx"])
def test_null_group_pointer_is_einval(name):
    rc, err = tick(groups(**{name: None}))
    assert rc == _lib.QB_EINVAL and b"group pointer is NULL" in err


@pytest.mark.parametrize("name", ["tflags", "hb_commit", "hb_ctx", "stats"])
def test_null_output_pointer_is_einval(name):
    rc, err = tick(groups(), **{name: None})
    assert rc == _lib.QB_EINVAL and b"output pointer is NULL" in err


def test_rq_ctx_null_only_without_a_read_queue():
    rc, err = tick(groups(rq_ctx=None))
    assert rc == _lib.QB_EINVAL and b"rq_ctx is NULL with readq_cap 4" in err


def test_readq_cap_bound():
    rc, err = tick(groups(readq_cap=17))
    assert rc == _lib.QB_EINVAL and b"readq_cap 17 > 16" in err


@pytest.mark.parametrize("kw", [dict(election_timeout=0), dict(heartbeat_timeout=0)])
def test_zero_timeout_is_einval(kw):
    rc, err = tick(groups(**kw))
    assert rc == _lib.QB_EINVAL and b"must be >= 1" in err


def test_check_quorum_is_a_flag():
    rc, err = tick(groups(check_quorum=2))
    assert rc == _lib.QB_EINVAL and b"check_quorum must be 0 or 1" in err


def test_no_groups_is_ok_and_touches_nothing():
    """G == 0 returns QB_OK before any pointer is looked at."""
    tg = groups(G=0, **{p: None for p in PTRS})
    rc, _ = tick(tg, None, None, None, None)
    assert rc == _lib.QB_OK


def test_python_mirror_refuses_host_tensors():
    import torch
    from etcd_amd.quorum import tick as qt
    z = torch.zeros(4, dtype=torch.int32)
    st = qt.TickState(torch.zeros(4, dtype=torch.uint8), z, z, z)

    class FakeGroups:
        G, S, readq_cap, device = 4, 4, 0, torch.device("cpu")
        t = {k: torch.zeros(8, dtype=d) for k, d in (
            ("off", torch.int32), ("cfg", torch.int32), ("meta", torch.int32),
            ("committed", torch.int64), ("match", torch.int64), ("pstate", torch.uint8),
            ("rq_ctx", torch.int64))}
    with pytest.raises(_lib.QuorumBatchError, match="device tensor"):
        qt.leader_tick(FakeGroups, st, 10, 1, True)


def test_binding_layout_matches_header(tmp_path):
    """TickGroupsC has the header's size and field offsets (gcc on the header)."""
    names = ["G", "readq_cap", "election_timeout", "heartbeat_timeout", "check_quorum"] + list(PTRS)
    src = tmp_path / "layout.c"
    fmt = " ".join(["%zu"] * (len(names) + 1))
    args = ", ".join(f"offsetof(qb_tick_groups, {n})" for n in names)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quorum_batch.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", sizeof(qb_tick_groups), {args}); '
                   'return QB_TSTAT_COUNT == 8 && QB_MSG_HEARTBEAT == 8 && QB_TFLAG_STEPPED_DOWN == '
                   'QB_LFLAG_STEPPED_DOWN && QB_ROLE_PRE_CANDIDATE == 3 ? 0 : 1; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert got == [C.sizeof(TickGroupsC)] + [getattr(TickGroupsC, n).offset for n in names]
