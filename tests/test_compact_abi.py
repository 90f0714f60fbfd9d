"""qb_dev_log_compact: every host-side refusal by return code and error text,
with no GPU (the checks run before any HIP call), the scratch size, the
mirror's tensor checks, and the binding's structs and constants against the
header's."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from etcd_amd import _lib
from etcd_amd.quorum import compact as qcm
from etcd_amd.quorum.follower import FollowerLog
from etcd_amd.quorum.ready import MAX_GROUPS, ReadyState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 0x1000  # a non-NULL pointer; never dereferenced: each check fails first
GROUP = qcm._GROUP_FIELDS
LIST = ("cmflags",) + tuple(qcm._LIST)
REQUEST = ("snap_at", "compact_at", "force", "hold")
BIG = 1 << 40


def groups(**kw):
    f = dict(G=16)
    f.update({p: D for p in GROUP})
    f.update(kw)
    return qcm.CompactGroupsC(**f)


def request(mode=qcm.CM_EXPLICIT, **kw):
    f = dict(mode=mode, reserved=0, snapshot_count=10, catch_up_entries=5)
    f.update({p: D for p in REQUEST})
    f.update(kw)
    return qcm.CompactInC(**f)


def call(cg, ci="default", co="default", stats=D, ws=D, ws_bytes=BIG, cap=16, **kw):
    lib = _lib.load()
    if ci == "default":
        ci = request()
    if co == "default":
        co = qcm.CompactOutC(**{k: kw.get(k, D) for k in LIST + ("list_count",)})
    ref = lambda s: C.byref(s) if s is not None else None  # noqa: E731
    rc = lib.qb_dev_log_compact(ref(cg), ref(ci), cap, ref(co), stats, ws, C.c_size_t(ws_bytes), None)
    return rc, lib.qb_last_error()


def test_null_structs_are_einval():
    rc, err = call(None)
    assert rc == _lib.QB_EINVAL and b"cg is NULL" in err
    rc, err = call(groups(), ci=None)
    assert rc == _lib.QB_EINVAL and b"in is NULL" in err
    rc, err = call(groups(), co=None)
    assert rc == _lib.QB_EINVAL and b"out is NULL" in err


@pytest.mark.parametrize("mode", [2, 3, 0xFFFFFFFF])
def test_bad_mode_is_einval(mode):
    rc, err = call(groups(), ci=request(mode=mode))
    assert rc == _lib.QB_EINVAL and b"neither QB_CM_EXPLICIT nor QB_CM_TRIGGER" in err
    rc, err = call(groups(G=0), ci=request(mode=mode))      # before the G == 0 return too
    assert rc == _lib.QB_EINVAL and b"neither" in err


@pytest.mark.parametrize("name", GROUP)
def test_null_group_column_is_einval(name):
    for mode in (qcm.CM_EXPLICIT, qcm.CM_TRIGGER):
        rc, err = call(groups(**{name: None}), ci=request(mode=mode))
        assert rc == _lib.QB_EINVAL and b"qb_dev_log_compact: required group pointer is NULL" in err


@pytest.mark.parametrize("name", REQUEST)
def test_request_columns_are_optional(name):
    """A NULL request column passes: the next check refuses."""
    for mode in (qcm.CM_EXPLICIT, qcm.CM_TRIGGER):
        rc, err = call(groups(), ci=request(mode=mode, **{name: None}), cmflags=None)
        assert rc == _lib.QB_EINVAL and b"output pointer is NULL" in err


@pytest.mark.parametrize("name", LIST)
def test_null_output_column_is_einval(name):
    rc, err = call(groups(), **{name: None})
    assert rc == _lib.QB_EINVAL and b"output pointer is NULL" in err
    rc, err = call(groups(), cap=0, **{name: None})           # with list_cap == 0 too
    assert rc == _lib.QB_EINVAL and b"output pointer is NULL" in err


def test_null_count_stats_and_workspace():
    rc, err = call(groups(), list_count=None)
    assert rc == _lib.QB_EINVAL and b"list_count is NULL" in err
    rc, err = call(groups(G=0), list_count=None)
    assert rc == _lib.QB_EINVAL and b"list_count is NULL" in err
    rc, err = call(groups(), stats=None)
    assert rc == _lib.QB_EINVAL and b"output pointer is NULL" in err
    rc, err = call(groups(), ws=None)
    assert rc == _lib.QB_EINVAL and b"workspace too small" in err


@pytest.mark.parametrize("G", [1, 256, 257, 1 << 20, (1 << 20) + 1, 1 << 22])
def test_scratch_size_and_a_short_workspace(G):
    lib = _lib.load()
    need = lib.qb_log_compact_scratch_bytes(G)
    tiles = (G + 255) // 256
    assert need >= 4 * (tiles + 1) + 4 * ((tiles + 4095) // 4096 + 1)
    assert need <= 4 * tiles + 4096  # a few bytes per tile, no per-group scratch
    assert need == lib.qb_ready_scratch_bytes(G)   # the same carve: tile counts and the scan's sums
    rc, err = call(groups(G=G), ws_bytes=need - 1)
    assert rc == _lib.QB_EINVAL and b"workspace too small" in err
    rc, err = call(groups(G=G), ws_bytes=need, cmflags=None)  # enough: the next check refuses
    assert rc == _lib.QB_EINVAL and b"output pointer is NULL" in err


@pytest.mark.parametrize("G", [0xFFFFFFFF, 1 << 32, (1 << 64) - 1])
def test_group_count_above_the_bound(G):
    lib = _lib.load()
    assert lib.qb_log_compact_scratch_bytes(G) == 0
    assert lib.qb_log_compact_scratch_bytes(0xFFFFFFFE) > 0
    rc, err = call(groups(G=G))
    assert rc == _lib.QB_EINVAL and b"gid is a uint32" in err


def _host_args(G=8):
    z = lambda n, dt=torch.int64: torch.zeros(n, dtype=dt)  # noqa: E731
    log = FollowerLog(G, z(G, torch.int32), z(G), z(8 * G), z(8 * G))
    ready = ReadyState(G, {k: z(G) for k in ("last_index", "applied", "unstable_offset", "usnap_index")})
    return log, ready, z(G), z(G)


def test_python_mirror_refuses_before_the_c_call():
    log, ready, si, st = _host_args()
    with pytest.raises(_lib.QuorumBatchError, match="device tensor"):
        qcm.log_compact(log, ready, si, st, qcm.CompactRequest.explicit())
    ready.t["applied"] = None
    with pytest.raises(_lib.QuorumBatchError, match="applied is missing"):
        qcm.log_compact(log, ready, si, st, qcm.CompactRequest.explicit())
    log, ready, si, st = _host_args()
    ready.G = 9
    with pytest.raises(_lib.QuorumBatchError, match="the ready state 9"):
        qcm.log_compact(log, ready, si, st, qcm.CompactRequest.explicit())
    log, ready, si, st = _host_args()
    log.G = ready.G = MAX_GROUPS + 1
    with pytest.raises(_lib.QuorumBatchError, match="G must be"):
        qcm.log_compact(log, ready, si, st, qcm.CompactRequest.explicit())
    with pytest.raises(_lib.QuorumBatchError, match="CM_EXPLICIT or CM_TRIGGER"):
        qcm.CompactRequest(7).check()
    with pytest.raises(_lib.QuorumBatchError, match="snapshot_count must be a uint64"):
        qcm.CompactRequest.trigger(-1, 0).check()
    with pytest.raises(_lib.QuorumBatchError, match="catch_up_entries must be a uint64"):
        qcm.CompactRequest.trigger(0, 1 << 64).check()


class _Dev:
    """check_tensors' view of a tensor: lets the dtype / length / stride
    refusals be reached without a device."""

    def __init__(self, t):
        self.t = t
        self.is_cuda, self.dtype, self.device = True, t.dtype, "dev0"

    def is_contiguous(self):
        return self.t.is_contiguous()

    def numel(self):
        return self.t.numel()


def test_tensor_checks_name_the_column(monkeypatch):
    """dtype, length, contiguity and device of the state, request and output
    columns, with the device test stood in for."""
    import types

    from etcd_amd.quorum import _checks
    monkeypatch.setattr(_checks, "torch", types.SimpleNamespace(Tensor=_Dev))
    G = 8

    def args():
        log, ready, si, st = _host_args(G)
        log = FollowerLog(G, _Dev(log.meta), _Dev(log.first_index), _Dev(log.run_start),
                          _Dev(log.run_term))
        ready.t = {k: _Dev(v) for k, v in ready.t.items()}
        return log, ready, _Dev(si), _Dev(st)

    ex = qcm.CompactRequest.explicit
    log, ready, si, st = args()
    log.meta = _Dev(torch.zeros(G, dtype=torch.int64))                       # dtype
    with pytest.raises(_lib.QuorumBatchError, match="meta"):
        qcm.log_compact(log, ready, si, st, ex())
    log, ready, si, st = args()
    log.run_term = _Dev(torch.zeros(G, dtype=torch.int64))                   # 8 rows short
    with pytest.raises(_lib.QuorumBatchError, match="run_term"):
        qcm.log_compact(log, ready, si, st, ex())
    log, ready, si, st = args()
    ready.t["usnap_index"] = _Dev(torch.zeros(2 * G, dtype=torch.int64)[::2])  # strided
    with pytest.raises(_lib.QuorumBatchError, match="usnap_index"):
        qcm.log_compact(log, ready, si, st, ex())
    log, ready, si, st = args()
    with pytest.raises(_lib.QuorumBatchError, match="snap_term"):             # short
        qcm.log_compact(log, ready, si, _Dev(torch.zeros(G - 1, dtype=torch.int64)), ex())
    other = _Dev(torch.zeros(G, dtype=torch.int64))
    other.device = "dev1"
    with pytest.raises(_lib.QuorumBatchError, match="snap_index is on dev1"):
        qcm.log_compact(log, ready, other, st, ex())
    with pytest.raises(_lib.QuorumBatchError, match="compact_at"):
        qcm.log_compact(log, ready, si, st, ex(None, _Dev(torch.zeros(G - 1, dtype=torch.int64))),
                        out=_fake_out(G, G))
    with pytest.raises(_lib.QuorumBatchError, match="hold"):
        qcm.log_compact(log, ready, si, st,
                        qcm.CompactRequest.trigger(1, 1, None, _Dev(torch.zeros(G, dtype=torch.int64))),
                        out=_fake_out(G, G))
    out = _fake_out(G, G)
    out.cols["first_before"] = _Dev(torch.zeros(G - 1, dtype=torch.int64))
    with pytest.raises(_lib.QuorumBatchError, match="first_before"):
        qcm.log_compact(log, ready, si, st, ex(), out=out)
    with pytest.raises(_lib.QuorumBatchError, match="list_cap must be non-negative"):
        qcm.log_compact(log, ready, si, st, ex(), out=_fake_out(G, G), list_cap=-1)


def _fake_out(G, cap):
    z = lambda n, dt: _Dev(torch.zeros(max(n, 1), dtype=dt))  # noqa: E731
    return qcm.CompactResult(G, cap, z(G, torch.int16),
                             {k: z(cap, qcm._TORCH[dt]) for k, (dt, _) in qcm._LIST.items()},
                             z(1, torch.int64), z(len(qcm.CMSTAT_NAMES), torch.int64))


def test_binding_layout_and_constants_match_header(tmp_path):
    """The three mirrors have the header's sizes and field offsets, and the
    module's constants the header's values (gcc on the header)."""
    structs = (("qb_compact_groups", qcm.CompactGroupsC), ("qb_compact_in", qcm.CompactInC),
               ("qb_compact_out", qcm.CompactOutC))
    consts = [("QB_CMSTAT_COUNT", len(qcm.CMSTAT_NAMES)), ("QB_CM_EXPLICIT", qcm.CM_EXPLICIT),
              ("QB_CM_TRIGGER", qcm.CM_TRIGGER), ("QB_READY_MAX_GROUPS == 0xFFFFFFFEull", 1)]
    consts += [("QB_CMF_" + n, getattr(qcm, "CMF_" + n)) for n in (
        "SNAPPED", "COMPACTED", "SNAP_OUT_OF_DATE", "ALREADY_COMPACTED", "OUT_OF_BOUND",
        "PAST_APPLIED", "HELD", "PENDING_SNAPSHOT", "BAD_LOG", "DEFERRED")]
    consts += [("QB_CMSTAT_" + n.upper(), i) for i, n in enumerate(qcm.CMSTAT_NAMES)]
    items, want = [], []
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
    # the test restatement's names and flags are the mirror's
    from tests import compact_ref as R
    assert R.STAT_NAMES == qcm.CMSTAT_NAMES
    assert [getattr(R, n.upper()) for n in R.FLAG_NAMES] == [1 << b for b in range(10)]
    for n in R.FLAG_NAMES:
        assert getattr(R, n.upper()) == getattr(qcm, "CMF_" + n.upper())
