"""qb_dev_ready / qb_dev_advance / qb_dev_unstable_truncate: every host-side
refusal by return code and error text, with no GPU (the checks run before any
HIP call), the mirror's tensor checks, and the binding's structs and constants
against the header's."""
import ctypes as C
import importlib
import os
import subprocess

import pytest
import torch

from etcd_amd import _lib

qy = importlib.import_module("etcd_amd.quorum.ready")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 0x1000  # a non-NULL pointer; never dereferenced: each check fails first
REQUIRED = tuple(k for k in qy.COLUMNS if k != "ext")
LIST = ("rflags",) + tuple(qy._LIST)
ADV = tuple(qy._ADV)
BIG = 1 << 40


def groups(**kw):
    f = dict(G=16)
    f.update({p: D for p in qy.COLUMNS})
    f.update(kw)
    return qy.ReadyGroupsC(**f)


def ready_call(rg, ro="default", stats=D, ws=D, ws_bytes=BIG, cap=16, **kw):
    lib = _lib.load()
    if ro == "default":
        ro = qy.ReadyOutC(**{k: kw.get(k, D) for k in LIST + ("ready_count",)})
    ref = lambda s: C.byref(s) if s is not None else None  # noqa: E731
    rc = lib.qb_dev_ready(ref(rg), 1, cap, ref(ro), stats, ws, C.c_size_t(ws_bytes), None)
    return rc, lib.qb_last_error()


def advance_call(rg, ai="default", A=4, aflags=D, stats=D, **kw):
    lib = _lib.load()
    if ai == "default":
        ai = qy.AdvanceInC(**{k: kw.get(k, D) for k in ADV})
    ref = lambda s: C.byref(s) if s is not None else None  # noqa: E731
    rc = lib.qb_dev_advance(ref(rg), A, ref(ai), aflags, stats, None)
    return rc, lib.qb_last_error()


def test_null_structs_are_einval():
    rc, err = ready_call(None)
    assert rc == _lib.QB_EINVAL and b"rg is NULL" in err
    rc, err = ready_call(groups(), ro=None)
    assert rc == _lib.QB_EINVAL and b"out is NULL" in err
    rc, err = advance_call(None)
    assert rc == _lib.QB_EINVAL and b"rg is NULL" in err
    rc, err = advance_call(groups(), ai=None)
    assert rc == _lib.QB_EINVAL and b"in is NULL" in err


@pytest.mark.parametrize("name", REQUIRED)
def test_null_group_column_is_einval(name):
    rc, err = ready_call(groups(**{name: None}))
    assert rc == _lib.QB_EINVAL and b"qb_dev_ready: required group pointer is NULL" in err
    rc, err = advance_call(groups(**{name: None}))
    assert rc == _lib.QB_EINVAL and b"qb_dev_advance: required group pointer is NULL" in err


def test_ext_is_optional():
    """A NULL ext passes the group check: the next check refuses."""
    rc, err = ready_call(groups(ext=None), rflags=None)
    assert rc == _lib.QB_EINVAL and b"output pointer is NULL" in err
    rc, err = advance_call(groups(ext=None), adv_gid=None)
    assert rc == _lib.QB_EINVAL and b"input pointer is NULL" in err


@pytest.mark.parametrize("name", LIST)
def test_null_output_column_is_einval(name):
    rc, err = ready_call(groups(), **{name: None})
    assert rc == _lib.QB_EINVAL and b"output pointer is NULL" in err


def test_null_count_stats_and_workspace():
    rc, err = ready_call(groups(), ready_count=None)
    assert rc == _lib.QB_EINVAL and b"ready_count is NULL" in err
    rc, err = ready_call(groups(), stats=None)
    assert rc == _lib.QB_EINVAL and b"output pointer is NULL" in err
    rc, err = ready_call(groups(), ws=None)
    assert rc == _lib.QB_EINVAL and b"workspace too small" in err


@pytest.mark.parametrize("G", [1, 256, 257, 1 << 20, (1 << 20) + 1, 1 << 22])
def test_workspace_too_small(G):
    lib = _lib.load()
    need = lib.qb_ready_scratch_bytes(G)
    tiles = (G + 255) // 256
    assert need >= 4 * (tiles + 1) + 4 * ((tiles + 4095) // 4096 + 1)
    assert need <= 4 * tiles + 4096  # a few bytes per tile, no per-group scratch
    rc, err = ready_call(groups(G=G), ws_bytes=need - 1)
    assert rc == _lib.QB_EINVAL and b"workspace too small" in err
    rc, err = ready_call(groups(G=G), ws_bytes=need, rflags=None)  # enough: the next check refuses
    assert rc == _lib.QB_EINVAL and b"output pointer is NULL" in err


@pytest.mark.parametrize("G", [0xFFFFFFFF, 1 << 32, (1 << 64) - 1])
def test_group_count_above_the_bound(G):
    lib = _lib.load()
    assert lib.qb_ready_scratch_bytes(G) == 0
    assert lib.qb_ready_scratch_bytes(0xFFFFFFFE) > 0
    rc, err = ready_call(groups(G=G))
    assert rc == _lib.QB_EINVAL and b"ready_gid is a uint32" in err
    rc, err = advance_call(groups(G=G))
    assert rc == _lib.QB_EINVAL and b"qb_dev_advance: G" in err


@pytest.mark.parametrize("name", ADV)
def test_null_advance_column_is_einval(name):
    rc, err = advance_call(groups(), **{name: None})
    assert rc == _lib.QB_EINVAL and b"input pointer is NULL" in err


def test_null_aflags_and_stats():
    for kw in ({"aflags": None}, {"stats": None}):
        rc, err = advance_call(groups(), **kw)
        assert rc == _lib.QB_EINVAL and b"aflags / stats is NULL" in err


def test_nothing_to_do_is_ok_and_touches_nothing():
    """A == 0 and M == 0 return QB_OK before any pointer is looked at."""
    lib = _lib.load()
    rg = groups(**{p: None for p in qy.COLUMNS})
    assert lib.qb_dev_advance(C.byref(rg), 0, None, None, None, None) == _lib.QB_OK
    assert lib.qb_dev_unstable_truncate(0, None, None, 16, None, None) == _lib.QB_OK


def test_truncate_null_columns():
    lib = _lib.load()
    assert lib.qb_dev_unstable_truncate(4, None, D, 16, D, None) == _lib.QB_EINVAL
    assert b"group / app_from is NULL" in lib.qb_last_error()
    assert lib.qb_dev_unstable_truncate(4, D, None, 16, D, None) == _lib.QB_EINVAL
    assert lib.qb_dev_unstable_truncate(4, D, D, 16, None, None) == _lib.QB_EINVAL
    assert b"unstable_offset is NULL" in lib.qb_last_error()


def _host_state(G=8):
    t = {}
    for k, (dt, _, per) in qy.COLUMNS.items():
        t[k] = torch.zeros(per * G, dtype=qy._TORCH[dt])
    return qy.ReadyState(G, t)


def test_python_mirror_refuses_host_tensors_and_bad_shapes():
    st = _host_state()
    with pytest.raises(_lib.QuorumBatchError, match="device tensor"):
        qy.ready(st)
    recs = qy.AdvanceRecords(2, {k: torch.zeros(2, dtype=qy._TORCH[dt])
                                 for k, (dt, _) in qy._ADV.items()})
    with pytest.raises(_lib.QuorumBatchError, match="device tensor"):
        qy.advance(st, recs)
    with pytest.raises(_lib.QuorumBatchError, match="device tensor"):
        qy.unstable_truncate(st, torch.zeros(2, dtype=torch.int32),
                             torch.zeros(2, dtype=torch.int64))
    missing = _host_state()
    missing.t["applied"] = None
    with pytest.raises(_lib.QuorumBatchError, match="applied is missing"):
        qy.ready(missing)
    big = _host_state()
    big.G = qy.MAX_GROUPS + 1
    with pytest.raises(_lib.QuorumBatchError, match="G must be"):
        qy.ready(big)


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
    """dtype, length and contiguity of every kind of column, with the
    device test stood in for (the checks' module sees _Dev as its tensor type)."""
    import types

    from etcd_amd.quorum import _checks
    monkeypatch.setattr(_checks, "torch", types.SimpleNamespace(Tensor=_Dev))
    G = 8
    for name, bad in (("role", torch.zeros(G, dtype=torch.int64)),          # dtype
                      ("run_start", torch.zeros(G, dtype=torch.int64)),      # 8 rows short
                      ("prev_lead", torch.zeros(2 * G, dtype=torch.int64)[::2]),  # strided
                      ("meta", torch.zeros(G - 1, dtype=torch.int32))):      # short
        st = _host_state(G)
        st.t = {k: (_Dev(v) if v is not None else None) for k, v in st.t.items()}
        st.t[name] = _Dev(bad)
        with pytest.raises(_lib.QuorumBatchError, match=name):
            st.check()
    st = _host_state(G)
    st.t = {k: _Dev(v) for k, v in st.t.items()}
    st.check()
    other = _Dev(torch.zeros(G, dtype=torch.int64))
    other.device = "dev1"
    st.t["applied"] = other
    with pytest.raises(_lib.QuorumBatchError, match="applied is on dev1"):
        st.check()


def test_from_numpy_checks_lengths():
    import numpy as np
    a = {k: np.zeros(per * 4, dt) for k, (dt, _, per) in qy.COLUMNS.items()}
    a["vote"] = np.zeros(3, np.uint64)
    with pytest.raises(_lib.QuorumBatchError, match="vote has 3 entries, want 4"):
        qy.ReadyState.from_numpy(a, device="cpu")
    del a["vote"]
    with pytest.raises(_lib.QuorumBatchError, match="vote is missing"):
        qy.ReadyState.from_numpy(a, device="cpu")
    with pytest.raises(_lib.QuorumBatchError, match="hs_term has 1 entries"):
        qy.AdvanceRecords.from_numpy({"adv_gid": np.zeros(2, np.uint32),
                                      "hs_term": np.zeros(1, np.uint64)}, device="cpu")


def test_binding_layout_and_constants_match_header(tmp_path):
    """The three mirrors have the header's sizes and field offsets, and the
    module's constants the header's values (gcc on the header)."""
    structs = (("qb_ready_groups", qy.ReadyGroupsC), ("qb_ready_out", qy.ReadyOutC),
               ("qb_advance_in", qy.AdvanceInC))
    consts = [("QB_RSTAT_COUNT", len(qy.RSTAT_NAMES)), ("QB_ASTAT_COUNT", len(qy.ASTAT_NAMES)),
              ("QB_READY_MAX_GROUPS == 0xFFFFFFFEull", 1), ("QB_ROLE_PROMOTABLE", qy.ROLE_PROMOTABLE),
              ("QB_LEADER_MAX_RUNS", qy.MAX_RUNS)]
    consts += [("QB_RDF_" + n, getattr(qy, "RDF_" + n)) for n in (
        "SOFT", "HARD", "ENTRIES", "SNAPSHOT", "COMMITTED", "MSGS", "READSTATES", "MUST_SYNC",
        "BAD_LOG", "DEFERRED")]
    consts += [("QB_RDP_MSGS", qy.RDP_MSGS), ("QB_RDP_READSTATES", qy.RDP_READSTATES)]
    consts += [("QB_AFLAG_" + n, getattr(qy, "AFLAG_" + n)) for n in (
        "APPLIED_RANGE", "AUTO_LEAVE", "STABLE_STALE", "BAD_GROUP")]
    consts += [("QB_RSTAT_" + n.upper(), i) for i, n in enumerate(qy.RSTAT_NAMES)]
    consts += [("QB_ASTAT_" + n.upper(), i) for i, n in enumerate(qy.ASTAT_NAMES)]
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
    # the test restatement's names are the mirror's
    from tests import ready_ref as R
    assert R.RSTAT_NAMES == qy.RSTAT_NAMES and R.ASTAT_NAMES == qy.ASTAT_NAMES
