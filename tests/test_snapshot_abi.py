"""qb_dev_follower_snapshot: every host-side refusal by return code and error
text, with no GPU (the checks run before any HIP call), the wrapper's
duplicate-group refusal and tensor checks, and the binding's structs and
constants against the header's."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

from etcd_amd import _lib
from etcd_amd.quorum import follower as qf, snapshot as qs, tick as qt

qy = importlib.import_module("etcd_amd.quorum.ready")  # (the package exports the function ready)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 0x1000  # a non-NULL pointer; never dereferenced: each check fails first
GROUP_PTRS = tuple(qs._GROUP_FIELDS)
REQUIRED = tuple(k for k in GROUP_PTRS if k != "pending")
IN_PTRS = tuple(qs._RECORD) + ("cs_off", "cs_id", "cs_set")
OUT_PTRS = ("sflags", "resp_type", "resp_term", "resp_index")


def groups(**kw):
    f = dict(G=16, election_timeout=10, check_quorum=1, pre_vote=1, reserved=0)
    f.update({p: D for p in GROUP_PTRS})
    f.update(kw)
    return qs.SnapshotGroupsC(**f)


def inbox(**kw):
    f = dict(R=4, C=8)
    f.update({p: D for p in IN_PTRS})
    f.update(kw)
    return qs.SnapshotInboxC(**f)


def outs(**kw):
    f = {p: D for p in OUT_PTRS}
    f.update(kw)
    return qs.SnapshotOutC(**f)


def call(sg="default", ib="default", so="default", stats=D):
    lib = _lib.load()
    sg = groups() if sg == "default" else sg
    ib = inbox() if ib == "default" else ib
    so = outs() if so == "default" else so
    ref = lambda s: C.byref(s) if s is not None else None  # noqa: E731
    rc = lib.qb_dev_follower_snapshot(ref(sg), ref(ib), ref(so), stats, None)
    return rc, lib.qb_last_error()


def test_null_structs_are_einval():
    rc, err = call(sg=None)
    assert rc == _lib.QB_EINVAL and b"sg is NULL" in err
    rc, err = call(ib=None)
    assert rc == _lib.QB_EINVAL and b"in is NULL" in err
    rc, err = call(so=None)
    assert rc == _lib.QB_EINVAL and b"out is NULL" in err


@pytest.mark.parametrize("name", REQUIRED)
def test_null_group_column_is_einval(name):
    rc, err = call(sg=groups(**{name: None}))
    assert rc == _lib.QB_EINVAL and b"qb_dev_follower_snapshot: required group pointer is NULL" in err


def test_pending_is_optional():
    """A NULL pending passes the group check: the next check refuses."""
    rc, err = call(sg=groups(pending=None), ib=inbox(group=None))
    assert rc == _lib.QB_EINVAL and b"input pointer is NULL" in err


@pytest.mark.parametrize("name", IN_PTRS)
def test_null_input_column_is_einval(name):
    rc, err = call(ib=inbox(**{name: None}))
    assert rc == _lib.QB_EINVAL and b"required input pointer is NULL" in err


def test_conf_state_columns_are_not_needed_without_ids():
    """C == 0: cs_id / cs_set may be NULL; the next check refuses."""
    rc, err = call(ib=inbox(C=0, cs_id=None, cs_set=None), so=outs(sflags=None))
    assert rc == _lib.QB_EINVAL and b"output pointer is NULL" in err


@pytest.mark.parametrize("name", OUT_PTRS + ("stats",))
def test_null_output_column_is_einval(name):
    rc, err = call(stats=None) if name == "stats" else call(so=outs(**{name: None}))
    assert rc == _lib.QB_EINVAL and b"required output pointer is NULL" in err


@pytest.mark.parametrize("G", [0xFFFFFFFF, 1 << 32, (1 << 64) - 1])
def test_group_count_above_the_bound(G):
    rc, err = call(sg=groups(G=G))
    assert rc == _lib.QB_EINVAL and b"qb_dev_follower_snapshot: G" in err


@pytest.mark.parametrize("R", [0xFFFFFFFF, 1 << 32, (1 << 64) - 1])
def test_record_count_above_the_bound(R):
    rc, err = call(ib=inbox(R=R))
    assert rc == _lib.QB_EINVAL and b"2^32 - 2" in err


def test_nothing_to_do_is_ok_and_touches_nothing():
    """R == 0 or G == 0 returns QB_OK before any pointer is looked at."""
    none_g = groups(**{p: None for p in GROUP_PTRS})
    none_i = inbox(**{p: None for p in IN_PTRS})
    none_o = outs(**{p: None for p in OUT_PTRS})
    lib = _lib.load()
    for sg, ib in ((groups(G=0, **{p: None for p in GROUP_PTRS}), none_i),
                   (none_g, inbox(R=0, **{p: None for p in IN_PTRS}))):
        assert lib.qb_dev_follower_snapshot(C.byref(sg), C.byref(ib), C.byref(none_o), None,
                                            None) == _lib.QB_OK


def test_the_call_has_no_workspace_export():
    lib = _lib.load()
    for name in ("qb_snapshot_workspace_bytes", "qb_follower_snapshot_workspace_bytes",
                 "qb_snapshot_scratch_bytes"):
        assert not hasattr(lib, name)
    assert _lib.SIGNATURES["qb_dev_follower_snapshot"] == (C.c_int, [C.c_void_p] * 5)


# ---- the wrapper ----
def _host_state(G=8):
    z = lambda dt, n=G: torch.zeros(n, dtype=dt)  # noqa: E731
    ts = qt.TickState(z(torch.uint8), z(torch.int32), z(torch.int32), z(torch.int32))
    groups_ = qf.FollowerGroups(G, 10, True, True, {k: z(torch.int64) for k in qf._U64_FIELDS}, ts)
    log = qf.FollowerLog(G, z(torch.int32), z(torch.int64), z(torch.int64, 8 * G),
                         z(torch.int64, 8 * G))
    ready = qy.ReadyState(G, {k: z(torch.int64) for k in ("unstable_offset", "usnap_index",
                                                          "usnap_term")})
    return groups_, log, ready, z(torch.int64)


def _inbox(groups_):
    n = len(groups_)
    z = np.zeros(n, np.uint64)
    return qs.SnapshotInbox.from_numpy(np.array(groups_, np.uint32), z, z, z, z,
                                       [{"voters": [1, 2, 3]}] * n, device="cpu")


def test_wrapper_refuses_duplicate_groups_before_the_call():
    g, log, ready, sid = _host_state()
    with pytest.raises(_lib.QuorumBatchError, match="group 3 has more than one record"):
        qs.follower_snapshot(g, log, ready, sid, _inbox([1, 3, 5, 3]))
    # distinct groups (or the check switched off) get as far as the tensor checks
    for ib, kw in ((_inbox([1, 3, 5]), {}), (_inbox([1, 3, 3]), {"check_distinct": False})):
        with pytest.raises(_lib.QuorumBatchError, match="device tensor"):
            qs.follower_snapshot(g, log, ready, sid, ib, **kw)


def test_wrapper_checks_its_arguments():
    g, log, ready, sid = _host_state()
    ib = _inbox([0, 1])
    with pytest.raises(_lib.QuorumBatchError, match="self_id is missing"):
        qs.follower_snapshot(g, log, ready, None, ib)
    with pytest.raises(_lib.QuorumBatchError, match="the log has 4 groups"):
        qs.follower_snapshot(g, qf.FollowerLog(4, log.meta, log.first_index, log.run_start,
                                               log.run_term), ready, sid, ib)
    ready.t["usnap_term"] = None
    ib_dev = _inbox([0, 1])
    ib_dev.check = lambda: None
    with pytest.raises(_lib.QuorumBatchError, match="usnap_term is missing"):
        qs.follower_snapshot(g, log, ready, sid, ib_dev)
    with pytest.raises(_lib.QuorumBatchError, match="inbox term has 1 entries, group has 2"):
        qs.SnapshotInbox.from_numpy(np.zeros(2, np.uint32), np.zeros(2), np.zeros(1), np.zeros(2),
                                    np.zeros(2), [{}, {}], device="cpu")


def test_conf_states_pack_in_list_order():
    off, ids, sets = qs.pack_conf_states([
        {"voters": [2, 3], "learners_next": [1], "voters_outgoing": [1, 2], "auto_leave": True},
        {}, {"learners": [9]}])
    assert off.tolist() == [0, 5, 5, 6]
    assert ids.tolist() == [2, 3, 1, 2, 1, 9]
    assert sets.tolist() == [qs.CS_VOTERS, qs.CS_VOTERS, qs.CS_VOTERS_OUTGOING,
                             qs.CS_VOTERS_OUTGOING, qs.CS_LEARNERS_NEXT, qs.CS_LEARNERS]
    ib = _inbox([4, 2, 7])
    groups_, css = qs.restored_conf_states(ib, np.array([qs.SNF_RESTORED, qs.SNF_OLD,
                                                         qs.SNF_RESTORED | qs.SNF_RESET], np.uint16))
    assert groups_.tolist() == [4, 7] and css == [{"voters": [1, 2, 3]}] * 2


def test_binding_layout_and_constants_match_header(tmp_path):
    """The three mirrors have the header's sizes and field offsets, and the
    module's constants the header's values (gcc on the header)."""
    structs = (("qb_snapshot_groups", qs.SnapshotGroupsC), ("qb_snapshot_inbox", qs.SnapshotInboxC),
               ("qb_snapshot_out", qs.SnapshotOutC))
    consts = [("QB_SSTAT_COUNT", len(qs.SSTAT_NAMES)), ("QB_FRESP_APP_RESP", qs.MSG_APP_RESP),
              ("QB_RDP_MSGS", qs.RDP_MSGS), ("QB_READY_MAX_GROUPS == 0xFFFFFFFEull", 1)]
    consts += [("QB_SNF_" + n, getattr(qs, "SNF_" + n)) for n in (
        "RESTORED", "FAST_FORWARD", "OLD", "NOT_MEMBER", "STALE", "ROLE_IGNORED", "RESET",
        "COMMIT_RANGE", "BAD_GROUP", "HARDSTATE")]
    consts += [("QB_CS_" + n, getattr(qs, "CS_" + n)) for n in (
        "VOTERS", "LEARNERS", "VOTERS_OUTGOING", "LEARNERS_NEXT")]
    consts += [("QB_SSTAT_" + n.upper(), i) for i, n in enumerate(qs.SSTAT_NAMES)]
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
    # the test restatement's names and values are the mirror's
    from tests import snapshot_ref as S
    assert S.SSTAT_NAMES == qs.SSTAT_NAMES and S.CS_LISTS == qs.CS_LISTS
    for n in ("RESTORED", "FAST_FORWARD", "OLD", "NOT_MEMBER", "STALE", "ROLE_IGNORED", "RESET",
              "COMMIT_RANGE", "BAD_GROUP", "HARDSTATE"):
        assert getattr(S, "SNF_" + n) == getattr(qs, "SNF_" + n)
