"""qb_dev_follower_log_step's host-side argument checks: every refusal by
return code and error text, with no GPU (the checks run before any HIP call),
the binding's structs against the header's layout, the workspace size against
its formula, and the Python mirror's tensor and run-table checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from etcd_amd import _lib
from etcd_amd.quorum import follower as qf
from etcd_amd.quorum.follower import (FLSTAT_NAMES, FollowerAppInboxC, FollowerAppOutC,
                                      FollowerGroupsC, FollowerInboxC, FollowerLogC)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 0x1000   # a non-NULL pointer; never dereferenced: each check fails first
D2 = 0x2000
GROUP_PTRS = ("term", "vote", "lead", "committed", "last_index", "last_term", "role",
              "election_elapsed", "heartbeat_elapsed")
LOG_PTRS = ("meta", "first_index", "last_index", "last_term", "run_start", "run_term")
INBOX_PTRS = ("group", "flags", "from", "term", "index", "aux")
APP_PTRS = ("commit", "ent_off", "ent_term", "ent_len")
APP_OUT = ("resp_index", "resp_hint", "resp_log_term", "app_from")
OUTPUTS = ("resp_type", "resp_term", "stop_at", "gflags", "stats")


def groups(**kw):
    f = dict(G=16, election_timeout=10, check_quorum=1, pre_vote=1, reserved=0)
    f.update({p: D for p in GROUP_PTRS})
    f.update(kw)
    return FollowerGroupsC(**f)


def log(**kw):
    f = {p: D for p in LOG_PTRS}
    f.update(kw)
    return FollowerLogC(**f)


def inbox(M=32, **kw):
    f = {p: D for p in INBOX_PTRS}
    f.update(kw)
    ib = FollowerInboxC(M=M)
    for k, v in f.items():
        setattr(ib, k, v)
    return ib


def app(E=8, **kw):
    f = {p: D for p in APP_PTRS}
    f.update(kw)
    return FollowerAppInboxC(E=E, **f)


def app_out(**kw):
    f = {p: D for p in APP_OUT}
    f.update(kw)
    return FollowerAppOutC(**f)


def ref(x):
    return C.byref(x) if x is not None else None


def step(fg, lg, ib, ap, ao, ws=D, ws_bytes=1 << 40, **out):
    lib = _lib.load()
    o = {k: D for k in OUTPUTS}
    o.update(out)
    rc = lib.qb_dev_follower_log_step(ref(fg), ref(lg), ref(ib), ref(ap), o["resp_type"],
                                      o["resp_term"], ref(ao), o["stop_at"], o["gflags"],
                                      o["stats"], ws, C.c_size_t(ws_bytes), None)
    return rc, lib.qb_last_error()


def ok_args():
    return [groups(), log(), inbox(), app(), app_out()]


@pytest.mark.parametrize("k,name", enumerate(("fg", "lg", "in", "app", "out")))
def test_null_structs_are_einval(k, name):
    a = ok_args()
    a[k] = None
    rc, err = step(*a)
    assert rc == _lib.QB_EINVAL and f"qb_dev_follower_log_step: {name} is NULL".encode() in err


@pytest.mark.parametrize("name", GROUP_PTRS)
def test_null_group_pointer_is_einval(name):
    rc, err = step(groups(**{name: None}), log(), inbox(), app(), app_out())
    assert rc == _lib.QB_EINVAL and b"group pointer is NULL" in err


@pytest.mark.parametrize("name", LOG_PTRS)
def test_null_log_pointer_is_einval(name):
    rc, err = step(groups(), log(**{name: None}), inbox(), app(), app_out())
    assert rc == _lib.QB_EINVAL and b"log pointer is NULL" in err


@pytest.mark.parametrize("name", ("last_index", "last_term"))
def test_log_must_share_the_groups_last_index_and_term(name):
    rc, err = step(groups(), log(**{name: D2}), inbox(), app(), app_out())
    assert rc == _lib.QB_EINVAL and f"lg->{name} != fg->{name}".encode() in err


@pytest.mark.parametrize("name", INBOX_PTRS)
def test_null_inbox_pointer_is_einval(name):
    rc, err = step(groups(), log(), inbox(**{name: None}), app(), app_out())
    assert rc == _lib.QB_EINVAL and b"required inbox pointer is NULL" in err


@pytest.mark.parametrize("name", APP_PTRS)
def test_null_app_inbox_pointer_is_einval(name):
    rc, err = step(groups(), log(), inbox(), app(**{name: None}), app_out())
    assert rc == _lib.QB_EINVAL and b"append-inbox pointer is NULL" in err


@pytest.mark.parametrize("name", OUTPUTS)
def test_null_output_pointer_is_einval(name):
    rc, err = step(*ok_args(), **{name: None})
    assert rc == _lib.QB_EINVAL and b"required output pointer is NULL" in err


@pytest.mark.parametrize("name", APP_OUT)
def test_null_app_output_pointer_is_einval(name):
    rc, err = step(groups(), log(), inbox(), app(), app_out(**{name: None}))
    assert rc == _lib.QB_EINVAL and b"append-output pointer is NULL" in err


def test_config_refusals():
    rc, err = step(groups(election_timeout=0), log(), inbox(), app(), app_out())
    assert rc == _lib.QB_EINVAL and b"election_timeout must be >= 1" in err
    for name in ("check_quorum", "pre_vote"):
        rc, err = step(groups(**{name: 2}), log(), inbox(), app(), app_out())
        assert rc == _lib.QB_EINVAL and f"{name} must be 0 or 1".encode() in err


def test_record_count_bound():
    assert qf.follower_log_workspace_bytes(16, (1 << 32) - 2) > 0
    for G, M in ((16, (1 << 32) - 1), (1 << 32, 1)):
        with pytest.raises(_lib.QuorumBatchError, match="no follower-log-step workspace"):
            qf.follower_log_workspace_bytes(G, M)
    rc, err = step(groups(), log(), inbox(M=(1 << 32) - 1), app(), app_out())
    assert rc == _lib.QB_EINVAL and b"M 4294967295 > 2^32 - 2" in err


def test_workspace_is_required_sized_and_aligned():
    need = qf.follower_log_workspace_bytes(16, 32)
    rc, err = step(*ok_args(), ws=None)
    assert rc == _lib.QB_EINVAL and b"workspace is NULL" in err
    rc, err = step(*ok_args(), ws_bytes=need - 1)
    assert rc == _lib.QB_EINVAL and b"workspace too small" in err
    assert b"(qb_follower_workspace_bytes)" in err     # the size function to ask
    rc, err = step(*ok_args(), ws=D + 4)
    assert rc == _lib.QB_EINVAL and b"workspace must be 8-byte aligned" in err


def up256(x):
    return (x + 255) & ~255


@pytest.mark.parametrize("G", (0, 1, 513, 4097))
@pytest.mark.parametrize("M", (0, 1, 513, 4097))
def test_workspace_size_is_the_formula(G, M):
    """cnt [G + 1] u32 | 256 | the scan's block sums (one u32 per 4096
    counters, + 1) | the long-run list [M / 17 + 1] u32 | perm [max(M, 1)]
    u32, each rounded up to 256 bytes: the follower step's own workspace,
    which is the size function the C call names (there is no second one)."""
    lib = _lib.load()
    scan_blocks = (G + 4095) // 4096
    want = (up256(4 * (G + 1)) + 256 + up256(4 * (scan_blocks + 1)) + up256(4 * (M // 17 + 1)) +
            up256(4 * max(M, 1)))
    assert qf.follower_log_workspace_bytes(G, M) == want
    assert lib.qb_follower_workspace_bytes(G, M) == want
    assert not hasattr(lib, "qb_follower_log_workspace_bytes")


def test_no_groups_or_no_records_is_ok():
    """G == 0 returns QB_OK before any pointer is looked at."""
    fg = groups(G=0, **{p: None for p in GROUP_PTRS})
    rc, _ = step(fg, log(**{p: None for p in LOG_PTRS}), inbox(**{p: None for p in INBOX_PTRS}),
                 app(**{p: None for p in APP_PTRS}), app_out(**{p: None for p in APP_OUT}),
                 ws=None, ws_bytes=0, **{k: None for k in OUTPUTS})
    assert rc == _lib.QB_OK


def test_abi_version_stays_and_the_new_kind_follows_host():
    lib = _lib.load()
    assert lib.qb_abi_version() == 1
    assert qf.FIN_APP == 5 and qf.FIN_HOST == 4


def test_binding_layout_matches_header(tmp_path):
    """The four structs have the header's sizes and field offsets (gcc on the
    header), and the mirror's constants its values."""
    structs = (("qb_follower_log", FollowerLogC, LOG_PTRS),
               ("qb_follower_app_inbox", FollowerAppInboxC, APP_PTRS + ("E",)),
               ("qb_follower_app_out", FollowerAppOutC, APP_OUT))
    args, want = [], []
    for cname, cls, names in structs:
        args.append(f"sizeof({cname})")
        want.append(C.sizeof(cls))
        for n in names:
            args.append(f"offsetof({cname}, {n})")
            want.append(getattr(cls, n).offset)
    fmt = " ".join(["%zu"] * len(args))
    consts = (f"QB_FLSTAT_COUNT == {len(FLSTAT_NAMES)} && QB_FIN_APP == {qf.FIN_APP} && "
              f"QB_FFLAG_LOG_CONFLICT == {qf.FFLAG_LOG_CONFLICT} && "
              f"QB_FFLAG_LOG_RUNS == {qf.FFLAG_LOG_RUNS} && QB_FFLAG_APPENDED == {qf.FFLAG_APPENDED} && "
              f"QB_LEADER_MAX_RUNS == {qf.MAX_RUNS} && QB_FSTAT_COUNT == 11 && "
              + " && ".join(f"QB_FLSTAT_{n.upper()} == {i}"
                            for i, n in enumerate(FLSTAT_NAMES) if i >= 11))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quorum_batch.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", {", ".join(args)}); '
                   f'return {consts} ? 0 : 1; }}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert got == want


def _cpu_args(G=4, M=4, E=2):
    import torch
    from etcd_amd.quorum import tick as qt
    z32 = torch.zeros(max(G, M + 1), dtype=torch.int32)
    z64 = torch.zeros(8 * G, dtype=torch.int64)
    st = qt.TickState(torch.zeros(G, dtype=torch.uint8), z32, z32, z32)
    fg = qf.FollowerGroups(G, 10, True, True, {k: z64 for k in qf._U64_FIELDS}, st)
    lg = qf.FollowerLog(G, z32, z64, z64, z64)
    ib = qf.FollowerInbox(z32, torch.zeros(M, dtype=torch.uint8), z64, z64, z64, z64)
    ib._m = M
    ap = qf.FollowerAppInbox(z64, z32, z64, z32, E)
    return fg, lg, ib, ap


def test_python_mirror_refuses_bad_tensors():
    import torch
    fg, lg, ib, ap = _cpu_args()
    with pytest.raises(_lib.QuorumBatchError, match="device tensor"):
        qf.follower_log_step(fg, lg, ib, ap)
    ib._m = 1 << 32
    with pytest.raises(_lib.QuorumBatchError, match="2\\^32 - 2"):
        qf.follower_log_step(fg, lg, ib, ap)
    ib._m = 4
    lg.G = 5
    with pytest.raises(_lib.QuorumBatchError, match="the log has 5 groups"):
        qf.follower_log_step(fg, lg, ib, ap)
    lg.G = 4
    fg.election_timeout = 0
    with pytest.raises(_lib.QuorumBatchError, match="election_timeout"):
        qf.follower_log_step(fg, lg, ib, ap)
    with pytest.raises(_lib.QuorumBatchError, match="ent_off has 4 entries, not M \\+ 1 = 5"):
        qf.FollowerAppInbox.from_numpy(np.zeros(4), np.zeros(4), np.zeros(2), np.zeros(2), "cpu")
    with pytest.raises(_lib.QuorumBatchError, match="ent_term has 3 entries, ent_len 2"):
        qf.FollowerAppInbox.from_numpy(np.zeros(4), np.zeros(5), np.zeros(3), np.zeros(2), "cpu")
    assert torch.zeros(1).device.type == "cpu"


def good_table():
    """Two groups: log [dummy t0 | 1 1 2] at first_index 1, and [dummy t3 | 3 5] at 10."""
    rs = np.zeros((8, 2), np.uint64)
    rt = np.zeros((8, 2), np.uint64)
    rs[:3, 0], rt[:3, 0] = [0, 1, 3], [0, 1, 2]
    rs[:2, 1], rt[:2, 1] = [9, 11], [3, 5]
    return dict(meta=np.array([3 << 16, 2 << 16 | 0x07], np.uint32),
                first_index=np.array([1, 10], np.uint64), run_start=rs, run_term=rt,
                last_index=np.array([3, 11], np.uint64), last_term=np.array([2, 5], np.uint64),
                committed=np.array([0, 9], np.uint64))


def test_run_table_check_accepts_a_good_table():
    qf.check_run_table(**good_table())


@pytest.mark.parametrize("what,edit", [
    ("run count", lambda t: t["meta"].__setitem__(0, 0)),
    ("run count", lambda t: t["meta"].__setitem__(1, 9 << 16)),
    ("first_index must be >= 1", lambda t: t["first_index"].__setitem__(0, 0)),
    ("run 0 must start at first_index - 1", lambda t: t["run_start"].__setitem__((0, 1), 10)),
    ("committed is below", lambda t: t["committed"].__setitem__(1, 8)),
    ("run 2 does not start behind run 1", lambda t: t["run_start"].__setitem__((2, 0), 1)),
    ("run 1 has the term of run 0", lambda t: t["run_term"].__setitem__((1, 1), 3)),
    ("a run starts behind last_index", lambda t: t["last_index"].__setitem__(0, 2)),
    ("the last run's term is not last_term", lambda t: t["last_term"].__setitem__(1, 4)),
])
def test_run_table_check_refuses(what, edit):
    t = good_table()
    edit(t)
    with pytest.raises(_lib.QuorumBatchError, match=what):
        qf.check_run_table(**t)


def test_from_numpy_checks_the_table():
    t = good_table()
    g = {k: t.pop(k) for k in ("last_index", "last_term", "committed")}
    lg = qf.FollowerLog.from_numpy(t["meta"], t["first_index"], t["run_start"], t["run_term"], g,
                                   "cpu")
    assert lg.G == 2 and lg.run_start.numel() == 16
    g["last_term"][0] = 7
    with pytest.raises(_lib.QuorumBatchError, match="group 0: the last run's term"):
        qf.FollowerLog.from_numpy(t["meta"], t["first_index"], t["run_start"], t["run_term"], g,
                                  "cpu")
    with pytest.raises(_lib.QuorumBatchError, match="run_start has 8 entries, not 16"):
        qf.FollowerLog.from_numpy(t["meta"], t["first_index"], t["run_start"][:4], t["run_term"],
                                  g, "cpu")
