"""qb_dev_switch_config's refusals, before any device work: the C entry's
(NULL pointers, inflight_cap, readq_cap) and the wrapper's (device, dtype,
contiguity and length of every tensor), the struct mirrors' sizes against the
header, and G == 0.  No GPU."""
import ctypes as C
import os
import subprocess
import types

import pytest
import torch

from etcd_amd import _lib
from etcd_amd.quorum import confchange as qcc, switch as qs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 0x1000  # never dereferenced: each check fails first


def groups(**kw):
    sg = qs.SwitchGroupsC(G=4, inflight_cap=2, readq_cap=0)
    for n in qs._POINTERS:
        setattr(sg, n, D)
    for k, v in kw.items():
        setattr(sg, k, v)
    return sg


def outs(**kw):
    so = qs.SwitchOutC(**{n: D for n in qs._OUT_POINTERS})
    for k, v in kw.items():
        setattr(so, k, v)
    return so


def call(sg, action=D, so=None, stats=D):
    lib = _lib.load()
    rc = lib.qb_dev_switch_config(C.byref(sg) if sg is not None else None, action,
                                  C.byref(so) if so is not None else None, stats, None)
    return rc, lib.qb_last_error()


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "quorum_batch.h")).read()
    for name, v in (("QB_SW_NONE", qs.SW_NONE), ("QB_SW_SWITCH", qs.SW_SWITCH),
                    ("QB_SW_RESTORE", qs.SW_RESTORE), ("QB_SWFLAG_SWITCHED", qs.SWFLAG_SWITCHED),
                    ("QB_SWFLAG_COMMITTED", qs.SWFLAG_COMMITTED), ("QB_SWFLAG_SENT", qs.SWFLAG_SENT),
                    ("QB_SWFLAG_TRANSFER_ABORTED", qs.SWFLAG_TRANSFER_ABORTED),
                    ("QB_SWFLAG_SELF_REMOVED", qs.SWFLAG_SELF_REMOVED),
                    ("QB_SWFLAG_SELF_LEARNER", qs.SWFLAG_SELF_LEARNER),
                    ("QB_SWFLAG_VOTE_DROPPED", qs.SWFLAG_VOTE_DROPPED),
                    ("QB_SWFLAG_HOST", qs.SWFLAG_HOST)):
        import re
        m = re.search(rf"#define {name} (0x[0-9A-Fa-f]+|\d+)u?\b", text)
        assert m and int(m.group(1), 0) == v, name
    assert f"QB_SWSTAT_COUNT = {len(qs.SWSTAT_NAMES)}" in text
    for i, n in enumerate(qs.SWSTAT_NAMES):
        assert f"QB_SWSTAT_{n.upper()} = {i}," in text, n


def test_struct_mirrors_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quorum_batch.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(qb_switch_groups), '
                   'offsetof(qb_switch_groups, old_off), offsetof(qb_switch_groups, rq_meta), '
                   'offsetof(qb_switch_groups, infl_buf), sizeof(qb_switch_out), '
                   'offsetof(qb_switch_out, msg_n)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert got == [C.sizeof(qs.SwitchGroupsC), qs.SwitchGroupsC.old_off.offset,
                   qs.SwitchGroupsC.rq_meta.offset, qs.SwitchGroupsC.infl_buf.offset,
                   C.sizeof(qs.SwitchOutC), qs.SwitchOutC.msg_n.offset]


def test_c_entry_refusals():
    cases = [(lambda: call(None, so=outs()), b"sg is NULL"),
             (lambda: call(groups(), so=None), b"out is NULL"),
             (lambda: call(groups(inflight_cap=0), so=outs()), b"inflight_cap must be 1..4096"),
             (lambda: call(groups(inflight_cap=4097), so=outs()), b"inflight_cap must be 1..4096"),
             (lambda: call(groups(readq_cap=17), so=outs()), b"readq_cap must be 0..16"),
             (lambda: call(groups(readq_cap=1, rq_meta=None), so=outs()), b"rq_meta is NULL"),
             (lambda: call(groups(), action=None, so=outs()), b"action is NULL"),
             (lambda: call(groups(), so=outs(), stats=None), b"required output pointer")]
    for n in qs._POINTERS:
        if n not in ("votes", "rq_meta"):
            cases.append((lambda n=n: call(groups(**{n: None}), so=outs()),
                          b"required group pointer"))
    for n in qs._OUT_POINTERS:
        if n != "slot_map":
            cases.append((lambda n=n: call(groups(), so=outs(**{n: None})),
                          b"required output pointer"))
    for fn, why in cases:
        rc, err = fn()
        assert rc == _lib.QB_EINVAL and why in err, (why, rc, err)


def test_no_groups_is_ok_and_touches_nothing():
    sg = groups(G=0)
    for n in qs._POINTERS:
        setattr(sg, n, None)
    rc, _ = call(sg, action=None, so=qs.SwitchOutC(), stats=None)
    assert rc == _lib.QB_OK


def test_wrapper_refuses_host_tensors_and_bad_shapes():
    """The wrapper checks every tensor before the C call: with host tensors
    it must raise QuorumBatchError, never reach the library."""
    G, S = 2, 4
    i64 = lambda n: torch.zeros(n, dtype=torch.int64)  # noqa: E731
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)  # noqa: E731
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8)  # noqa: E731
    t = {"off": i32(G + 1), "cfg": i32(G), "meta": i32(G), "term": i64(G), "committed": i64(G),
         "first_index": i64(G), "last_index": i64(G), "snap_index": i64(G), "snap_term": i64(G),
         "max_ents": i64(G), "run_start": i64(8 * G), "run_term": i64(8 * G), "rq_meta": i32(1)}
    lg = types.SimpleNamespace(G=G, S=S, device=torch.device("cpu"), t=t, inflight_cap=2,
                               readq_cap=0)
    ft = {"term": t["term"], "committed": t["committed"], "last_index": t["last_index"],
          "last_term": i64(G)}
    fg = types.SimpleNamespace(G=G, state=types.SimpleNamespace(role=u8(G)), t=ft)
    es = types.SimpleNamespace(follower=fg, self_id=i64(G), votes=i32(G))
    old = qcc.ConfigTable(G, S, 2, {"off": i32(G + 1), "ids": i64(S)})
    nt = {"off": i32(G + 1), "cfg": i32(G), "ids": i64(S), "match": i64(S), "next": i64(S),
          "pending_snapshot": i64(S), "pstate": u8(S), "infl_pos": i32(S), "infl_buf": i64(2 * S)}
    new = qcc.ConfigTable(G, S, 2, nt)
    out = qs.SwitchResult(u8(G), u8(S), u8(S), i64(S), i64(S), i64(S), i64(len(qs.SWSTAT_NAMES)))
    with pytest.raises(_lib.QuorumBatchError, match="device tensor"):
        qs.switch_config(lg, es, old, new, u8(G), out=out)
    lg.inflight_cap = 0
    with pytest.raises(_lib.QuorumBatchError, match="inflight_cap"):
        qs.switch_config(lg, es, old, new, u8(G), out=out)
    lg.inflight_cap, lg.readq_cap = 2, 17
    with pytest.raises(_lib.QuorumBatchError, match="readq_cap"):
        qs.switch_config(lg, es, old, new, u8(G), out=out)
    lg.readq_cap = 0
    with pytest.raises(_lib.QuorumBatchError, match="groups"):
        qs.switch_config(lg, es, qcc.ConfigTable(G + 1, S, 2, old.t), new, u8(G), out=out)
    with pytest.raises(_lib.QuorumBatchError, match="rings"):
        qs.switch_config(lg, es, old, qcc.ConfigTable(G, S, 4, nt), u8(G), out=out)
