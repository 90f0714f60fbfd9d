"""qb_dev_ingest_follower: the symbol, every host-side refusal (no GPU
needed), the constants against the header, the ctypes struct mirror against
the header's layout and the workspace size."""
import ctypes as C
import os
import re
import subprocess

import pytest

from etcd_amd import _lib
from etcd_amd.quorum import follower, wire
from tests import follower_wire_ref as FW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "quorum_batch.h")
D = C.c_void_p(0x1000)  # never dereferenced: each check fails first
BIG = C.c_size_t(1 << 40)
REQUIRED = ("group", "flags", "from", "term", "index", "aux", "commit", "status")
NULLABLE = ("msg_type", "ent_pos", "ent_bytes", "ent_n", "stats")


def _out(**kw):
    f = {k: D for k in REQUIRED + NULLABLE + ("ent_off", "ent_term", "ent_len", "ent_total")}
    f["ent_cap"] = 64
    f.update(kw)
    return wire.FollowerWireOutC(**f)


def _call(M=8, bytes_=D, nbytes=100, msg_off=D, msg_group=D, G=4, out=None, ws=D, ws_bytes=BIG):
    lib = _lib.load()
    o = _out() if out is None else out
    return lib.qb_dev_ingest_follower(M, bytes_, nbytes, msg_off, msg_group, G,
                                      None if o is False else C.byref(o), ws, ws_bytes, None)


def _refused(rc, why):
    lib = _lib.load()
    assert rc == _lib.QB_EINVAL, (why, rc)
    assert why in lib.qb_last_error(), (why, lib.qb_last_error())


def _define(name):
    return int(re.search(rf"#define {name} (\d+)", open(HEADER).read()).group(1))


def test_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in ("qb_dev_ingest_follower", "qb_wire_follower_scratch_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES


def test_status_constants_match_the_header():
    names = ("OK", "UNMARSHAL", "TYPE", "CTX", "ENTRIES", "NO_SPACE")
    for k, name in enumerate(names):
        assert _define(f"QB_WIRE_{name}") == k == getattr(wire, f"WIRE_{name}") == getattr(FW, name)
    assert _define("QB_WIRE_FOLLOWER_STATUS_COUNT") == len(names) == FW.STATUS_COUNT
    assert len(wire.WIRE_FOLLOWER_STAT_NAMES) == len(names)
    for name in ("HEARTBEAT", "VOTE", "PREVOTE", "TIMEOUT_NOW", "HOST", "APP"):
        assert _define(f"QB_FIN_{name}") == getattr(FW, f"FIN_{name}")
    assert FW.FORCE == follower.FREC_FORCE and follower.FIN_APP == FW.FIN_APP


def test_workspace_size_is_monotone_and_bounded():
    lib = _lib.load()
    f = lib.qb_wire_follower_scratch_bytes
    sizes = [f(M) for M in (0, 1, 255, 256, 257, 4096, 4097, 1 << 20, 1 << 24, (1 << 32) - 2)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] > 0
    # the entry ranges (12 bytes a message) and the scan's block sums
    assert f(1 << 24) >= 12 << 24
    assert f((1 << 32) - 1) == 0 and f(1 << 40) == 0


def test_refusals_before_any_launch():
    _refused(_call(out=False), b"out is NULL")
    for k in ("ent_off", "ent_total"):
        _refused(_call(out=_out(**{k: None})), b"ent_off / ent_total")
        # nothing to decode still needs somewhere to say so
        _refused(_call(M=0, out=_out(**{k: None})), b"ent_off / ent_total")
    _refused(_call(msg_off=None), b"msg_off / msg_group")
    _refused(_call(msg_group=None), b"msg_off / msg_group")
    _refused(_call(bytes_=None), b"bytes is NULL")
    for k in REQUIRED:
        _refused(_call(out=_out(**{k: None})), b"are required")
    for k in ("ent_term", "ent_len"):
        _refused(_call(out=_out(**{k: None})), b"ent_term / ent_len")
    _refused(_call(ws=None), b"workspace too small")
    need = _lib.load().qb_wire_follower_scratch_bytes(8)
    _refused(_call(ws_bytes=C.c_size_t(need - 1)), b"workspace too small")
    _refused(_call(M=(1 << 32) - 1), b"pass 2^32 - 2")
    _refused(_call(nbytes=1 << 32), b"bytes pass 2^32")


def test_what_may_be_null():
    """Every nullable column NULL, bytes NULL with no bytes, the runs' arrays
    NULL with ent_cap 0: the refusal then is the next check's."""
    o = _out(ent_term=None, ent_len=None, ent_cap=0, **{k: None for k in NULLABLE})
    _refused(_call(bytes_=None, nbytes=0, out=o, ws_bytes=C.c_size_t(8)), b"workspace too small")


def test_struct_mirror_matches_header(tmp_path):
    cls, name = wire.FollowerWireOutC, "qb_follower_wire_out"
    lines = [f'printf("%zu\\n", sizeof({name}));']
    want = [C.sizeof(cls)]
    for fname, _ in cls._fields_:
        lines.append(f'printf("%zu\\n", offsetof({name}, {fname}));')
        want.append(getattr(cls, fname).offset)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quorum_batch.h"\n'
                   "int main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in got] == want


def test_wrapper_refuses_host_tensors_and_bad_sizes():
    import torch
    z8 = torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(_lib.QuorumBatchError, match="device tensor"):
        wire.ingest_follower(z8, 16, torch.zeros(3, dtype=torch.int64),
                             torch.zeros(2, dtype=torch.int32), 4)
    with pytest.raises(_lib.QuorumBatchError, match="nbytes"):
        wire.ingest_follower(z8, -1, torch.zeros(3, dtype=torch.int64),
                             torch.zeros(2, dtype=torch.int32), 4)
