"""qb_dev_ingest_requests: the symbols, every host-side refusal (no GPU
needed), the constants against the header, the ctypes struct mirror against
the header's layout and the workspace size."""
import ctypes as C
import os
import re
import subprocess

import pytest

from etcd_amd import _lib
from etcd_amd.quorum import propose, request, wire
from tests import request_wire_ref as RW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "quorum_batch.h")
D = C.c_void_p(0x1000)  # never dereferenced: each check fails first
BIG = C.c_size_t(1 << 40)
MSG = tuple(n for n, _ in wire._RW_MSG)
DENSE = tuple(n for n, _, _ in wire._RW_DENSE)


def _out(**kw):
    f = {k: D for k in MSG + DENSE + ("stats",)}
    f.update(kw)
    return wire.RequestWireOutC(**f)


def _call(M=8, bytes_=D, nbytes=100, msg_off=D, msg_group=D, G=4, off=D, ids=D, max_reads=1, concat=0,
          out=None, ws=D, ws_bytes=BIG):
    lib = _lib.load()
    o = _out() if out is None else out
    return lib.qb_dev_ingest_requests(M, bytes_, nbytes, msg_off, msg_group, G, off, ids, max_reads,
                                      concat, None if o is False else C.byref(o), ws, ws_bytes, None)


def _refused(rc, why):
    lib = _lib.load()
    assert rc == _lib.QB_EINVAL, (why, rc)
    assert why in lib.qb_last_error(), (why, lib.qb_last_error())


def _define(name):
    return int(re.search(rf"#define {name} (\w+)", open(HEADER).read()).group(1).rstrip("u"), 0)


def _enum(name):
    return int(re.search(rf"\b{name} = (\d+)", open(HEADER).read()).group(1))


def test_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in ("qb_dev_ingest_requests", "qb_wire_requests_scratch_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    from etcd_amd import quorum
    assert quorum.ingest_requests is wire.ingest_requests and "ingest_requests" in quorum.__all__


def test_constants_match_the_header():
    names = ("OK", "UNMARSHAL", "TYPE", "CTX", "ENTRIES", "NO_SPACE", "TERM", "CONF_CHANGE", "GROUP",
             "DEFERRED")
    for k, name in enumerate(names):
        assert _define(f"QB_WIRE_{name}") == k == getattr(wire, f"WIRE_{name}") == getattr(RW, name)
    for k, name in enumerate(("NONE", "PROP", "READ", "TRANSFER", "READ_RESP")):
        assert _define(f"QB_RQ_{name}") == k == getattr(wire, f"RQ_{name}") == getattr(RW, f"RQ_{name}")
    for k, name in enumerate(("TAKEN_PROPS", "TAKEN_READS", "TAKEN_TRANSFERS", "READ_RESPS",
                              "ENTRIES_TAKEN")):
        assert _enum(f"QB_RWSTAT_{name}") == 10 + k == getattr(RW, f"STAT_{name}")
        assert wire.WIRE_REQUEST_STAT_NAMES[10 + k] == name.lower()
    assert _enum("QB_RWSTAT_COUNT") == RW.STAT_COUNT == len(wire.WIRE_REQUEST_STAT_NAMES)
    assert _define("QB_RWFLAG_TAKEN") == RW.FLAG_TAKEN == wire.RWFLAG_TAKEN
    assert _define("QB_RWFLAG_DEFERRED") == RW.FLAG_DEFERRED == wire.RWFLAG_DEFERRED
    assert (RW.PROP_ENTRIES, RW.PROP_CONF_CHANGE, RW.PROP_CC_LEAVE_JOINT) == \
        (propose.PROP_ENTRIES, propose.PROP_CONF_CHANGE, propose.PROP_CC_LEAVE_JOINT)
    assert RW.SLOT_LOCAL == request.NO_SLOT == wire.SLOT_LOCAL and RW.MAX_SLOTS == _lib.QB_MAX_SLOTS
    assert RW.NO_CC == wire.NO_CONF_CHANGE and _define("QB_ABI_VERSION") == 1


def test_workspace_size_is_monotone_and_bounded():
    f = _lib.load().qb_wire_requests_scratch_bytes
    sizes = (0, 1, 16, 17, 255, 256, 257, 4096, 4097, 1 << 20, 1 << 24, (1 << 32) - 2)
    for fixed in (0, 1, 1 << 20):
        by_m = [f(fixed, M) for M in sizes]
        by_g = [f(G, fixed) for G in sizes]
        assert all(a <= b for a, b in zip(by_m, by_m[1:])) and by_m[0] > 0
        assert all(a <= b for a, b in zip(by_g, by_g[1:])) and by_g[0] > 0
    # the counts (4 bytes a group) and the grouped batch indices (4 bytes a message)
    assert f(1 << 24, 1 << 24) >= 8 << 24
    for big in ((1 << 32) - 1, 1 << 40):
        assert f(big, 1) == 0 and f(1, big) == 0


def test_refusals_before_any_launch():
    _refused(_call(out=False), b"out is NULL")
    for r in (0, 17, 1 << 31):
        _refused(_call(max_reads=r), b"max_reads")
    _refused(_call(off=None), b"off / ids")
    _refused(_call(ids=None), b"off / ids")
    for k in DENSE:
        _refused(_call(out=_out(**{k: None})), b"a dense output")
        _refused(_call(M=0, out=_out(**{k: None})), b"a dense output")  # no messages still writes them
    _refused(_call(msg_off=None), b"msg_off / msg_group")
    _refused(_call(msg_group=None), b"msg_off / msg_group")
    _refused(_call(bytes_=None), b"bytes is NULL")
    for k in MSG:
        _refused(_call(out=_out(**{k: None})), b"a message column")
    _refused(_call(M=(1 << 32) - 1), b"messages pass 2^32 - 2")
    _refused(_call(G=(1 << 32) - 1), b"groups pass 2^32 - 2")
    _refused(_call(nbytes=1 << 32), b"bytes pass 2^32")
    _refused(_call(ws=None), b"workspace too small")
    need = _lib.load().qb_wire_requests_scratch_bytes(4, 8)
    _refused(_call(ws_bytes=C.c_size_t(need - 1)), b"workspace too small")


def test_what_may_be_null_and_no_groups():
    """stats NULL, bytes NULL with no bytes, every message column NULL with
    no messages: the refusal then is the next check's.  G == 0 is QB_OK before
    anything is looked at but out and max_reads."""
    o = _out(stats=None)
    _refused(_call(bytes_=None, nbytes=0, out=o, ws_bytes=C.c_size_t(8)), b"workspace too small")
    o = _out(stats=None, **{k: None for k in MSG})
    _refused(_call(M=0, msg_off=None, msg_group=None, bytes_=None, out=o, ws_bytes=C.c_size_t(8)),
             b"workspace too small")
    assert _call(G=0, off=None, ids=None, ws=None, out=_out(**{k: None for k in MSG + DENSE})) == _lib.QB_OK
    _refused(_call(G=0, max_reads=0), b"max_reads")


def test_struct_mirror_matches_header(tmp_path):
    cls, name = wire.RequestWireOutC, "qb_request_wire_out"
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


def test_wrapper_refuses_host_tensors_and_bad_arguments():
    import torch
    z8 = torch.zeros(16, dtype=torch.uint8)
    args = (torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32),
            torch.zeros(5, dtype=torch.int32), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(_lib.QuorumBatchError, match="device tensor"):
        wire.ingest_requests(z8, 16, *args)
    with pytest.raises(_lib.QuorumBatchError, match="nbytes"):
        wire.ingest_requests(z8, -1, *args)
