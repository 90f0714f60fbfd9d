"""qb_dev_encode_*: every host-side refusal (no GPU needed), the ctypes struct
mirrors against the header's layout, and the sizes of nothing."""
import ctypes as C
import os
import subprocess

import pytest

from etcd_amd import _lib
from etcd_amd.quorum import encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = C.c_void_p(0x1000)  # never dereferenced: each check fails first
BIG = C.c_size_t(1 << 40)
LIMIT = -(-(1 << 32) // encode.ENC_MAX_BYTES)  # the first M the 32-bit scan cannot hold


def _out(**kw):
    f = dict(bytes=D, cap=64, msg_off=D, status=D, ent_at=None, nbytes=D, stats=None)
    f.update(kw)
    return encode.EncodeOutC(**f)


def _groups(G=4, **kw):
    f = dict(G=G, off=D, ids=D, self_id=D, term=D)
    f.update(kw)
    return encode.EncodeGroupsC(**f)


def _cols():
    return encode.EncodeColsC(type=D)


def _slot_cols(S=8):
    return encode.EncodeSlotColsC(S=S, type_all=8, gmask=0xFF)


def _refused(rc, why):
    lib = _lib.load()
    assert rc == _lib.QB_EINVAL, (why, rc)
    assert why in lib.qb_last_error(), (why, lib.qb_last_error())


def test_workspace_sizes():
    lib = _lib.load()
    assert lib.qb_encode_scratch_bytes(1) > 0
    # lengths + total, the scan's sums and the slot groups: 8 bytes a message
    assert lib.qb_encode_scratch_bytes(1 << 24) >= 8 << 24
    assert lib.qb_encode_scratch_bytes(LIMIT - 1) > 0
    assert lib.qb_encode_scratch_bytes(LIMIT) == 0
    assert lib.qb_encode_scratch_bytes(1 << 40) == 0
    assert (LIMIT - 1) * encode.ENC_MAX_BYTES < 1 << 32 <= LIMIT * encode.ENC_MAX_BYTES


def test_encode_messages_refusals():
    lib = _lib.load()
    f = lib.qb_dev_encode_messages
    c, o = _cols(), _out()
    _refused(f(8, C.byref(c), None, D, BIG, None), b"out is NULL")
    _refused(f(8, None, C.byref(o), D, BIG, None), b"c / c->type is NULL")
    _refused(f(8, C.byref(encode.EncodeColsC()), C.byref(o), D, BIG, None), b"c / c->type is NULL")
    for k in ("msg_off", "nbytes"):
        _refused(f(8, C.byref(c), C.byref(_out(**{k: None})), D, BIG, None), b"msg_off / nbytes")
    _refused(f(8, C.byref(c), C.byref(_out(status=None)), D, BIG, None), b"status is NULL")
    _refused(f(8, C.byref(c), C.byref(_out(bytes=None)), D, BIG, None), b"bytes is NULL")
    _refused(f(8, C.byref(c), C.byref(o), None, BIG, None), b"workspace too small")
    need = lib.qb_encode_scratch_bytes(8)
    _refused(f(8, C.byref(c), C.byref(o), D, C.c_size_t(need - 1), None), b"workspace too small")
    _refused(f(LIMIT, C.byref(c), C.byref(o), D, BIG, None), b"pass 2^32")
    # nothing to encode still needs somewhere to say so
    _refused(f(0, C.byref(c), C.byref(_out(nbytes=None)), None, 0, None), b"msg_off / nbytes")


def test_encode_msg_out_refusals():
    lib = _lib.load()
    f = lib.qb_dev_encode_msg_out
    g, o = _groups(), _out()
    _refused(f(None, D, 8, None, C.byref(o), D, BIG, None), b"eg is NULL")
    for k in ("off", "ids", "self_id", "term"):
        _refused(f(C.byref(_groups(**{k: None})), D, 8, None, C.byref(o), D, BIG, None),
                 b"required group pointer")
    _refused(f(C.byref(_groups(G=(1 << 32) - 1)), D, 8, None, C.byref(o), D, BIG, None), b"G ")
    _refused(f(C.byref(g), D, 8, None, None, D, BIG, None), b"out is NULL")
    _refused(f(C.byref(g), None, 8, None, C.byref(o), D, BIG, None), b"msgs is NULL")
    _refused(f(C.byref(g), D, 8, None, C.byref(_out(status=None)), D, BIG, None), b"status is NULL")
    _refused(f(C.byref(g), D, 8, None, C.byref(o), D, C.c_size_t(8), None), b"workspace too small")
    _refused(f(C.byref(g), D, LIMIT, None, C.byref(o), D, BIG, None), b"pass 2^32")


def test_encode_slots_refusals():
    lib = _lib.load()
    f = lib.qb_dev_encode_slots
    g, s, o = _groups(), _slot_cols(), _out()
    _refused(f(None, C.byref(s), C.byref(o), D, BIG, None), b"eg is NULL")
    _refused(f(C.byref(_groups(ids=None)), C.byref(s), C.byref(o), D, BIG, None),
             b"required group pointer")
    _refused(f(C.byref(g), None, C.byref(o), D, BIG, None), b"s is NULL")
    _refused(f(C.byref(g), C.byref(s), None, D, BIG, None), b"out is NULL")
    _refused(f(C.byref(g), C.byref(s), C.byref(_out(bytes=None)), D, BIG, None), b"bytes is NULL")
    _refused(f(C.byref(g), C.byref(s), C.byref(o), D, C.c_size_t(8), None), b"workspace too small")
    _refused(f(C.byref(g), C.byref(_slot_cols(LIMIT)), C.byref(o), D, BIG, None), b"pass 2^32")


def test_bytes_may_be_null_only_with_cap_zero():
    """cap 0 sizes a batch (msg_off and nbytes are still complete): bytes is not
    needed; the refusal then is the next check's, not the buffer's."""
    lib = _lib.load()
    rc = lib.qb_dev_encode_messages(8, C.byref(_cols()), C.byref(_out(bytes=None, cap=0)), D,
                                    C.c_size_t(8), None)
    _refused(rc, b"workspace too small")


def test_struct_mirrors_match_header(tmp_path):
    """sizeof and every field offset of the four structs, from gcc on the
    header itself."""
    mirrors = {"qb_encode_out": encode.EncodeOutC, "qb_encode_cols": encode.EncodeColsC,
               "qb_encode_groups": encode.EncodeGroupsC,
               "qb_encode_slot_cols": encode.EncodeSlotColsC}
    lines, want = [], []
    for name, cls in mirrors.items():
        lines.append(f'printf("%zu\\n", sizeof({name}));')
        want.append(C.sizeof(cls))
        for fname, _ in cls._fields_:
            lines.append(f'printf("%zu\\n", offsetof({name}, {fname}));')
            want.append(getattr(cls, fname).offset)
    lines.append('printf("%d %d %d\\n", QB_ENC_MAX_BYTES, QB_ENC_STATUS_COUNT, (int)sizeof(qb_msg_out));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quorum_batch.h"\n'
                   "int main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in got[:-3]] == want
    assert [int(x) for x in got[-3:]] == [encode.ENC_MAX_BYTES, len(encode.ENC_STAT_NAMES),
                                          encode.MSG_OUT_BYTES]


def test_wrappers_refuse_host_tensors_and_short_columns():
    import torch
    z = torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(_lib.QuorumBatchError, match="device tensor"):
        encode.encode_columns({"type": z})
    with pytest.raises(_lib.QuorumBatchError, match="required"):
        encode.encode_columns({"to": z})
    with pytest.raises(_lib.QuorumBatchError, match="unknown"):
        encode.encode_columns({"type": z, "frm": z})
    g = encode.EncodeGroups(torch.zeros(2, dtype=torch.int32), z, z, z, 1)
    with pytest.raises(_lib.QuorumBatchError, match="device tensor"):
        encode.encode_slots(g)
    with pytest.raises(_lib.QuorumBatchError, match="device tensor"):
        encode.encode_msg_out(g, z)
    assert encode.max_bytes(0) == 0 and encode.max_bytes(1000) == 111000
