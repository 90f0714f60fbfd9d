"""qb_dev_ingest_follower on the device, bit-exact against
tests/follower_wire_ref.py on every output column, ent_off, the term runs,
ent_total and the stats, with the byte buffer and every output inside
marker-filled guarded buffers (tests/follower_wire_pack.py).

The mixture: the issue asks that the generator leave "at least a fifth of the
messages in each of the five device kinds with status OK", which five kinds
beside host types cannot all have of the whole batch; it is asserted here as
what the sentence can mean — of each kind's own messages at least a fifth is
OK — and, stronger, each kind with status OK is an eighth of the batch (the
generator's rotation: five lanes in eight, a fifth of them each)."""
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch

from etcd_amd import _lib
from etcd_amd.quorum import wire
from oracle import raftpb_ref as W
from tests import follower_wire_pack as P, follower_wire_ref as FW

pytestmark = pytest.mark.gpu
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1000)
TILE = 256
STAGE_FITS = 16 * 1024 - 16  # the longest byte span a workgroup stages


def test_generator_leaves_every_device_kind(base_want):
    P.assert_mixture(base_want, 1000)
    msgs, _ = P.base_batch()
    r = random.Random(1)
    names = set(P.app_cases(r)) | set(P.corruptions(r))
    assert len(names) == 17 and len(msgs) // 8 >= 2 * len(names)  # every case is in the batch


@pytest.fixture(scope="module")
def base_want():
    msgs, grp = P.base_batch()
    buf, off = P.pack(msgs)
    return FW.ingest(buf, len(buf), off, grp)


@pytest.mark.parametrize("M", SIZES)
def test_mixture(M):
    msgs, grp = P.base_batch()
    want, _ = P.run(msgs[:M], grp[:M])
    if M >= 63:
        P.assert_mixture(want, M)
    if M == 1000:
        assert any(len(r) == 9 for r in want["runs"]) and any(r == [(9, 200)] for r in want["runs"])
        assert want["ent_bytes"].max() > 3000


def test_every_msgapp_case_alone():
    r = random.Random(3)
    cases = P.app_cases(r)
    want, _ = P.run(list(cases.values()), list(range(len(cases))))
    st = dict(zip(cases, want["status"].tolist()))
    bad = {"gap", "repeated index", "first index off", "commit between entries"}
    assert {k for k, v in st.items() if v == FW.ENTRIES} == bad
    assert all(v == FW.OK for k, v in st.items() if k not in bad)
    runs = dict(zip(cases, want["runs"]))
    assert runs["no entries"] == [] and runs["one entry"] == [(7, 1)]
    assert runs["one run of 200"] == [(9, 200)] and len(runs["nine runs"]) == 9
    assert runs["alternating terms"] == [(4, 1), (5, 1)] * 6
    assert runs["term 0"] == [(0, 2), (3, 1)] and runs["wrap"] == [(2, 2), (3, 1)]
    assert runs["data sizes"] == [(6, 3), (8, 1)]


def _padded_block(total):
    """256 messages of exactly ``total`` bytes: 255 short ones of four kinds and
    one MsgApp whose entry's Data (and, where the varint lengths jump past the
    size, an unknown field 13 behind it) makes up the rest."""
    msgs = [W.marshal_message(type=(8, 5, 17, 14)[i % 4], to=1, frm=i, term=2, commit=i,
                              snapshot=(W.EMPTY_SNAPSHOT, P.BRIEF_SNAPSHOT)[i % 2]) for i in range(255)]
    rest = total - sum(len(m) for m in msgs)
    assert rest > 3000
    mk = lambda n: W.marshal_message(type=3, to=1, frm=2, term=3, log_term=3, index=5, commit=5,  # noqa: E731
                                     entries=P.f7([(3, 6, bytes(n))]))
    for pad in (b"", b"\x68\x00", b"\x68\x80\x00"):
        for n in range(rest - 60, rest):
            if len(mk(n)) + len(pad) == rest:
                return msgs + [mk(n) + pad]
    raise AssertionError("no padding reaches the size")


def test_a_block_that_fits_the_stage_exactly_and_one_that_does_not():
    r = random.Random(5)
    blocks = _padded_block(STAGE_FITS) + _padded_block(STAGE_FITS + 1) + \
        [P.device_kind(r, i) for i in range(40)]
    _, off = P.pack(blocks)
    assert int(off[256]) == STAGE_FITS and int(off[512] - off[256]) == STAGE_FITS + 1
    want, _ = P.run(blocks, [i % (P.G + 3) for i in range(len(blocks))])
    assert (want["status"] == FW.OK).all()


def test_run_total_past_one_scan_block():
    r = random.Random(7)
    msgs = [P.app(r, 10 * i, [1, 2, 3, 4, 5]) for i in range(1000)]
    want, _ = P.run(msgs, list(range(1000)))
    assert want["ent_total"] == 5000 > 4096 and (want["status"] == FW.OK).all()


def test_ent_cap_clips_at_message_granularity():
    M = 300
    msgs, grp = P.base_batch()
    msgs, grp = msgs[:M], grp[:M]
    buf, off = P.pack(msgs)
    full = FW.ingest(buf, len(buf), off, grp)
    eo = full["ent_off"].astype(np.int64)
    counts = np.diff(eo)
    j = int(np.nonzero(counts[140:] >= 2)[0][0]) + 140   # runs in the first tile
    k = int(np.nonzero(counts[270:] > 0)[0][0]) + 270    # and in the second
    caps = {"zero": 0, "inside a message": int(eo[j]) + 1, "at a message's end": int(eo[k + 1]),
            "exact": int(full["ent_total"])}
    assert 0 < caps["inside a message"] < eo[j + 1] < caps["at a message's end"] <= caps["exact"]
    for what, cap in caps.items():
        want, _ = P.run(msgs, grp, ent_cap=cap)
        first = {"zero": int(np.nonzero(counts)[0][0]), "inside a message": j,
                 "at a message's end": (k + 1 + int(np.nonzero(counts[k + 1:])[0][0])
                                        if counts[k + 1:].any() else None)}.get(what)
        ns = np.nonzero(want["status"] == FW.NO_SPACE)[0]
        if first is None:
            assert len(ns) == 0
        else:
            assert ns[0] == first and np.array_equal(ns, first + np.nonzero(counts[first:])[0]), what
        assert np.array_equal(want["ent_off"], full["ent_off"]) and want["ent_total"] == full["ent_total"]


@functools.lru_cache(maxsize=None)
def _victim():
    return W.marshal_message(type=3, to=1, frm=2, term=3, log_term=3, index=1000, commit=7,
                             entries=P.f7([(3, 1001, b"xyz"), (4, 1002, b"")]))


def test_truncation_at_every_byte_of_one_msgapp():
    v = _victim()
    msgs, grp = map(list, P.base_batch())
    msgs, grp = msgs[:257], grp[:257]
    cuts = [v[:n] for n in range(len(v) + 1)]
    for n, c in enumerate(cuts):  # spread through both tiles
        msgs.insert(3 * n + 1, c)
        grp.insert(3 * n + 1, n)
    want, _ = P.run(msgs, grp)
    st = [int(want["status"][3 * n + 1]) for n in range(len(cuts))]
    assert st[-1] == FW.OK and st[0] == FW.TYPE  # whole, and the empty message (type 0)
    assert st.count(FW.UNMARSHAL) >= len(v) // 2 and set(st) <= {FW.OK, FW.UNMARSHAL, FW.TYPE, FW.ENTRIES}


def test_corruptions_fed_through_the_whole_batch():
    r = random.Random(9)
    bad = P.corruptions(r)
    msgs, grp = map(list, P.base_batch())
    msgs, grp = msgs[:300], grp[:300]
    at = {}
    for n, (name, b) in enumerate(bad.items()):
        at[name] = 70 * n + 5
        msgs[at[name]] = b
    want, _ = P.run(msgs, grp)
    for name, i in at.items():
        assert want["status"][i] == FW.UNMARSHAL and want["group"][i] == FW.NO_GROUP, name


@pytest.mark.parametrize("what", ("descending", "past nbytes", "huge", "block past the buffer",
                                  "short buffer"))
def test_offsets_that_are_not_inside_the_buffer(what):
    msgs, grp = P.base_batch()
    M = 600
    msgs, grp = msgs[:M], grp[:M]
    buf, off = P.pack(msgs)
    off = off.copy()
    nbytes = len(buf)
    hit = []
    if what == "descending":
        for i in (7, 256, 300):
            off[i] = off[i + 1] + 5
            hit.append(i)
    elif what == "past nbytes":
        for i in (9, 255, 512):
            off[i] = nbytes + 100
            hit += [i - 1, i]
    elif what == "huge":
        for i, v in ((11, 1 << 63), (256, (1 << 64) - 1), (513, 1 << 32)):
            off[i] = v
            hit += [i - 1, i]
    elif what == "block past the buffer":   # a whole tile's span behind the bytes, small enough to stage
        off[512:] = nbytes + 100 + 40 * np.arange(M + 1 - 512, dtype=np.uint64)
        hit = list(range(511, M))
    else:
        nbytes -= 700                        # the offsets run on behind a shorter buffer
        hit = [int(np.nonzero(off > nbytes)[0][0]) - 1, M - 1]
    want, _ = P.run(msgs, grp, off=off, nbytes=nbytes)
    for i in hit:
        assert want["status"][i] == FW.UNMARSHAL and want["group"][i] == FW.NO_GROUP, (what, i)
    assert (want["status"] == FW.OK).sum() > 200


@pytest.mark.parametrize("residue", range(16))
def test_byte_buffer_at_every_alignment(residue):
    msgs, grp = P.base_batch()
    P.run(msgs[:300], grp[:300], residue=residue)


def test_empty_batch_still_says_so():
    want, g = P.run([], [])
    assert want["ent_total"] == 0 and int(g.host("ent_off")[0][0]) == 0


def test_wrapper_allocates_and_defaults():
    msgs, grp = P.base_batch()
    buf, off = P.pack(msgs)
    want = FW.ingest(buf, len(buf), off, grp)
    b = P.Bytes(buf)
    got = wire.ingest_follower(b.buf, len(buf), P.dev(off), P.dev(np.array(grp, np.uint32)), P.G)
    torch.cuda.synchronize()
    assert got.app.E == len(buf) // 2 and got.inbox.M == 1000
    assert np.array_equal(got.status.cpu().numpy(), want["status"])
    assert np.array_equal(got.ent_n.cpu().numpy().view(np.uint32), want["ent_n"])
    assert int(got.ent_total[0]) == want["ent_total"]


def test_raw_c_abi_with_every_nullable_pointer_null():
    """qb_dev_ingest_follower through ctypes alone: msg_type, ent_pos,
    ent_bytes, ent_n and stats NULL (the entry ranges then live in the
    workspace)."""
    M = 257
    msgs, grp = P.base_batch()
    buf, off = P.pack(msgs[:M])
    want = FW.ingest(buf, len(buf), off, grp[:M])
    cap = want["ent_total"]
    lib = _lib.load()
    need = lib.qb_wire_follower_scratch_bytes(M)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=P.DEV)
    b = P.Bytes(buf)
    o = wire.new_follower_out(M, cap, P.DEV)
    c = wire.FollowerWireOutC(o.inbox.group.data_ptr(), o.inbox.flags.data_ptr(), o.inbox.frm.data_ptr(),
                              o.inbox.term.data_ptr(), o.inbox.index.data_ptr(), o.inbox.aux.data_ptr(),
                              o.app.commit.data_ptr(), o.status.data_ptr(), None, None, None, None,
                              o.app.ent_off.data_ptr(), o.app.ent_term.data_ptr(),
                              o.app.ent_len.data_ptr(), cap, o.ent_total.data_ptr(), None)
    d_off, d_grp = P.dev(off), P.dev(np.array(grp[:M], np.uint32))
    rc = lib.qb_dev_ingest_follower(M, b.buf.data_ptr(), len(buf), d_off.data_ptr(),
                                    d_grp.data_ptr(), P.G, C.byref(c),
                                    ws.data_ptr(), C.c_size_t(need),
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.QB_OK, lib.qb_last_error()
    torch.cuda.synchronize()
    h = lambda t, dt, n: t.cpu().numpy().view(dt)[:n]  # noqa: E731
    assert np.array_equal(h(o.status, np.uint8, M), want["status"])
    assert np.array_equal(h(o.inbox.flags, np.uint8, M), want["flags"])
    assert np.array_equal(h(o.inbox.index, np.uint64, M), want["index"])
    assert np.array_equal(h(o.app.ent_off, np.uint32, M + 1), want["ent_off"])
    flat = [x for r in want["runs"] for x in r]
    assert len(flat) == cap == int(o.ent_total[0])
    assert h(o.app.ent_term, np.uint64, cap).tolist() == [t for t, _ in flat]
    assert h(o.app.ent_len, np.uint32, cap).tolist() == [n for _, n in flat]
