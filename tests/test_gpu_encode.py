"""qb_dev_encode_messages / _msg_out / _slots on the device, bit-exact against
tests/encode_ref.py: bytes[0:nbytes], msg_off, status, ent_at, nbytes and the
stats, with every output pre-filled with a marker that must survive wherever
nothing is to be written (tests/encode_pack.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from etcd_amd import _lib
from etcd_amd.quorum import encode, wire
from tests import encode_pack as P, encode_ref as E

pytestmark = pytest.mark.gpu
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1000)
TILE = 256


def test_columns_inputs_cover_every_path():
    P.assert_columns_cover(P.column_batch(1000), 1000)


@pytest.mark.parametrize("M", SIZES)
def test_columns(M):
    cols = P.column_batch(1000)
    P.assert_columns_cover(cols, 1000)
    want = E.finish(E.columns(cols, M))
    g = P.Guarded(M, want["nbytes"] + 9)
    encode.encode_columns(P.cols_dev(cols, M), M=M, out=g.out)
    g.check(want)


@pytest.mark.parametrize("M", SIZES)
def test_msg_out_list(M):
    G, off, ids, self_id, term = P.group_table()
    recs = P.list_batch(1000)
    total = 1000 - 3
    P.assert_list_covers(recs, 1000, total)
    tot = None if M in (63, 256) else max(M - 3, 0)   # msg_total below msg_cap, and absent
    want = E.finish(E.msg_out(G, off, ids, self_id, term, recs, M, tot))
    g = P.Guarded(M, want["nbytes"] + 1)
    msgs = torch.from_numpy(recs[:max(M, 1)].view(np.uint8).copy()).to(P.DEV)
    encode.encode_msg_out(P.groups_dev(), msgs, M,
                          None if tot is None else P.dev(np.array([tot], np.uint64)), out=g.out)
    g.check(want)
    if tot is not None:
        assert (want["status"][tot:] == E.NONE).all()


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("form", ("heartbeats", "bcast"))
def test_slots(M, form):
    """The tick's heartbeats (type_all, gflags & mask, per-slot commit, the
    group's context) and bcastAppend's columns (per-slot types, gflags NULL,
    the group's commit); S = M slots of the table, and 5 the table does not
    cover at the largest size."""
    G, off, ids, self_id, term = P.group_table()
    sc = P.slot_columns()
    assert int(off[-1]) >= 1000
    S = M if M < 1000 else int(off[-1]) + 5
    assert any(int(self_id[g]) not in ids[off[g]:off[g + 1]].tolist() for g in range(G))
    if form == "heartbeats":
        cols = {"commit": sc["commit"], "ctx_g": sc["ctx_g"]}
        kw = dict(gflags=sc["gflags"], gmask=2, type_all=E.MSG_HEARTBEAT)
    else:
        cols = {k: sc[k] for k in ("type", "index", "log_term", "n_entries", "commit_g")}
        kw = dict(gflags=None, gmask=0xFF, type_all=0)
    recs = E.slots(G, off, ids, self_id, term, S, cols=cols, **kw)
    if S >= 1000:
        want_st = {E.OK, E.NONE} if form == "heartbeats" else {E.OK, E.ENTRIES, E.HOST, E.NONE}
        assert {st for st, _ in recs} == want_st
        assert all(st == E.NONE for st, _ in recs[int(off[-1]):])
    want = E.finish(recs)
    g = P.Guarded(S, want["nbytes"])
    encode.encode_slots(P.groups_dev(S), gflags=None if kw["gflags"] is None else P.dev(kw["gflags"]),
                        gmask=kw["gmask"], type_all=kw["type_all"], cols=P.cols_dev(cols), out=g.out)
    g.check(want)


def test_a_full_stage_of_all_maximum_messages():
    top = (1 << 64) - 1
    M = 2 * TILE + 1
    cols = {"type": np.full(M, 16, np.uint8), "reject": np.ones(M, np.uint8)}
    for k in P.U64_COLS + ("context",):
        cols[k] = np.full(M, top, np.uint64)
    want = E.finish(E.columns(cols, M))
    assert want["nbytes"] == M * encode.ENC_MAX_BYTES
    g = P.Guarded(M, want["nbytes"])
    encode.encode_columns(P.cols_dev(cols), out=g.out)
    g.check(want)


def test_only_length_zero_statuses():
    M = 700
    cols = {"type": np.where(np.arange(M) % 3 == 0, 7, 0).astype(np.uint8),
            "to": np.arange(M, dtype=np.uint64)}
    want = E.finish(E.columns(cols, M))
    assert want["nbytes"] == 0 and set(want["status"].tolist()) == {E.HOST, E.NONE}
    g = P.Guarded(M, 40)
    encode.encode_columns(P.cols_dev(cols), out=g.out)
    g.check(want)


def test_tile_boundaries_at_every_residue():
    """17 tiles, each one byte longer than a multiple of 16: the tile
    boundaries take every residue mod 16, whatever the buffer's own."""
    M = 17 * TILE
    to = np.full(M, 5, np.uint64)
    to[::TILE] = 128                      # one message a tile is a byte longer
    cols = {"type": np.full(M, 8, np.uint8), "to": to, "commit": np.full(M, 300, np.uint64)}
    want = E.finish(E.columns(cols, M))
    starts = want["msg_off"][::TILE].astype(np.int64)
    assert len(starts) == 18 and {int(x) % 16 for x in starts[:17]} == set(range(16))
    g = P.Guarded(M, want["nbytes"])
    assert {int(g.residue() + x) % 16 for x in starts[:17]} == set(range(16))
    encode.encode_columns(P.cols_dev(cols), out=g.out)
    g.check(want)


def test_cap_clips_at_message_granularity():
    M = 300
    cols = P.column_batch(1000)
    full = E.finish(E.columns(cols, M))
    off = full["msg_off"].astype(np.int64)
    lens = np.diff(off)
    j = int(np.nonzero(lens[140:] > 0)[0][0]) + 140     # a message with bytes, in the first tile
    k = int(np.nonzero(lens[270:] > 0)[0][0]) + 270     # and one in the second
    caps = {"zero": 0, "inside a message": int(off[j]) + 5, "at a message's end": int(off[k + 1]),
            "exact": int(full["nbytes"])}
    assert 0 < caps["inside a message"] < off[j + 1] < caps["at a message's end"] < caps["exact"]
    for what, cap in caps.items():
        want = E.finish(E.columns(cols, M), cap)
        first = {"zero": int(np.nonzero(lens > 0)[0][0]), "inside a message": j,
                 "at a message's end": k + 1 + int(np.nonzero(lens[k + 1:] > 0)[0][0])}.get(what)
        if first is None:
            assert E.NO_SPACE not in want["status"]
        else:
            ns = np.nonzero(want["status"] == E.NO_SPACE)[0]
            assert ns[0] == first and np.array_equal(ns, first + np.nonzero(lens[first:] > 0)[0]), what
        assert np.array_equal(want["msg_off"], full["msg_off"])
        g = P.Guarded(M, cap)
        encode.encode_columns(P.cols_dev(cols, M), M=M, out=g.out)
        g.check(want)


def test_equals_encode_appresp_on_its_domain():
    M = 1000
    gen = torch.Generator(device="cpu").manual_seed(3)
    r = lambda lo, hi: torch.randint(lo, hi, (M,), generator=gen, dtype=torch.int64).to(P.DEV)  # noqa: E731
    to, frm, term = r(1 << 14, 1 << 21), r(1 << 14, 1 << 21), r(1 << 14, 1 << 21)
    index, reject = r(1 << 35, 1 << 42), r(0, 2).to(torch.uint8)
    buf, nbytes, moff = wire.encode_appresp(to, frm, term, index, reject)
    b, off, st, at, nb = encode.encode_columns(
        {"type": torch.full((M,), 4, dtype=torch.uint8, device=P.DEV), "to": to, "from": frm,
         "term": term, "index": index, "reject": reject})
    torch.cuda.synchronize()
    assert int(nb[0]) == nbytes and torch.equal(off, moff)
    assert torch.equal(b[:nbytes], buf[:nbytes]) and int(st.max()) == encode.ENC_OK


def test_responses_round_trip_through_wire_ingest():
    """MsgAppResp / MsgHeartbeatResp from encode_columns, fed as device bytes
    and offsets into wire.ingest, come back as the columns they were built
    from."""
    G, off, ids, self_id, term = P.group_table()
    M = 1000
    rng = np.random.default_rng(17)
    grp = rng.integers(0, G, M).astype(np.uint32)
    slot = (rng.integers(0, 1 << 30, M) % (off[grp + 1] - off[grp])).astype(np.uint32)
    hb = rng.random(M) < 0.4
    r = P.random.Random(17)
    u64 = lambda: np.array([P.rand_u64(r) for _ in range(M)], np.uint64)  # noqa: E731
    ctx = np.where(hb & (rng.random(M) < 0.7), u64() | np.uint64(1), 0).astype(np.uint64)
    cols = {"type": np.where(hb, 9, 4).astype(np.uint8), "to": self_id[grp],
            "from": ids[off[grp] + slot], "term": u64(), "log_term": u64(), "index": u64(),
            "reject": (rng.random(M) < 0.3).astype(np.uint8), "reject_hint": u64(),
            "context": ctx}
    b, moff, st, _, nb = encode.encode_columns(P.cols_dev(cols))
    torch.cuda.synchronize()
    assert int(st.max()) == encode.ENC_OK
    gd = P.groups_dev()
    ib, wst, mtype = wire.ingest(b, int(nb[0]), moff, P.dev(grp), gd.off, gd.ids)
    torch.cuda.synchronize()
    assert int(wst.max()) == wire.WIRE_OK
    assert np.array_equal(mtype.cpu().numpy(), cols["type"])
    assert np.array_equal(ib.group.cpu().numpy().view(np.uint32)[:M], grp)
    flags = slot.astype(np.uint8) | np.where(hb, 1 << 4, 0).astype(np.uint8) | (cols["reject"] << 7)
    assert np.array_equal(ib.flags.cpu().numpy()[:M], flags)
    u = lambda t: t.cpu().numpy().view(np.uint64)[:M]  # noqa: E731
    assert np.array_equal(u(ib.index), np.where(hb, ctx, cols["index"]))
    assert np.array_equal(u(ib.term), cols["term"])
    assert np.array_equal(u(ib.hint), cols["reject_hint"])
    assert np.array_equal(u(ib.log_term), cols["log_term"])


def test_raw_c_abi_beside_the_wrapper():
    """qb_dev_encode_messages through ctypes alone, ent_at and stats NULL."""
    M = 257
    cols = P.column_batch(1000)
    want = E.finish(E.columns(cols, M))
    d = P.cols_dev(cols, M)
    lib = _lib.load()
    need = lib.qb_encode_scratch_bytes(M)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=P.DEV)
    cap = want["nbytes"]
    buf = torch.full((cap + 16,), P.FILL, dtype=torch.uint8, device=P.DEV)
    moff = torch.zeros(M + 1, dtype=torch.int64, device=P.DEV)
    st = torch.zeros(M, dtype=torch.uint8, device=P.DEV)
    nb = torch.zeros(1, dtype=torch.int64, device=P.DEV)
    cc = encode.EncodeColsC(**{k: d[k].data_ptr() for k in d})
    oc = encode.EncodeOutC(bytes=buf.data_ptr(), cap=cap, msg_off=moff.data_ptr(),
                           status=st.data_ptr(), ent_at=None, nbytes=nb.data_ptr(), stats=None)
    rc = lib.qb_dev_encode_messages(M, C.byref(cc), C.byref(oc), ws.data_ptr(), C.c_size_t(need),
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.QB_OK, lib.qb_last_error()
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert got[:cap].tobytes() == want["bytes"].tobytes() and (got[cap:] == P.FILL).all()
    assert np.array_equal(moff.cpu().numpy().view(np.uint64), want["msg_off"])
    assert np.array_equal(st.cpu().numpy(), want["status"]) and int(nb[0]) == cap
    b2 = encode.encode_columns(d, M=M)[0]
    assert torch.equal(b2[:cap], buf[:cap])
