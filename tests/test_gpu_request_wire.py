"""qb_dev_ingest_requests on the device, bit-exact against
tests/request_wire_ref.py on every message column, dense output and counter,
with the byte buffer and every output inside marker-filled guarded buffers
(tests/request_wire_pack.py).  G = 257 (a second, partial tile), M = 1031
seeded messages over every Message.Type value 0..19 and one above 2^31."""
import random

import numpy as np
import pytest

from oracle import raftpb_ref as W
from tests import request_wire_pack as P, request_wire_ref as RW

pytestmark = pytest.mark.gpu
STAGE_FITS = 16 * 1024 - 16  # the longest byte span a workgroup stages


@pytest.fixture(scope="module")
def base_want():
    msgs, grp = P.base_batch()
    buf, off = P.pack(msgs)
    goff, gids = P.config()
    return {(mr, cc): RW.ingest(buf, len(buf), off, grp, goff, gids, mr, cc)
            for mr in (1, 16) for cc in (False, True)}


def test_generator_meets_the_mixture(base_want):
    msgs, _ = P.base_batch()
    for want in base_want.values():
        P.assert_mixture(want, P.M)
    types = {RW.decode(m, 0, 1, ())["msg_type"] for m in msgs}
    assert set(range(20)) <= types  # (and the one above 2^31 is a special case)
    assert len(msgs) // 16 >= 2 * len(P.special_cases())  # every case is in the batch


@pytest.mark.parametrize("concat", (False, True))
@pytest.mark.parametrize("max_reads", (1, 16))
def test_mixture(max_reads, concat):
    msgs, grp = P.base_batch()
    want, _ = P.run(msgs, grp, max_reads=max_reads, concat=concat)
    P.assert_mixture(want, P.M)
    taken = (want["status"] == RW.OK) & (want["kind"] == RW.RQ_PROP)
    assert (want["ent_base"][taken] > 0).any() == concat
    assert (want["n_reads"] > 1).any() == (max_reads > 1)


@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257))
def test_sizes_around_the_tile(n):
    msgs, grp = P.base_batch()
    P.run(msgs[:n], grp[:n], max_reads=2, concat=True)


def test_every_special_case_alone():
    cases = P.special_cases()
    msgs = [b for b, _ in cases.values()]
    cfg = (np.arange(len(msgs) + 1, dtype=np.uint32) * 2, np.tile(np.array([3, 5], np.uint64), len(msgs)))
    want, _ = P.run(msgs, list(range(len(msgs))), n_groups=len(msgs), cfg=cfg)
    got = dict(zip(cases, want["status"].tolist()))
    assert got == {k: st for k, (_, st) in cases.items()}
    col = lambda name, k: int(want[k][list(cases).index(name)])  # noqa: E731
    assert col("unknown field inside ConfChangeV2", "cc_at") == 0
    assert col("unknown field inside ConfChangeV2", "cc_leave") == 0
    assert col("nil V2 leaves", "cc_leave") == 1 and col("nil V2 leaves", "cc_payload") == 0
    assert col("empty V1 is no leave", "cc_leave") == 0 and col("empty V1 is no leave", "cc_at") == 0
    assert col("conf change third of four", "cc_at") == 2 and col("conf change third of four", "ent_n") == 4
    assert col("nil Data", "payload") == 0 and col("nil Data", "cc_at") == RW.NO_CC
    assert col("repeated Data", "ctx") == int.from_bytes(b"ABCDEFGH", "big")
    assert col("varints of ten bytes", "frm") == (1 << 64) - 1


def test_from_zero_a_member_and_a_non_member():
    mem = P.members(5)  # 16 members: the lookup's fourth round trip
    assert len(mem) == 16
    froms = [0] + mem + [mem[3] + 1, (1 << 64) - 1]
    msgs = [P.transfer(f) for f in froms] + [P.read(100 + k, frm=f) for k, f in enumerate(froms)]
    want, _ = P.run(msgs, [5] * len(msgs), max_reads=16)
    slots = [RW.SLOT_LOCAL] + list(range(16)) + [RW.SLOT_NONE] * 2
    assert want["slot"].tolist() == [RW.SLOT_NONE] + slots[1:] + slots
    # the first transfer (From 0: no Progress) is taken, the second defers the rest
    assert int(want["n_reads"][5]) == 0 and int(want["xf_from"][5]) == RW.SLOT_NONE
    assert want["status"].tolist() == [RW.OK] + [RW.DEFERRED] * (len(msgs) - 1)
    want, _ = P.run(msgs[len(froms) - 1:], [5] * (len(froms) + 1), max_reads=16)
    assert int(want["n_reads"][5]) == 16 and want["rd_k"][1:17].tolist() == list(range(16))
    assert want["rd"][(0, 5)] == (100, RW.SLOT_LOCAL) and want["rd"][(3, 5)] == (103, 2)


def _victim():
    return P.prop([P.ent(b"xyz"), P.ent(P.marshal_cc_v2(1, [(0, 7), (1, 300)], b"c"), 2), P.ent(b"")],
                  frm=3, index=9)


def test_truncation_at_every_byte_of_one_msgprop_with_a_v2_conf_change():
    v = _victim()
    msgs, grp = map(list, P.base_batch())
    msgs, grp = msgs[:257], grp[:257]
    cuts = [v[:n] for n in range(len(v) + 1)]
    for n, c in enumerate(cuts):  # spread through the tiles
        msgs.insert(3 * n + 1, c)
        grp.insert(3 * n + 1, n % P.G)
    want, _ = P.run(msgs, grp, concat=True)
    st = [int(want["status"][3 * n + 1]) for n in range(len(cuts))]
    assert st[-1] in (RW.OK, RW.DEFERRED) and st[0] == RW.TYPE  # whole, and the empty message (type 0)
    assert st.count(RW.UNMARSHAL) >= len(v) // 2
    # (a cut inside the conf change's Data cuts its entry too: never CONF_CHANGE)
    assert set(st) <= {RW.OK, RW.DEFERRED, RW.UNMARSHAL, RW.TYPE, RW.ENTRIES}
    assert want["cc_at"][3 * len(v) + 1] == 1


def test_corruptions_fed_through_the_whole_batch():
    bad = P.corruptions()
    msgs, grp = map(list, P.base_batch())
    msgs, grp = msgs[:300], grp[:300]
    at = {}
    for n, (name, b) in enumerate(bad.items()):
        at[name] = 70 * n + 5
        msgs[at[name]] = b
    want, _ = P.run(msgs, grp)
    for name, i in at.items():
        assert want["status"][i] == RW.UNMARSHAL and want["group"][i] == RW.NO_GROUP, name


def test_a_msgprop_past_the_lds_stage_goes_to_the_global_launch():
    r = random.Random(5)
    big = P.prop([P.ent(bytes(STAGE_FITS + 100)), P.ent(P.marshal_cc_v2(0, [(0, 9)]), 2), P.ent(b"tail")], frm=1)
    assert len(big) > 16 * 1024
    msgs = [P._one(r, i % P.G, ("prop", "read", "transfer")[i % 3]) for i in range(300)]
    msgs.insert(130, big)
    grp = [i % P.G for i in range(300)]
    grp.insert(130, 256)
    want, _ = P.run(msgs, grp, concat=True, max_reads=4)
    assert want["status"][130] == RW.OK and want["cc_at"][130] == 1 and want["ent_bytes"][130] > STAGE_FITS
    assert want["payload"][130] == STAGE_FITS + 100 + len(P.marshal_cc_v2(0, [(0, 9)])) + 4


@pytest.mark.parametrize("residue", (0, 1, 7, 8, 15))
def test_byte_buffer_at_an_alignment(residue):
    msgs, grp = P.base_batch()
    P.run(msgs[:300], grp[:300], residue=residue, max_reads=3)


@pytest.mark.parametrize("what", ("descending", "past nbytes", "huge", "short buffer"))
def test_offsets_that_are_not_inside_the_buffer(what):
    msgs, grp = P.base_batch()
    n = 600
    msgs, grp = msgs[:n], grp[:n]
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
    else:
        nbytes -= 700  # the offsets run on behind a shorter buffer
        hit = [int(np.nonzero(off > nbytes)[0][0]) - 1, n - 1]
    want, _ = P.run(msgs, grp, off=off, nbytes=nbytes)
    for i in hit:
        assert want["status"][i] == RW.UNMARSHAL and want["group"][i] == RW.NO_GROUP, (what, i)


@pytest.mark.parametrize("concat", (False, True))
@pytest.mark.parametrize("max_reads", (1, 16))
def test_skew_every_message_to_one_group(max_reads, concat):
    """Exactly max_reads reads and one transfer, or one proposal (with concat:
    up to the second conf change), are taken; the rest is deferred in order."""
    msgs, _ = P.base_batch()
    want, _ = P.run(msgs, [200] * P.M, max_reads=max_reads, concat=concat)
    live = np.nonzero((want["status"] == RW.OK) | (want["status"] == RW.DEFERRED))[0]
    live = live[want["kind"][live] != RW.RQ_READ_RESP]
    st = want["status"][live]
    first = int(np.argmax(st == RW.DEFERRED))
    assert (st[:first] == RW.OK).all() and (st[first:] == RW.DEFERRED).all() and first > 0
    assert len(live) > 300 and want["gflags"][200] == 3 and (np.delete(want["gflags"], 200) == 0).all()
    taken = want["kind"][live[:first]].tolist()
    assert taken.count(RW.RQ_READ) <= max_reads and taken.count(RW.RQ_TRANSFER) <= 1
    if not concat:
        assert taken.count(RW.RQ_PROP) <= 1
    # what stopped the walk is what the rules name
    k = want["kind"][live[first]]
    assert (k == RW.RQ_READ and (taken.count(RW.RQ_READ) == max_reads or RW.RQ_PROP in taken)) or \
        (k == RW.RQ_TRANSFER and (RW.RQ_TRANSFER in taken or RW.RQ_PROP in taken)) or \
        (k == RW.RQ_PROP and RW.RQ_PROP in taken)


def test_a_long_run_past_the_lds_sort():
    """5000 requests of one group (past the 4096 the long-run kernel sorts in
    LDS) beside 40 of another: sorted in the workspace."""
    r = random.Random(11)
    msgs = [P.read(k + 1, frm=0) if k % 3 else P.prop([P.ent(b"ab")]) for k in range(5000)]
    msgs = msgs[1:] + [P._one(r, 7, "read") for _ in range(40)]
    want, _ = P.run(msgs, [3] * 4999 + [7] * 40, max_reads=16, concat=True)
    assert int(want["n_reads"][3]) == 2 and int(want["n_reads"][7]) == 16
    assert int((want["status"] == RW.DEFERRED).sum()) == 4999 - 3 + 40 - 16  # two reads and the proposal behind them


def test_no_messages_still_writes_the_dense_columns():
    want, g = P.run([], [], max_reads=2)
    assert (g.host("xf_from")[0] == RW.SLOT_LOCAL).all() and not g.host("gflags")[0].any()


def test_wrapper_allocates_and_returns_the_inboxes():
    import torch

    from etcd_amd.quorum import ProposeInbox, RequestInbox, ingest_requests
    msgs, grp = P.base_batch()
    buf, off = P.pack(msgs)
    goff, gids = P.config()
    want = RW.ingest(buf, len(buf), off, grp, goff, gids, 4, True)
    b = P.Bytes(buf)
    stats = torch.zeros(RW.STAT_COUNT, dtype=torch.int64, device=P.DEV)
    got = ingest_requests(b.buf, len(buf), P.dev(off), P.dev(np.array(grp, np.uint32)), P.dev(goff),
                          P.dev(gids), max_reads=4, concat=True, stats=stats)
    torch.cuda.synchronize()
    assert isinstance(got.request_in, RequestInbox) and isinstance(got.propose_in, ProposeInbox)
    assert got.request_in.max_reads == 4 and got.request_in.rd_ctx.numel() == 4 * P.G
    assert np.array_equal(got.status.cpu().numpy(), want["status"])
    assert np.array_equal(got.frm.cpu().numpy().view(np.uint64), want["frm"])
    assert np.array_equal(got.propose_in.n_ents.cpu().numpy().view(np.uint32), want["n_ents"])
    assert np.array_equal(got.request_in.n_reads.cpu().numpy(), want["n_reads"])
    assert np.array_equal(stats.cpu().numpy().view(np.uint64), want["stats"])
    assert W.decode_message(msgs[0])[0]
