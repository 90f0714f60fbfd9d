"""Inputs, device buffers and comparisons shared by the qb_dev_ingest_requests
GPU tests: the conf-change encoders, a seeded mixture of the four request
kinds, every failing status, every Message.Type value and the corruptions (its
coverage asserted on the CPU with the restatement alone), every output inside
marker-filled guarded buffers, and the bit-exact comparison against
tests/request_wire_ref.py.

Test infrastructure."""
from __future__ import annotations

import functools
import random

import numpy as np
import torch

from etcd_amd.quorum import wire
from etcd_amd.quorum.propose import ProposeInbox
from etcd_amd.quorum.request import RequestInbox
from oracle import raftpb_ref as W
from tests import request_wire_ref as RW
from tests.encode_pack import rand_u64
from tests.follower_wire_pack import DEV, FILL, GUARD, Bytes, dev, pack  # noqa: F401

G = 257
M = 1031
SEED = 1
GROUP_SIZES = (1, 3, 5, 7, 9, 16, 4, 12)  # members of group g: GROUP_SIZES[g % 8]
OTHER_TYPES = tuple(t for t in range(20) if t not in (2, 13, 15, 16)) + ((1 << 31) + 2,)
_SIGNED = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint32): torch.int32,
           np.dtype(np.uint64): torch.int64}
MARKER = {1: FILL, 4: 0x5A5A5A5A, 8: 0x5A5A5A5A5A5A5A5A}


# ------------------------------------------------------------ encoders ---

def marshal_cc(cid=0, ctype=0, node=0, context=None) -> bytes:
    """ConfChange.Marshal: id, type and node_id always written, in field
    order; Context only when non-nil."""
    out = W._key(1, 0) + W.varint(cid) + W._key(2, 0) + W.varint(ctype) + W._key(3, 0) + W.varint(node)
    if context is not None:
        out += W._key(4, 2) + W.varint(len(context)) + context
    return out


def marshal_cc_v2(transition=0, changes=(), context=None) -> bytes:
    """ConfChangeV2.Marshal: transition always written; each change a
    ConfChangeSingle {type, node_id}, both always written."""
    out = W._key(1, 0) + W.varint(transition)
    for ctype, node in changes:
        single = W._key(1, 0) + W.varint(ctype) + W._key(2, 0) + W.varint(node)
        out += W._key(2, 2) + W.varint(len(single)) + single
    if context is not None:
        out += W._key(3, 2) + W.varint(len(context)) + context
    return out


def ent(data=b"x", etype=0, term=0, index=0) -> bytes:
    return W.marshal_entry(term, index, etype, data)


def prop(entries, frm=0, term=0, **kw) -> bytes:
    return W.marshal_message(type=RW.MSG_PROP, frm=frm, term=term, entries=entries, **kw)


def read(ctx, frm=0, term=0, **kw) -> bytes:
    data = ctx if isinstance(ctx, bytes) else ctx.to_bytes(8, "big")
    return W.marshal_message(type=RW.MSG_READ_INDEX, frm=frm, term=term, entries=[ent(data)], **kw)


def transfer(frm, term=0, **kw) -> bytes:
    return W.marshal_message(type=RW.MSG_TRANSFER, frm=frm, term=term, **kw)


def read_resp(ctx, index, frm=0, term=0, **kw) -> bytes:
    data = ctx if isinstance(ctx, bytes) else ctx.to_bytes(8, "big")
    return W.marshal_message(type=RW.MSG_READ_INDEX_RESP, frm=frm, term=term, index=index,
                             entries=[ent(data)], **kw)


def between_entries(e1: bytes, e2: bytes, mtype=RW.MSG_PROP) -> bytes:
    """A message whose two entries have Commit between them."""
    pre = b"".join(W._key(f, 0) + W.varint(v) for f, v in ((1, mtype), (2, 2), (3, 77), (4, 0)))
    f7 = [b"\x3a" + W.varint(len(x)) + x for x in (e1, e2)]
    return pre + f7[0] + b"\x40\x05" + f7[1]


# ------------------------------------------------------------- configs ---

@functools.lru_cache(maxsize=None)
def config(n_groups=G, seed=SEED):
    """(off u32 [G+1], ids u64): ascending member IDs per group."""
    r = random.Random(seed * 31 + n_groups)
    off, ids = [0], []
    for g in range(n_groups):
        n = GROUP_SIZES[g % len(GROUP_SIZES)]
        ids += sorted({rand_u64(r) | 1 for _ in range(n + 4)})[:n]
        off.append(len(ids))
    return np.array(off, np.uint32), np.array(ids, np.uint64)


def members(g, n_groups=G, seed=SEED):
    off, ids = config(n_groups, seed)
    return [int(v) for v in ids[off[g]:off[g + 1]]]


# ------------------------------------------------------------- mixture ---

def special_cases():
    """name -> (bytes, the status it has alone at a member-less group 0)."""
    v2 = marshal_cc_v2(1, [(0, 5), (2, 6)], b"ctx")
    c = {}
    c["unknown field inside Entry"] = (prop([ent(b"abc") + b"\x68\x07" + b"\x72\x02hi"]), RW.OK)
    c["unknown field inside ConfChangeV2"] = (
        prop([ent(v2 + b"\x68\x07" + b"\x7a\x01z" + b"\x25abcd", RW.ENTRY_CONF_CHANGE_V2)]), RW.OK)
    c["unknown field inside ConfChangeSingle"] = (
        prop([ent(b"\x08\x00\x12\x06\x08\x00\x10\x05\x18\x01", RW.ENTRY_CONF_CHANGE_V2)]), RW.OK)
    c["varints of ten bytes"] = (prop([ent(b"p", 0, (1 << 64) - 1, (1 << 63) + 5)], frm=(1 << 64) - 1,
                                      index=(1 << 64) - 2, commit=1 << 63), RW.OK)
    c["type above 2^31"] = (W.marshal_message(type=(1 << 31) + 2, entries=[ent()]), RW.TYPE)
    c["type 2 + 2^32"] = (prop([ent()]).replace(b"\x08\x02", b"\x08\x82\x80\x80\x80\x10", 1), RW.OK)
    c["entry type 1 + 2^32"] = (prop([ent(b"\xff", (1 << 32) + 1)]), RW.CONF_CHANGE)
    c["nil Data"] = (prop([ent(None), ent(b"")]), RW.OK)
    c["empty V1 is no leave"] = (prop([ent(b"", RW.ENTRY_CONF_CHANGE)]), RW.OK)
    c["nil V2 leaves"] = (prop([ent(None, RW.ENTRY_CONF_CHANGE_V2)]), RW.OK)
    c["conf change third of four"] = (prop([ent(b"a"), ent(b"bb"), ent(v2, 2), ent(b"c")]), RW.OK)
    c["two conf changes"] = (prop([ent(marshal_cc(1, 0, 2), 1), ent(v2, 2)]), RW.CONF_CHANGE)
    c["V2 truncated"] = (prop([ent(v2[:-1], 2)]), RW.CONF_CHANGE)
    c["V1 wrong wiretype"] = (prop([ent(b"\x0a\x00", 1)]), RW.CONF_CHANGE)
    c["V2 change past its end"] = (prop([ent(b"\x12\x05\x08\x00", 2)]), RW.CONF_CHANGE)
    c["V2 end group"] = (prop([ent(b"\x0c", 2)]), RW.CONF_CHANGE)
    c["no entries"] = (prop([]), RW.ENTRIES)
    c["commit between entries"] = (between_entries(ent(b"a"), ent(b"b")), RW.ENTRIES)
    c["prop with a term"] = (prop([ent()], term=7), RW.TERM)
    c["read with a term"] = (read(9, term=1), RW.TERM)
    c["read without entry"] = (W.marshal_message(type=15, context=b"12345678"), RW.CTX)
    c["read with two entries"] = (W.marshal_message(type=15, entries=[ent(b"12345678")] * 2), RW.CTX)
    c["read of seven bytes"] = (read(b"1234567"), RW.CTX)
    c["read of zeros"] = (read(bytes(8)), RW.CTX)
    c["resp of nine bytes"] = (read_resp(b"123456789", 5), RW.CTX)
    c["read entries apart"] = (between_entries(ent(b"12345678"), ent(b"87654321"), 15), RW.CTX)
    c["repeated Data"] = (W.marshal_message(type=15, entries=[ent(b"bad") + b"\x22\x08ABCDEFGH"]), RW.OK)
    return c


def corruptions():
    """name -> bytes that do not unmarshal (a MsgProp with a V2 conf change, broken)."""
    good = prop([ent(b"x"), ent(marshal_cc_v2(0, [(0, 3)]), 2)], frm=2)
    at = good.index(b"\x3a")
    c = {}
    c["varint of 10 continuation bytes"] = b"\x08\x02\x20" + b"\xff" * 10 + b"\x01" + good[2:]
    c["end-group tag"] = good[:at] + b"\x3c" + good[at:]
    c["entry running past the message"] = good[:at + 1] + bytes([len(good)]) + good[at + 2:]
    c["entry Data with wiretype 0"] = good[:at + 8] + b"\x20" + good[at + 9:]
    assert good[at + 8] == 0x22 and all(not W.decode_message(b)[0] for b in c.values())
    return c


def _one(r, g, what):
    """One message of class ``what`` for group g."""
    mem = members(g) if g < G else []
    frm = r.choice([0] + mem + [rand_u64(r) & ~1]) if mem else rand_u64(r)
    snap = r.choice((W.EMPTY_SNAPSHOT, b"\x12\x00"))
    kw = dict(to=rand_u64(r), snapshot=snap, reject=r.random() < 0.2)
    if what == "prop":
        ents = [ent(bytes(r.randrange(40)), 0, rand_u64(r), rand_u64(r)) for _ in range(r.choice((1, 1, 2, 3)))]
        if r.random() < 0.25:
            cc = r.choice((ent(marshal_cc(rand_u64(r), r.randrange(4), rand_u64(r), b"c"), 1),
                           ent(marshal_cc_v2(r.randrange(3), [(r.randrange(4), rand_u64(r))] * r.randrange(1, 4)), 2),
                           ent(marshal_cc_v2(), 2)))
            ents.insert(r.randrange(len(ents) + 1), cc)
        return prop(ents, frm=frm, index=rand_u64(r), commit=rand_u64(r), **kw)
    if what == "read":
        return read(rand_u64(r) | 1, frm=frm, context=r.choice((None, b"ignored")), **kw)
    if what == "transfer":
        return transfer(r.choice(mem + [rand_u64(r) & ~1]) if mem else 5, term=r.choice((0, 0, rand_u64(r))), **kw)
    if what == "resp":
        return read_resp(rand_u64(r) | 1, rand_u64(r), frm=rand_u64(r), term=rand_u64(r), **kw)
    if what == "other":
        return W.marshal_message(type=r.choice(OTHER_TYPES), frm=rand_u64(r), term=rand_u64(r),
                                 entries=[ent(b"12345678")] if r.random() < 0.5 else (), **kw)
    if what == "term":
        return r.choice((prop([ent()], frm=frm, term=rand_u64(r) | 1, **kw), read(rand_u64(r) | 1, frm=frm, term=1, **kw)))
    if what == "entries":
        return r.choice((prop([], frm=frm, **kw), between_entries(ent(b"a"), ent(bytes(r.randrange(9))))))
    if what == "ccbad":
        v2 = marshal_cc_v2(1, [(0, rand_u64(r))])
        return prop(r.choice(([ent(v2[:-1], 2)], [ent(b"q"), ent(v2, 2), ent(marshal_cc(1, 1, 1), 1)],
                              [ent(b"\x10\xff", 1)])), frm=frm, **kw)
    if what == "ctx":
        return r.choice((read(bytes(8), frm=frm, **kw), read(b"short", frm=frm, **kw),
                         W.marshal_message(type=15, frm=frm, **kw), read_resp(b"", 3, frm=frm, **kw)))
    raise AssertionError(what)


@functools.lru_cache(maxsize=None)
def base_batch(n=M, seed=SEED):
    """n messages (bytes) and their groups: three in sixteen are proposals,
    three reads, two transfers, and one each a response, another type, a
    special case, a corruption, a request with a term, a proposal whose
    entries are not taken, a bad conf change, and a bad context or a group
    >= G in turn."""
    r = random.Random(seed * 7919 + n)
    special = [b for b, _ in special_cases().values()]
    bad = list(corruptions().values())
    lanes = ("prop", "read", "transfer", "prop", "read", "resp", "prop", "transfer", "read", "other",
             "term", "special", "entries", "ccbad", "bad", "far")
    msgs, grp, ks, kb = [], [], 0, 0
    for i in range(n):
        g = r.randrange(G)
        lane = lanes[i % 16]
        if lane == "special":
            msgs.append(special[ks % len(special)])
            ks += 1
        elif lane == "bad":
            msgs.append(bad[kb % len(bad)])
            kb += 1
        elif lane == "far" and i // 16 % 2:
            msgs.append(_one(r, g, "ctx"))
        elif lane == "far":
            g = G + r.randrange(5)
            msgs.append(_one(r, g, r.choice(("prop", "read", "transfer", "resp"))))
        else:
            msgs.append(_one(r, g, lane))
        grp.append(g)
    return tuple(msgs), tuple(grp)


def assert_mixture(want, n):
    """The restatement's view of a batch, as the issue sets it: at least 5 %
    each of taken (OK) proposals, reads and transfers; at least 1 % each of
    UNMARSHAL, TERM, CTX, ENTRIES, CONF_CHANGE and DEFERRED."""
    ok = want["status"] == RW.OK
    for kind in (RW.RQ_PROP, RW.RQ_READ, RW.RQ_TRANSFER):
        assert 20 * int((ok & (want["kind"] == kind)).sum()) >= n, (kind, n)
    for st in (RW.UNMARSHAL, RW.TERM, RW.CTX, RW.ENTRIES, RW.CONF_CHANGE, RW.DEFERRED):
        assert 100 * int((want["status"] == st).sum()) >= n, (st, n)
    if n >= 256:
        assert {RW.TYPE, RW.GROUP} <= set(want["status"].tolist())
        assert {RW.SLOT_LOCAL, RW.SLOT_NONE, 0, 1} <= set(want["slot"][want["kind"] == RW.RQ_READ].tolist())
        assert (ok & (want["kind"] == RW.RQ_READ_RESP)).any() and want["cc_leave"].any()


# ------------------------------------------------------------- buffers ---

class Guarded:
    """The outputs of one call.  Each is n elements inside a marker-filled
    buffer of 3 + n + 5: an odd element offset, guards on both sides."""
    FRONT, BACK = 3, 5

    def __init__(self, n_msgs, n_groups, max_reads, stats0=None):
        self.M, self.G, self.R = n_msgs, n_groups, max_reads
        self.bigs = {}
        t = self._col
        msg = [t(k, n_msgs, dt) for k, dt in RW.COLUMNS]
        d = {k: t(k, n_groups, dt) for k, dt in RW.DENSE}
        d["rd_ctx"] = t("rd_ctx", max_reads * n_groups, np.uint64)
        d["rd_from"] = t("rd_from", max_reads * n_groups, np.uint8)
        rin = RequestInbox(max_reads, d["n_reads"], d["rd_ctx"], d["rd_from"], d["xf_from"], d["xf_term"])
        pin = ProposeInbox(d["action"], d["n_ents"], d["g_payload"], d["g_cc_at"], d["g_cc_payload"])
        self.stats0 = np.arange(RW.STAT_COUNT, dtype=np.uint64) * 11 if stats0 is None else stats0
        self.stats = dev(self.stats0)
        self.out = wire.RequestIngest(*msg, rin, pin, d["gflags"])

    def _col(self, name, n, dt):
        es = np.dtype(dt).itemsize
        n1 = max(n, 1)
        big = torch.full(((self.FRONT + n1 + self.BACK) * es,), FILL, dtype=torch.uint8, device=DEV)
        self.bigs[name] = (big, n, np.dtype(dt))
        return big[self.FRONT * es:(self.FRONT + n1) * es].view(_SIGNED[np.dtype(dt)])

    def host(self, name):
        """(the n elements, everything around them) of an output."""
        big, n, dt = self.bigs[name]
        a = big.cpu().numpy().view(dt)
        return a[self.FRONT:self.FRONT + n], np.concatenate([a[:self.FRONT], a[self.FRONT + n:]])

    def check(self, want):
        """Bit-exact against request_wire_ref.ingest, and the marker wherever
        nothing is to be written."""
        torch.cuda.synchronize()
        for name in self.bigs:
            _, guard = self.host(name)
            assert (guard == MARKER[guard.dtype.itemsize]).all(), f"guards of {name}"
        for name, _ in RW.COLUMNS + RW.DENSE:
            got, _ = self.host(name)
            assert np.array_equal(got, want[name]), (name, np.nonzero(got != want[name])[0][:8])
        ctx = np.full(self.R * self.G, MARKER[8], np.uint64)
        frm = np.full(self.R * self.G, MARKER[1], np.uint8)
        for (k, g), (c, f) in want["rd"].items():
            ctx[k * self.G + g], frm[k * self.G + g] = c, f
        assert np.array_equal(self.host("rd_ctx")[0], ctx), "rd_ctx"
        assert np.array_equal(self.host("rd_from")[0], frm), "rd_from"
        stats = self.stats.cpu().numpy().view(np.uint64)
        assert np.array_equal(stats, self.stats0 + want["stats"]), (stats - self.stats0, want["stats"])


def run(msgs, grp, n_groups=G, max_reads=1, concat=False, off=None, nbytes=None, residue=None,
        cfg=None):
    """One guarded call over the messages (``off`` / ``nbytes`` override the
    packed ones: caller errors) checked against the restatement; returns
    (want, Guarded)."""
    buf, packed = pack(msgs)
    off = packed if off is None else off
    nbytes = len(buf) if nbytes is None else nbytes
    n = len(grp)
    goff, gids = config(n_groups) if cfg is None else cfg
    want = RW.ingest(buf, nbytes, off, grp, goff, gids, max_reads, concat)
    b = Bytes(buf, residue)
    g = Guarded(n, n_groups, max_reads)
    # (dev() never returns an empty tensor: the slice keeps M = 0 a batch of none)
    got = wire.ingest_requests(b.buf, nbytes, dev(off), dev(np.array(grp, np.uint32))[:n], dev(goff),
                               dev(gids), max_reads=max_reads, concat=concat, out=g.out, stats=g.stats)
    assert got is g.out
    g.check(want)
    assert (b.big[:GUARD] == FILL).all() and (b.big[-GUARD:] == FILL).all()
    return want, g
