"""Inputs, device buffers and comparisons shared by the qb_dev_ingest_follower
GPU tests: a seeded mixture of the five device kinds, the host types, every
MsgApp case and the corruptions (its coverage asserted on the CPU with the
restatement alone), the byte buffer and every output inside marker-filled
guarded buffers, and the bit-exact comparison against
tests/follower_wire_ref.py.

Test infrastructure."""
from __future__ import annotations

import functools
import random

import numpy as np
import torch

from etcd_amd.quorum import wire
from etcd_amd.quorum.follower import FollowerAppInbox, FollowerInbox
from oracle import raftpb_ref as W
from tests import follower_wire_ref as FW
from tests.encode_pack import rand_u64

DEV = "cuda"
FILL = 0x5A
GUARD = 64
G = 300
TOP = (1 << 64) - 1
BRIEF_SNAPSHOT = b"\x12\x00"  # an empty Metadata: 4a 02 12 00 with the key
HOST_TYPES = (0, 1, 2, 4, 6, 7, 9, 10, 11, 12, 13, 15, 16, 18, 19, 200, 264)
_SIGNED = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint32): torch.int32,
           np.dtype(np.uint64): torch.int64}


def f7(entries):
    """(term, index, data) -> the encoded Entry bodies of marshal_message."""
    return [W.marshal_entry(t, i, 0, d) for t, i, d in entries]


def app(r, index, terms, data=lambda k: b"x", **kw):
    """A MsgApp whose entries follow Index with the given terms."""
    ents = [(t, (index + 1 + k) & TOP, data(k)) for k, t in enumerate(terms)]
    return W.marshal_message(type=3, to=rand_u64(r), frm=rand_u64(r), term=rand_u64(r),
                             log_term=rand_u64(r), index=index, commit=rand_u64(r),
                             entries=f7(ents), **kw)


def app_cases(r):
    """name -> bytes of every MsgApp case of the issue's list."""
    idx = lambda: rand_u64(r) >> 1  # noqa: E731
    c = {}
    c["no entries"] = app(r, idx(), [])
    c["one entry"] = app(r, idx(), [7])
    c["one run of 200"] = app(r, idx(), [9] * 200)
    c["nine runs"] = app(r, idx(), [1, 1, 2, 3, 3, 3, 4, 5, 6, 7, 7, 8, 9])
    c["alternating terms"] = app(r, idx(), [4, 5] * 6)
    c["term 0"] = app(r, idx(), [0, 0, 3])
    c["wrap"] = app(r, TOP - 1, [2, 2, 3])
    c["data sizes"] = app(r, idx(), [6, 6, 6, 8], data=lambda k: (b"", b"d", bytes(3000), None)[k])
    c["brief snapshot"] = app(r, idx(), [5, 6], snapshot=BRIEF_SNAPSHOT)
    i0 = idx()
    e = lambda t, i: (t, i, b"y")  # noqa: E731
    head = dict(type=3, to=2, frm=rand_u64(r), term=rand_u64(r), log_term=3, index=i0, commit=i0)
    c["gap"] = W.marshal_message(entries=f7([e(3, i0 + 1), e(3, i0 + 3)]), **head)
    c["repeated index"] = W.marshal_message(entries=f7([e(3, i0 + 1), e(3, i0 + 1)]), **head)
    c["first index off"] = W.marshal_message(entries=f7([e(3, i0 + 2)]), **head)
    pre = b"".join(W._key(f, 0) + W.varint(v) for f, v in ((1, 3), (2, 2), (3, 77), (4, 9), (5, 3), (6, i0)))
    e1, e2 = (b"\x3a" + W.varint(len(x)) + x for x in f7([e(3, i0 + 1), e(4, i0 + 2)]))
    tail = b"\x4a" + W.varint(len(W.EMPTY_SNAPSHOT)) + W.EMPTY_SNAPSHOT + b"\x50\x00\x58\x00"
    assert W.decode_message(pre + e1 + e2 + b"\x40\x05" + tail)[0]
    c["commit between entries"] = pre + e1 + b"\x40\x05" + e2 + tail
    return c


def corruptions(r):
    """name -> bytes that do not unmarshal (a MsgApp with two entries, broken)."""
    good = W.marshal_message(type=3, to=1, frm=2, term=3, log_term=3, index=1000, commit=7,
                             entries=f7([(3, 1001, b"x"), (4, 1002, b"y")]))
    at = good.index(b"\x3a")
    assert at == 13 and FW.decode(good, 0)["status"] == FW.OK
    entry_len = good[at + 1]
    c = {}
    c["varint of 10 continuation bytes"] = b"\x08\x03\x20" + b"\xff" * 10 + b"\x01" + good[2:]
    # the first entry's Term key (0x10) with wiretype 2
    term_key = good.index(b"\x10", at + 2)
    assert term_key < at + 2 + entry_len
    c["entry with a wrong wiretype"] = good[:term_key] + b"\x12" + good[term_key + 1:]
    c["end-group tag"] = good[:at] + b"\x3c" + good[at:]
    c["entry running past the message"] = good[:at + 1] + bytes([len(good)]) + good[at + 2:]
    return c


def device_kind(r, i, context="usual"):
    """Message i of the rotation over the five device kinds."""
    t = (8, 5, 17, 14, 3)[i % 5]
    if t == 3:
        n = r.choice((0, 1, 2, 3, 5))
        terms = sorted(r.choice((1, 2, 3, 1 << 40)) for _ in range(n))
        return app(r, rand_u64(r) >> 1, terms, snapshot=r.choice((W.EMPTY_SNAPSHOT, BRIEF_SNAPSHOT)))
    ctx = None
    if t == 8 and r.random() < 0.5:
        ctx = (rand_u64(r) | 1).to_bytes(8, "big")
    if t in (5, 17):
        ctx = r.choice((None, None, FW.CAMPAIGN_TRANSFER, b""))
    if context == "odd":
        ctx = r.choice((bytes(8), b"CampaignTransfes", b"12345", FW.CAMPAIGN_TRANSFER, b"", b"z" * 20))
    return W.marshal_message(type=t, to=rand_u64(r), frm=rand_u64(r), term=rand_u64(r),
                             log_term=rand_u64(r), index=rand_u64(r), commit=rand_u64(r),
                             reject=r.random() < 0.2, reject_hint=rand_u64(r), context=ctx,
                             snapshot=r.choice((W.EMPTY_SNAPSHOT, W.EMPTY_SNAPSHOT, BRIEF_SNAPSHOT)))


def host_kind(r):
    t = r.choice(HOST_TYPES)
    ents = f7([(1, 5, b"prop")]) if t in (2, 15, 16) else ()
    snap = W.marshal_snapshot(b"snap", 9, 2, W.marshal_conf_state((1, 2, 3))) if t == 7 else W.EMPTY_SNAPSHOT
    return W.marshal_message(type=t, to=rand_u64(r), frm=rand_u64(r), term=rand_u64(r),
                             index=rand_u64(r), entries=ents, snapshot=snap,
                             context=r.choice((None, b"12345678")))


@functools.lru_cache(maxsize=None)
def base_batch(M=1000, seed=1):
    """M messages (bytes) and their groups: five in eight rotate over the device
    kinds, one is a host type, one a MsgApp case or a corruption, one a device
    kind with an unusual context."""
    r = random.Random(seed * 7919 + M)
    special = list(app_cases(r).values()) + list(corruptions(r).values())
    msgs, k = [], 0
    for i in range(M):
        lane = i % 8
        if lane < 5:
            msgs.append(device_kind(r, i // 8 + lane))
        elif lane == 5:
            msgs.append(host_kind(r))
        elif lane == 6:
            msgs.append(special[k % len(special)])
            k += 1
        else:
            msgs.append(device_kind(r, i // 8, context="odd"))
    grp = [r.randrange(G) if r.random() < 0.9 else G + r.randrange(5) for _ in range(M)]
    return tuple(msgs), tuple(grp)


def pack(msgs):
    off = np.zeros(len(msgs) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    return b"".join(msgs), off


def assert_mixture(want, M):
    """The restatement's view of a batch: each of the five device kinds keeps
    an eighth of the messages with status OK (the rotation gives five lanes
    in eight to them, so a fifth each of those), and at least a fifth of each
    kind's own messages is OK; host types, every failing status and groups
    >= G are there."""
    ok = want["status"] == FW.OK
    kinds = want["flags"] & 7
    for t, kind in ((8, FW.FIN_HEARTBEAT), (5, FW.FIN_VOTE), (17, FW.FIN_PREVOTE),
                    (14, FW.FIN_TIMEOUT_NOW), (3, FW.FIN_APP)):
        n_ok = int((ok & (kinds == kind)).sum())
        assert 8 * n_ok >= M - 7, (t, n_ok, M)  # an eighth of the whole groups of eight
        assert 5 * n_ok >= int((want["msg_type"] == t).sum()), (t, n_ok)
    if M >= 256:
        assert set(want["status"].tolist()) == {FW.OK, FW.UNMARSHAL, FW.TYPE, FW.CTX, FW.ENTRIES}
        assert (want["group"][want["status"] != FW.UNMARSHAL] >= G).any()
        assert (want["flags"] & FW.FORCE).any()


def dev(a):
    a = np.ascontiguousarray(a)
    if a.size == 0:
        a = np.zeros(1, a.dtype)
    return torch.from_numpy(a.view({np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
                                   .get(a.dtype, a.dtype)).copy()).to(DEV)


class Bytes:
    """The batch's bytes inside a marker-filled buffer: GUARD marker bytes in
    front and behind, the first byte at address = ``residue`` mod 16 (default:
    an odd address)."""

    def __init__(self, buf: bytes, residue=None):
        n = len(buf)
        self.big = torch.full((GUARD + 16 + max(n, 1) + GUARD,), FILL, dtype=torch.uint8, device=DEV)
        base = self.big.data_ptr() + GUARD
        if residue is None:
            start = GUARD + (1 if base % 2 == 0 else 0)
        else:
            start = GUARD + (residue - base) % 16
        self.buf = self.big[start:start + max(n, 1)]
        if n:
            self.buf.copy_(torch.from_numpy(np.frombuffer(buf, np.uint8).copy()))
        self.nbytes = n
        assert residue is None and self.buf.data_ptr() % 2 == 1 or self.buf.data_ptr() % 16 == residue


class Guarded:
    """The outputs of one call.  Each is n elements inside a marker-filled
    buffer of 3 + n + 5: an odd element offset (the byte columns at an odd
    address, the wider ones off any 16-byte boundary), guards on both sides."""
    FRONT, BACK = 3, 5

    def __init__(self, M, cap, stats0=None):
        self.M, self.cap = M, cap
        self.bigs = {}
        t = self._col
        ib = FollowerInbox(t("group", M, np.uint32), t("flags", M, np.uint8), t("frm", M, np.uint64),
                           t("term", M, np.uint64), t("index", M, np.uint64), t("aux", M, np.uint64))
        ib._m = M
        app_ = FollowerAppInbox(t("commit", M, np.uint64), t("ent_off", M + 1, np.uint32),
                                t("ent_term", cap, np.uint64), t("ent_len", cap, np.uint32), cap)
        self.stats0 = np.arange(FW.STATUS_COUNT, dtype=np.uint64) * 11 if stats0 is None else stats0
        self.stats = dev(self.stats0)
        self.out = wire.FollowerIngest(ib, app_, t("status", M, np.uint8), t("msg_type", M, np.uint8),
                                       t("ent_pos", M, np.uint64), t("ent_bytes", M, np.uint32),
                                       t("ent_n", M, np.uint32), t("ent_total", 1, np.uint64))

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
        """Bit-exact against follower_wire_ref.ingest, and the marker wherever
        nothing is to be written."""
        torch.cuda.synchronize()
        M = self.M
        marker = {1: FILL, 4: 0x5A5A5A5A, 8: 0x5A5A5A5A5A5A5A5A}
        for name in self.bigs:
            _, guard = self.host(name)
            assert (guard == marker[guard.dtype.itemsize]).all(), f"guards of {name}"
        for name, _ in FW.COLUMNS:
            got, _ = self.host(name)
            assert np.array_equal(got, want[name][:M]), name
        off, _ = self.host("ent_off")
        assert np.array_equal(off, want["ent_off"])
        tot, _ = self.host("ent_total")
        assert int(tot[0]) == want["ent_total"]
        term = np.full(self.cap, marker[8], np.uint64)
        length = np.full(self.cap, marker[4], np.uint32)
        for i, runs in enumerate(want["runs"]):
            o = int(off[i])
            assert not runs or int(off[i + 1]) == o + len(runs) <= self.cap
            for k, (t, n) in enumerate(runs):
                term[o + k], length[o + k] = t, n
        assert np.array_equal(self.host("ent_term")[0], term), "ent_term"
        assert np.array_equal(self.host("ent_len")[0], length), "ent_len"
        stats = self.stats.cpu().numpy().view(np.uint64)
        assert np.array_equal(stats, self.stats0 + want["stats"]), (stats, want["stats"])


def run(msgs, grp, off=None, nbytes=None, ent_cap=None, residue=None):
    """One guarded call over the messages (``off`` / ``nbytes`` override the
    packed ones: caller errors) checked against the restatement; returns
    (want, Guarded)."""
    buf, packed = pack(msgs)
    off = packed if off is None else off
    nbytes = len(buf) if nbytes is None else nbytes
    M = len(grp)
    want = FW.ingest(buf, nbytes, off, grp, ent_cap)
    cap = want["ent_total"] if ent_cap is None else ent_cap
    b = Bytes(buf, residue)
    g = Guarded(M, cap)
    # (dev() never returns an empty tensor: the slice keeps M = 0 a batch of none)
    got = wire.ingest_follower(b.buf, nbytes, dev(off), dev(np.array(grp, np.uint32))[:M], G,
                               out=g.out, stats=g.stats)
    assert got is g.out
    g.check(want)
    assert (b.big[:GUARD] == FILL).all() and (b.big[-GUARD:] == FILL).all()
    return want, g
