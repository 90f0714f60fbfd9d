"""Inputs, device buffers and comparisons shared by the qb_dev_encode_* GPU
tests: seeded batches that reach every path of the encoder (asserted on the
CPU when they are built), outputs pre-filled with a marker inside a guarded
buffer, and the bit-exact comparison against tests/encode_ref.py.

Test infrastructure."""
from __future__ import annotations

import functools
import random

import numpy as np
import torch

from etcd_amd.quorum import encode
from etcd_amd.quorum.leader import MSG_DTYPE
from tests import encode_ref as E

DEV = "cuda"
FILL = 0x5A
GUARD = 64
U64_COLS = ("to", "from", "term", "log_term", "index", "commit", "reject_hint")
_SIGNED = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint32): np.int32,
           np.dtype(np.uint64): np.int64}


def dev(a):
    """A host array as a device tensor of the same bytes (never empty)."""
    a = np.ascontiguousarray(a)
    if a.size == 0:
        a = np.zeros(1, a.dtype)
    return torch.from_numpy(a.view(_SIGNED[a.dtype]).copy()).to(DEV)


def rand_u64(r):
    """0, or a value of a uniformly drawn bit length 1..64: every varint
    length 1..10 comes up about equally often."""
    k = r.randint(0, 64)
    return 0 if k == 0 else (r.getrandbits(k) | (1 << (k - 1)))


TYPES = (0, 7, 3, 3, 4, 4, 8, 9, 9, 14, 15, 16, 5, 6, 2, 128, 255, 1)


@functools.lru_cache(maxsize=None)
def column_batch(M, seed=1):
    """The general form's columns (numpy) for M messages."""
    r = random.Random(seed * 7919 + M)
    cols = {"type": np.array([r.choice(TYPES) for _ in range(M)], np.uint8)}
    for k in U64_COLS:
        cols[k] = np.array([rand_u64(r) for _ in range(M)], np.uint64)
    cols["context"] = np.array([rand_u64(r) if r.random() < 0.5 else 0 for _ in range(M)], np.uint64)
    cols["reject"] = np.array([r.choice((0, 0, 1, 2)) for _ in range(M)], np.uint8)
    cols["n_entries"] = np.array([r.choice((0, 0, 0, 1, 5)) for _ in range(M)], np.uint64)
    return cols


def assert_columns_cover(cols, M):
    """The batch reaches every status the columns can give, every varint
    length of every u64 field, both read types, Context nil and set, Reject 0
    and 1."""
    recs = E.columns(cols, M)
    assert {st for st, _ in recs} == {E.OK, E.ENTRIES, E.HOST, E.NONE}
    ms = [m for _, m in recs if m is not None]
    for k in ("to", "frm", "term", "log_term", "index", "commit", "reject_hint"):
        assert {E.sov(m[k]) for m in ms} == set(range(1, 11)), k
    assert {E.sov(m["type"]) for m in ms} == {1, 2}
    for t in (15, 16):
        assert {m["ctx"] != 0 for m in ms if m["type"] == t} == {False, True}, t
    assert {m["ctx"] != 0 for m in ms if m["type"] not in (15, 16)} == {False, True}
    assert {m["reject"] for m in ms} == {0, 1}


@functools.lru_cache(maxsize=None)
def group_table(G=300, seed=3):
    """G groups of 1..7 slots: off, ascending ids, self_id (one group in nine
    has its own slot absent), term."""
    r = random.Random(seed)
    n = [1 + (g * 5 + r.randint(0, 6)) % 7 for g in range(G)]
    off = np.zeros(G + 1, np.uint32)
    off[1:] = np.cumsum(n)
    ids, self_id = [], []
    for g in range(G):
        members = set()
        while len(members) < n[g]:
            members.add(rand_u64(r) or 1)
        members = sorted(members)
        ids += members
        self_id.append(members[r.randrange(n[g])] if g % 9 else (1 << 63) + 12345 + g)
    term = np.array([rand_u64(r) for _ in range(G)], np.uint64)
    assert set(n) == set(range(1, 8))
    return G, off, np.array(ids, np.uint64), np.array(self_id, np.uint64), term


@functools.lru_cache(maxsize=None)
def list_batch(M, seed=5):
    """qb_msg_out records over group_table(): every type the front end forms
    and refuses, groups >= G, slots outside their group, local ReadStates."""
    G, off, _, _, _ = group_table()
    r = random.Random(seed * 104729 + M)
    recs = np.zeros(max(M, 1), MSG_DTYPE)
    for i in range(M):
        g = r.randrange(G) if r.random() < 0.95 else G + r.randrange(4)
        ns = int(off[g + 1] - off[g]) if g < G else 3
        to = r.randrange(ns) if r.random() < 0.9 else r.choice((ns, 7, 0xFF))
        t = r.choice((3, 3, 3, 8, 14, 16, 16, 7, 0, 255, 5, 4))
        aux = r.choice((0, 0, 1, 3, rand_u64(r)))
        recs[i] = (rand_u64(r), rand_u64(r), rand_u64(r), aux, g, to, t, 0)
    return recs


def assert_list_covers(recs, M, total):
    G, off, ids, self_id, term = group_table()
    out = E.msg_out(G, off, ids, self_id, term, recs, M, total)
    assert {st for st, _ in out} == {E.OK, E.ENTRIES, E.HOST, E.NONE}
    ms = [m for _, m in out if m is not None]
    assert {m["type"] for m in ms} == {3, 8, 14, 16}
    assert {m["ctx"] != 0 for m in ms if m["type"] == 16} == {False, True}
    assert (recs["group"][:M] >= G).any() and (recs["to"][:M] == 0xFF).any()


@functools.lru_cache(maxsize=None)
def slot_columns(seed=11):
    """Slot-aligned columns over group_table() (+ 5 slots no group covers)."""
    G, off, _, _, _ = group_table()
    S = int(off[-1]) + 5
    r = random.Random(seed)
    return {"type": np.array([r.choice((3, 3, 0, 7, 8, 14, 16, 5, 255)) for _ in range(S)], np.uint8),
            "index": np.array([rand_u64(r) for _ in range(S)], np.uint64),
            "log_term": np.array([rand_u64(r) for _ in range(S)], np.uint64),
            "commit": np.array([rand_u64(r) for _ in range(S)], np.uint64),
            "n_entries": np.array([r.choice((0, 0, 2)) for _ in range(S)], np.uint64),
            "commit_g": np.array([rand_u64(r) for _ in range(G)], np.uint64),
            "ctx_g": np.array([rand_u64(r) if g % 3 else 0 for g in range(G)], np.uint64),
            "gflags": np.array([r.choice((0, 2, 3, 4)) for _ in range(G)], np.uint8)}


class Guarded:
    """The outputs of one call, every one pre-filled with the marker; bytes is
    an interior slice of a larger buffer, at an odd address, with GUARD marker
    bytes in front of and behind it."""

    def __init__(self, M, cap, stats0=None):
        self.M, self.cap = M, cap
        self.big = torch.full((GUARD + 1 + max(cap, 1) + GUARD,), FILL, dtype=torch.uint8, device=DEV)
        self.start = GUARD + (1 if (self.big.data_ptr() + GUARD) % 2 == 0 else 0)
        b = self.big[self.start:self.start + max(cap, 1)]
        assert b.data_ptr() % 2 == 1
        f = lambda n, dt: torch.full((n * torch.empty(0, dtype=dt).element_size(),), FILL,  # noqa: E731
                                     dtype=torch.uint8, device=DEV).view(dt)
        self.stats0 = np.arange(5, dtype=np.uint64) * 7 if stats0 is None else stats0
        self.out = encode.EncodeOut(b, cap, f(M + 3, torch.int64), f(M + 2, torch.uint8),
                                    f(M + 2, torch.int32), f(2, torch.int64), dev(self.stats0))

    def residue(self):
        return self.out.bytes.data_ptr() % 16

    def check(self, want):
        """Bit-exact against encode_ref.finish's layout, and the marker
        wherever nothing is to be written."""
        torch.cuda.synchronize()
        M, cap, o = self.M, self.cap, self.out
        big = self.big.cpu().numpy()
        got = big[self.start:self.start + cap]
        n = want["written"]
        assert n <= cap and want["nbytes"] >= n
        assert got[:n].tobytes() == want["bytes"].tobytes()
        assert (got[n:] == FILL).all(), "bytes behind the written ones"
        assert (big[:self.start] == FILL).all() and (big[self.start + cap:] == FILL).all(), "guards"
        off = o.msg_off.cpu().numpy().view(np.uint64)
        assert np.array_equal(off[:M + 1], want["msg_off"])
        assert (off[M + 1:] == 0x5A5A5A5A5A5A5A5A).all()
        st = o.status.cpu().numpy()
        assert np.array_equal(st[:M], want["status"])
        assert (st[M:] == FILL).all()
        at = o.ent_at.cpu().numpy().view(np.uint32).astype(np.int64)
        assert np.array_equal(at[:M], np.where(want["ent_at"] >= 0, want["ent_at"], 0x5A5A5A5A))
        assert (at[M:] == 0x5A5A5A5A).all()
        nb = o.nbytes.cpu().numpy().view(np.uint64)
        assert nb[0] == want["nbytes"] and nb[1] == 0x5A5A5A5A5A5A5A5A
        stats = o.stats.cpu().numpy().view(np.uint64)
        assert np.array_equal(stats, self.stats0 + want["stats"])


def groups_dev(S=None):
    G, off, ids, self_id, term = group_table()
    S = int(off[-1]) if S is None else S
    ids_d = np.concatenate([ids, np.full(max(S - len(ids), 0), 77, np.uint64)])
    return encode.EncodeGroups(dev(off), dev(ids_d), dev(self_id), dev(term), S)


def cols_dev(cols, M=None):
    return {k: dev(v if M is None else v[:M]) for k, v in cols.items() if v is not None}
