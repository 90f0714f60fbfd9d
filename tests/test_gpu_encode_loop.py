"""The raft loop closed in both directions on the device, at 257 three-node
groups (the cluster of tests/test_gpu_requests_loop.py: node j holds slot j
and raft ID j + 1, node 0 leads, node 1 lags by an entry in every other
group), every call beside its restatement:

  requests queue a read per group -> the tick -> its heartbeats through
  qb_dev_encode_slots -> the bytes decoded on the CPU into the follower step's
  inbox -> the responses through qb_dev_encode_messages -> qb_dev_ingest_messages
  on the device bytes -> qb_dev_leader_step on the ingested records -> its
  qb_msg_out list through qb_dev_encode_msg_out: a MsgApp with QB_ENC_ENTRIES
  for the lagging peer and, from the pending read of a peer, a
  MsgReadIndexResp whose entry carries the request id."""
import numpy as np
import pytest
import torch

from etcd_amd.quorum import encode, leader as ql, tick as qt, wire
from oracle import leader_ref as L, raftpb_ref as W
from tests import encode_ref as E, follower_ref as F, request_ref as R
from tests import test_gpu_requests_loop as RL

pytestmark = pytest.mark.gpu
G, TERM, DEV = RL.G, RL.TERM, RL.DEV
NO = R.NO_SLOT


def host(t, dt, n=None):
    return ql._to_np(t, dt, n)


def same_layout(got, want, M):
    """A wrapper's 5-tuple against encode_ref.finish's layout."""
    b, moff, st, at, nb = got
    torch.cuda.synchronize()
    n = int(want["nbytes"])
    assert int(nb[0]) == n and want["written"] == n
    assert host(b, np.uint8, n).tobytes() == want["bytes"].tobytes()
    assert np.array_equal(host(moff, np.uint64, M + 1), want["msg_off"])
    assert np.array_equal(host(st, np.uint8, M), want["status"])
    w = want["ent_at"]
    assert np.array_equal(host(at, np.uint32, M)[w >= 0], w[w >= 0])
    return host(b, np.uint8, n).tobytes(), want["msg_off"].astype(np.int64)


class Cluster(RL.Cluster):
    """The requests loop's cluster with the device outputs of the tick and of
    the leader step kept, and the leader step fed what the ingest decoded."""
    inbox = None

    def tick(self):
        lg = self.runs[0].lg
        real = lg.tick

        def spy(*a, **k):
            self.tick_res = real(*a, **k)
            return self.tick_res
        lg.tick = spy
        try:
            return super().tick()
        finally:
            del lg.tick

    def leader_step(self, resps):
        lg = self.runs[0].lg
        real = lg.step

        def ingested(ib, *a, **k):
            M = ib.M
            assert self.inbox.M == M
            for col, dt in (("group", np.uint32), ("flags", np.uint8), ("index", np.uint64),
                            ("term", np.uint64), ("hint", np.uint64), ("log_term", np.uint64)):
                assert np.array_equal(host(getattr(self.inbox, col), dt, M),
                                      host(getattr(ib, col), dt, M)), col
            return real(self.inbox, *a, **k)
        lg.step = ingested
        try:
            return super().leader_step(resps)
        finally:
            del lg.step


def test_the_loop_closes_in_both_directions():
    rng = np.random.default_rng(21)
    logs = RL.make_logs(rng)
    lag = [g % 2 for g in range(G)]
    c = Cluster(logs, lag)
    lead = c.runs[0]
    ctx = [(1 << 56) + 1000 + g for g in range(G)]
    frm = [2 if g % 3 == 0 else NO for g in range(G)]
    reads = [[] if g % 7 == 6 else [(ctx[g], frm[g])] for g in range(G)]
    c.requests(reads, None)

    # 1. the tick: every leader beats, with the newest pending context
    beat = c.tick()
    assert beat == [ctx[g] if reads[g] else 0 for g in range(G)]
    tr = c.tick_res

    # 2. its heartbeats through the slot form
    S = lead.lg.S
    off = lead.off
    ids = np.tile(np.arange(1, 4, dtype=np.uint64), G)
    self_id = np.ones(G, np.uint64)
    term = host(lead.lg.t["term"], np.uint64, G)
    groups = encode.EncodeGroups(lead.lg.t["off"], ql._to_dev(ids, np.uint64, DEV),
                                 ql._to_dev(self_id, np.uint64, DEV), lead.lg.t["term"], S)
    want = E.finish(E.slots(G, off, ids, self_id, term, S, host(tr.tflags, np.uint8, G),
                            qt.TFLAG_BEAT, E.MSG_HEARTBEAT,
                            {"commit": host(tr.hb_commit, np.uint64, S),
                             "ctx_g": host(tr.hb_ctx, np.uint64, G)}))
    assert (want["status"].reshape(G, 3) == [E.NONE, E.OK, E.OK]).all()
    by, mo = same_layout(encode.encode_slots(groups, gflags=tr.tflags, gmask=qt.TFLAG_BEAT,
                                             cols={"commit": tr.hb_commit, "ctx_g": tr.hb_ctx}),
                        want, S)

    # 3. the bytes decoded on the CPU are the follower step's inbox
    resp = {"type": [], "to": [], "from": [], "term": [], "context": [], "group": []}
    acks = []
    for j in (1, 2):
        recs = []
        for g in range(G):
            s = 3 * g + j
            ok, f = W.decode_message(by[mo[s]:mo[s + 1]])
            assert ok and (f[1], f[2], f[3], f[4]) == (E.MSG_HEARTBEAT, j + 1, 1, TERM)
            c8 = int.from_bytes(f.get(12, b""), "big") if 12 in f else 0
            assert c8 == beat[g] and 7 not in f
            recs.append((g, F.Rec(F.HEARTBEAT, f[3], f[4], f[8], c8)))
        rt, _ = c.follower_step(j, recs)
        assert all(x == F.MSG_HEARTBEAT_RESP for x in rt)
        # the host answers with the heartbeat's context (raft.go:1515)
        acks += [(g, L.Inbound(L.IN_HEARTBEAT_RESP, j, TERM, m.aux)) for g, m in recs]
    acks.sort(key=lambda x: x[0])
    for g, m in acks:
        for k, v in (("type", 9), ("to", 1), ("from", m.slot + 1), ("term", m.term),
                     ("context", m.index), ("group", g)):
            resp[k].append(v)

    # 4. the responses through the general columns, 5. ingested on the device
    M = len(acks)
    cols = {k: np.array(resp[k], np.uint8 if k == "type" else np.uint64)
            for k in ("type", "to", "from", "term", "context")}
    want = E.finish(E.columns(cols, M))
    assert (want["status"] == E.OK).all()
    dcols = {k: ql._to_dev(v, v.dtype.type, DEV) for k, v in cols.items()}
    got = encode.encode_columns(dcols, M=M)
    same_layout(got, want, M)
    b, moff, _, _, nb = got
    grp = ql._to_dev(np.array(resp["group"], np.uint32), np.uint32, DEV)
    c.inbox, wst, mtype = wire.ingest(b, int(nb[0]), moff, grp, groups.off, groups.ids)
    torch.cuda.synchronize()
    assert int(wst.max()) == wire.WIRE_OK and bool((mtype == 9).all())

    # 6. the leader step on the ingested records, 7. its list through the list form
    msgs = c.leader_step(acks)
    out = lead.lg._out
    cap = out["msgs"].numel() // encode.MSG_OUT_BYTES
    total = int(out["total"].cpu()[0])
    assert total == sum(len(m) for m in msgs) and total < cap
    recs = out["msgs"].cpu().numpy().view(ql.MSG_DTYPE)
    lay = E.msg_out(G, off, ids, self_id, term, recs, cap, total)
    want = E.finish(lay)
    by, mo = same_layout(encode.encode_msg_out(groups, out["msgs"], cap, out["total"]), want, cap)
    assert set(want["status"][:total].tolist()) == {E.OK, E.ENTRIES, E.NONE}
    assert (want["status"][total:] == E.NONE).all()
    seen = {"app": 0, "resp": 0, "local": 0}
    for i in range(total):
        g, t = int(recs[i]["group"]), int(recs[i]["type"])
        if t == L.READ_STATE:
            assert want["status"][i] == E.NONE and frm[g] == NO
            seen["local"] += 1
            continue
        ok, f = W.decode_message(by[mo[i]:mo[i + 1]])
        assert ok and (f[3], f[4]) == (1, TERM)
        if t == L.MSG_APP:
            assert lag[g] and f[2] == 2 and want["status"][i] == (E.ENTRIES if recs[i]["aux"] else E.OK)
            assert 7 not in f and (f[6], f[5], f[8]) == tuple(int(recs[i][k]) for k in
                                                            ("index", "log_term", "commit"))
            seen["app"] += int(want["status"][i] == E.ENTRIES)
        else:
            assert t == L.MSG_READ_INDEX_RESP and frm[g] == 2 and f[2] == 3
            assert f[7] == [{1: 0, 2: 0, 3: 0, 4: ctx[g].to_bytes(8, "big")}] and 12 not in f
            assert f[6] == int(recs[i]["index"])
            seen["resp"] += 1
    assert seen["app"] > 0 and seen["resp"] > 0 and seen["local"] > 0
