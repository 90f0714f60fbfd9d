"""tests/test_gpu_encode_loop.py's loop at 257 three-node groups with the CPU
decode replaced: what the followers receive is decoded on the device by
qb_dev_ingest_follower and stepped from those columns as they are.

  the tick's heartbeats     encode_slots -> ingest_follower -> follower_step;
                            the responses -> encode_columns -> wire.ingest ->
                            the leader step;
  a proposal's bcastAppend  encode_slots with QB_ENC_ENTRIES -> the host splices
                            its entries at ent_at -> ingest_follower ->
                            follower_log_step -> the responses as above;
  a campaign's requests     encode_columns -> ingest_follower -> follower_step.

Every follower call runs on the ingested columns after they were found equal
to the inbox the same bytes give when decoded on the CPU (the existing loop's
way), and is compared with its restatement and the node's whole table by the
cluster of tests/test_gpu_requests_loop.py; every message comes back
QB_WIRE_OK, so nothing falls back to the host unnoticed."""
import contextlib

import numpy as np
import pytest
import torch

from etcd_amd.quorum import encode, follower as qf, leader as ql, propose as qp, tick as qt, wire
from oracle import leader_ref as L, raftpb_ref as W
from tests import campaign_ref as CR, encode_ref as E, follower_ref as F, follower_wire_ref as FW
from tests import propose_ref as PR, request_ref as R
from tests import test_gpu_encode_loop as EL, test_gpu_requests_loop as RL

pytestmark = pytest.mark.gpu
G, TERM, DEV = RL.G, RL.TERM, RL.DEV
NO = R.NO_SLOT
host, same_layout = EL.host, EL.same_layout
INBOX = (("group", np.uint32), ("flags", np.uint8), ("frm", np.uint64), ("term", np.uint64),
         ("index", np.uint64), ("aux", np.uint64))


def route(b, moff, sel):
    """The transport's part, on the device: the messages ``sel`` of a batch
    gathered into a buffer of their own -> (bytes, nbytes, msg_off)."""
    start = moff[sel]
    lens = moff[sel + 1] - start
    off = torch.zeros(sel.numel() + 1, dtype=torch.int64, device=b.device)
    off[1:] = torch.cumsum(lens, 0)
    total = int(off[-1])
    src = torch.repeat_interleave(start - off[:-1], lens) + torch.arange(total, device=b.device)
    return (b[src] if total else torch.zeros(1, dtype=torch.uint8, device=b.device)), total, off


def dev_u32(a):
    return ql._to_dev(np.asarray(a, np.uint32), np.uint32, DEV)


class Cluster(EL.Cluster):
    """The encode loop's cluster whose follower calls step what
    ingest_follower decoded (``fin``), once it equals the CPU-decoded inbox."""
    fin = None

    @contextlib.contextmanager
    def ingested(self, name):
        real = getattr(qf, name)

        def stepped(groups, *a, **k):
            ib = a[0] if name == "follower_step" else a[1]
            fi, M = self.fin, ib.M
            assert fi.inbox.M == M and M > 0
            for col, dt in INBOX:
                assert np.array_equal(host(getattr(fi.inbox, col), dt, M),
                                      host(getattr(ib, col), dt, M)), col
            if name == "follower_step":
                return real(groups, fi.inbox, *a[1:], **k)
            flog, _, app = a[:3]
            E_ = int(app.E)
            assert int(fi.ent_total[0]) == E_ <= fi.app.E
            assert np.array_equal(host(fi.app.commit, np.uint64, M), host(app.commit, np.uint64, M))
            assert np.array_equal(host(fi.app.ent_off, np.uint32, M + 1),
                                  host(app.ent_off, np.uint32, M + 1))
            assert np.array_equal(host(fi.app.ent_term, np.uint64, E_), host(app.ent_term, np.uint64, E_))
            assert np.array_equal(host(fi.app.ent_len, np.uint32, E_), host(app.ent_len, np.uint32, E_))
            return real(groups, flog, fi.inbox, fi.app, *a[3:], **k)
        setattr(qf, name, stepped)
        try:
            yield
        finally:
            setattr(qf, name, real)

    def follower_step(self, j, recs, stops=False):
        with self.ingested("follower_step"):
            return super().follower_step(j, recs, stops)

    def follower_log_step(self, j, msgs):
        with self.ingested("follower_log_step"):
            return super().follower_log_step(j, msgs)

    def propose(self):
        real = qp.leader_propose

        def spy(*a, **k):
            self.propose_res = real(*a, **k)
            return self.propose_res
        qp.leader_propose = spy
        try:
            return super().propose()
        finally:
            qp.leader_propose = real


def all_ok(fi, kind, mtype):
    torch.cuda.synchronize()
    assert int(fi.status.max()) == wire.WIRE_OK
    assert bool((fi.msg_type == mtype).all()) and bool(((fi.inbox.flags[:fi.inbox.M] & 7) == kind).all())


def respond(c, groups, resps, mtype):
    """The followers' responses through encode_columns and wire.ingest into
    the leader step (the encode loop's steps 4-6)."""
    resps.sort(key=lambda x: x[0])
    M = len(resps)
    cols = {"type": np.full(M, mtype, np.uint8), "to": np.ones(M, np.uint64),
            "from": np.array([m.slot + 1 for _, m in resps], np.uint64),
            "term": np.array([m.term for _, m in resps], np.uint64)}
    cols["context" if mtype == 9 else "index"] = np.array([m.index for _, m in resps], np.uint64)
    want = E.finish(E.columns(cols, M))
    assert (want["status"] == E.OK).all()
    got = encode.encode_columns({k: ql._to_dev(v, v.dtype.type, DEV) for k, v in cols.items()}, M=M)
    same_layout(got, want, M)
    b, moff, _, _, nb = got
    c.inbox, wst, mt = wire.ingest(b, int(nb[0]), moff, dev_u32([g for g, _ in resps]), groups.off,
                                   groups.ids)
    torch.cuda.synchronize()
    assert int(wst.max()) == wire.WIRE_OK and bool((mt == mtype).all())
    return c.leader_step(resps)


def test_the_loop_closes_with_no_host_decode():
    rng = np.random.default_rng(23)
    logs = RL.make_logs(rng)
    lag = [g % 2 for g in range(G)]
    c = Cluster(logs, lag)
    lead = c.runs[0]
    ctx = [(1 << 56) + 2000 + g for g in range(G)]
    frm = [2 if g % 3 == 0 else NO for g in range(G)]
    reads = [[] if g % 7 == 6 else [(ctx[g], frm[g])] for g in range(G)]
    c.requests(reads, None)
    S, off = lead.lg.S, lead.off
    ids = np.tile(np.arange(1, 4, dtype=np.uint64), G)
    self_id = np.ones(G, np.uint64)
    groups = encode.EncodeGroups(lead.lg.t["off"], ql._to_dev(ids, np.uint64, DEV),
                                 ql._to_dev(self_id, np.uint64, DEV), lead.lg.t["term"], S)
    every = torch.arange(G, device=DEV)
    grp = dev_u32(np.arange(G))

    # ---- 1. the tick's heartbeats, decoded on the device --------------------
    beat = c.tick()
    tr = c.tick_res
    term = host(lead.lg.t["term"], np.uint64, G)
    want = E.finish(E.slots(G, off, ids, self_id, term, S, host(tr.tflags, np.uint8, G),
                            qt.TFLAG_BEAT, E.MSG_HEARTBEAT,
                            {"commit": host(tr.hb_commit, np.uint64, S),
                             "ctx_g": host(tr.hb_ctx, np.uint64, G)}))
    got = encode.encode_slots(groups, gflags=tr.tflags, gmask=qt.TFLAG_BEAT,
                              cols={"commit": tr.hb_commit, "ctx_g": tr.hb_ctx})
    by, mo = same_layout(got, want, S)
    acks = []
    for j in (1, 2):
        bj, nbj, offj = route(got[0], got[1], 3 * every + j)
        c.fin = wire.ingest_follower(bj, nbj, offj, grp, G)
        all_ok(c.fin, FW.FIN_HEARTBEAT, 8)
        recs = []
        for g in range(G):      # the same bytes decoded on the CPU: what the inbox must equal
            ok, f = W.decode_message(by[mo[3 * g + j]:mo[3 * g + j + 1]])
            assert ok and (f[1], f[2], f[3], f[4]) == (E.MSG_HEARTBEAT, j + 1, 1, TERM)
            recs.append((g, F.Rec(F.HEARTBEAT, f[3], f[4], f[8], int.from_bytes(f.get(12, b""), "big"))))
            assert recs[-1][1].aux == beat[g]
        rt, _ = c.follower_step(j, recs)
        assert all(x == F.MSG_HEARTBEAT_RESP for x in rt)
        acks += [(g, L.Inbound(L.IN_HEARTBEAT_RESP, j, TERM, m.aux)) for g, m in recs]
    respond(c, groups, acks, 9)

    # ---- 2. a proposal's bcastAppend, the host's entries spliced in ----------
    pf = c.propose()
    assert (pf & PR.PFLAG_BCAST).all()
    pr = c.propose_res
    mt, idx, lt, n = (host(pr.msg_type, np.uint8, S), host(pr.msg_index, np.uint64, S),
                      host(pr.msg_log_term, np.uint64, S), host(pr.msg_n, np.uint64, S))
    committed = host(lead.lg.t["committed"], np.uint64, G)
    term = host(lead.lg.t["term"], np.uint64, G)
    want = E.finish(E.slots(G, off, ids, self_id, term, S, pf, PR.PFLAG_BCAST, 0,
                            {"type": mt, "index": idx, "log_term": lt, "n_entries": n,
                             "commit_g": committed}))
    got = encode.encode_slots(groups, gflags=pr.pflags, gmask=PR.PFLAG_BCAST, type_all=0,
                              cols={"type": pr.msg_type, "index": pr.msg_index,
                                    "log_term": pr.msg_log_term, "n_entries": pr.msg_n,
                                    "commit_g": lead.lg.t["committed"]})
    by, mo = same_layout(got, want, S)
    at = host(got[3], np.uint32, S)
    resps = []
    for j in (1, 2):
        sent, apps, mids = [], [], []
        for g in range(G):
            s = 3 * g + j
            if want["status"][s] == E.NONE:
                continue
            assert want["status"][s] == E.ENTRIES and mt[s] == E.MSG_APP and n[s] > 0
            ents = [W.marshal_entry(c.nodes[0][g].prop.log_term(int(idx[s]) + 1 + q),
                                    int(idx[s]) + 1 + q, 0, b"payload%d" % (g + q))
                    for q in range(int(n[s]))]
            whole = E.splice(by[mo[s]:mo[s + 1]], int(at[s]), ents)
            mids.append(whole[int(at[s]):len(whole) - (int(mo[s + 1] - mo[s]) - int(at[s]))])
            sent.append(whole)
            apps.append((g, int(idx[s]), int(lt[s]), int(committed[g]), int(n[s])))
        assert len(sent) >= G // 2
        b, nb, moff, dgrp = wire.pack_messages(sent, [a[0] for a in apps], DEV)
        c.fin = wire.ingest_follower(b, nb, moff, dgrp, G)
        all_ok(c.fin, FW.FIN_APP, 3)
        # where the host takes the entries it persists from: exactly what it spliced in
        pos, nby = host(c.fin.ent_pos, np.uint64, len(sent)), host(c.fin.ent_bytes, np.uint32, len(sent))
        raw = b.cpu().numpy().tobytes()
        assert all(raw[int(p):int(p) + int(k)] == m for p, k, m in zip(pos, nby, mids))
        assert np.array_equal(host(c.fin.ent_n, np.uint32, len(sent)), [a[4] for a in apps])
        resps += c.follower_log_step(j, apps)
    respond(c, groups, resps, 4)

    # ---- 3. a campaign's vote requests through the general columns ----------
    cf, rt, req_term = c.campaign(2, np.full(G, CR.CAMP_HUP, np.uint8))
    assert (rt == CR.MSG_PREVOTE).all() and (cf & CR.CFLAG_REQUESTS).all()
    last = np.array([n_.prop.last for n_ in c.nodes[2]], np.uint64)
    last_term = np.array([n_.camp.last_term for n_ in c.nodes[2]], np.uint64)
    M = 2 * G
    cols = {"type": np.full(M, 17, np.uint8), "to": np.tile(np.array([1, 2], np.uint64), G),
            "from": np.full(M, 3, np.uint64), "term": np.repeat(req_term, 2),
            "index": np.repeat(last, 2), "log_term": np.repeat(last_term, 2)}
    want = E.finish(E.columns(cols, M))
    got = encode.encode_columns({k: ql._to_dev(v, v.dtype.type, DEV) for k, v in cols.items()}, M=M)
    same_layout(got, want, M)
    for j in (0, 1):
        bj, nbj, offj = route(got[0], got[1], 2 * every + j)
        c.fin = wire.ingest_follower(bj, nbj, offj, grp, G)
        all_ok(c.fin, FW.FIN_PREVOTE, 17)
        recs = [(g, F.Rec(F.PREVOTE, 3, int(req_term[g]), int(last[g]), int(last_term[g])))
                for g in range(G)]
        c.follower_step(j, recs)
