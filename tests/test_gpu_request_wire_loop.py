"""The loop qb_dev_ingest_requests closes, on the device, for 257 three-node
groups on two "nodes" whose tables the test owns (node j holds slot j and raft
ID j + 1; node 0 leads, node 1 follows):

  at the follower   qb_dev_leader_requests and qb_dev_leader_propose answer
                    QB_RD_FORWARD / QB_QFLAG_FORWARD / QB_PFLAG_FORWARD;
  on the wire       the forwarded MsgReadIndex and MsgTransferLeader are
                    marshalled by qb_dev_encode_messages, the MsgProps (their
                    entries are the host's) by raftpb_ref.marshal_message;
  at the leader     qb_dev_ingest_requests over its config feeds
                    qb_dev_leader_requests, then qb_dev_leader_propose, with
                    no host pass between the three calls;
  back              the leader's QB_RD_RESP goes out as MsgReadIndexResp
                    (qb_dev_encode_messages) and the ingest at the follower
                    returns its index and context.

The leader's final state and every output equal those of a second, identical
leader that gets the same requests as hand-built columns (which
tests/test_gpu_requests.DeviceRun compares with tests/request_ref.py and
tests/propose_ref.py call by call).  Group 7 is joint: its conf change is
refused and its leave, a round later, accepted."""
import numpy as np
import pytest
import torch

from etcd_amd.quorum import encode, leader as ql, propose as qp, request as qr, wire
from oracle import raftpb_ref as W
from tests import propose_pack as PP, propose_ref as PR, request_pack as Q, request_ref as R
from tests import request_wire_pack as P, request_wire_ref as RW
from tests.test_gpu_requests import DEV, DeviceRun
from tests.test_gpu_requests_loop import make_logs

pytestmark = pytest.mark.gpu
G, TERM, JOINT = 257, 2, 7
CFG = R.Config(R.LEASE, 4, 2)   # lease reads: a forwarded read is answered at once (QB_RD_RESP)
NO = R.NO_SLOT
LEADER_ID, FOLLOWER_ID, THIRD_ID = 1, 2, 3


def nodes_of(logs, j):
    """Node j's RequestNodes: the leader (0) or a follower of node 0."""
    out = []
    for g in range(G):
        n = Q.make_node(3, 0b111, 0b011 if g == JOINT else 0, j, terms=logs[g], term=TERM,
                        self_id=j + 1, role=R.LEADER if j == 0 else R.FOLLOWER, lead=LEADER_ID,
                        committed=len(logs[g]) - 1, ee=g % 3)
        n.camp.vote = LEADER_ID
        out.append(n)
    return out


class Node:
    """One node's tables on the device beside their reference copy."""

    def __init__(self, logs, j):
        self.run = DeviceRun(nodes_of(logs, j), CFG)
        z = np.zeros(G, np.uint64)
        self.ps = qp.ProposeState.from_numpy(z, z, z, device=DEV)

    def requests(self, reads, xf_from, xf_term, where):
        return self.run.call(Q.inputs(G, CFG.max_reads, reads, xf_from, xf_term), where)

    def propose(self, inp, where):
        """Hand-built columns through qb_dev_leader_propose, against propose_ref."""
        run = self.run
        ib = qp.ProposeInbox.from_numpy(inp["action"], inp["n_ents"], inp["payload"], inp["cc_at"],
                                        inp["cc_payload"], device=DEV)
        res = qp.leader_propose(run.lg, run.es, self.ps, ib)
        pf, _, _ = PP.ref_propose([n.prop for n in run.nodes], inp, PR.Config(), run.off,
                                  PP.new_msg(run.lg.S))
        assert np.array_equal(res.pflags.cpu().numpy()[:G], pf), where
        for n in run.nodes:
            n.sync()
        run.check_state(where)
        return res, pf

    def tables(self):
        t = dict(self.run.lg.numpy())
        t.update({f"es.{k}": v for k, v in self.run.es.numpy().items()})
        t.update({f"ps.{k}": v for k, v in self.ps.numpy(G).items()})
        return t


def dev_u32(a):
    return ql._to_dev(np.asarray(a, np.uint32), np.uint32, DEV)


def on_the_wire(reads, xfers, props):
    """(bytes, nbytes, msg_off, msg_group) on the device: reads [(g, ctx)] and
    transfers [(g, transferee ID)] as the follower's raft.send leaves them,
    through qb_dev_encode_messages, then the MsgProps [(g, entries)] through
    marshal_message, in that order (within a group: arrival order)."""
    n_r, n_x = len(reads), len(xfers)
    M1 = n_r + n_x
    cols = {"type": np.array([15] * n_r + [13] * n_x, np.uint8),
            "to": np.full(M1, LEADER_ID, np.uint64),
            # a forwarded read gets the follower's ID, a transfer keeps the transferee's (raft.go:406-408)
            "from": np.array([FOLLOWER_ID] * n_r + [t for _, t in xfers], np.uint64),
            # raft.send: no term on MsgReadIndex, the sender's on MsgTransferLeader (raft.go:402-416)
            "term": np.array([0] * n_r + [TERM] * n_x, np.uint64),
            "context": np.array([c for _, c in reads] + [0] * n_x, np.uint64)}
    b, moff, st, _, nb = encode.encode_columns({k: ql._to_dev(v, v.dtype.type, DEV) for k, v in cols.items()},
                                               M=M1)
    torch.cuda.synchronize()
    assert M1 == 0 or int(st.max()) == encode.ENC_OK
    n1 = int(nb[0])
    pm = [W.marshal_message(type=2, to=LEADER_ID, frm=FOLLOWER_ID, entries=e) for _, e in props]
    pbuf, poff = P.pack(pm)
    buf = torch.cat([b[:n1], P.dev(np.frombuffer(pbuf, np.uint8))[:len(pbuf)]])
    off = torch.cat([moff[:M1], P.dev(poff) + n1])
    grp = dev_u32([g for g, _ in reads] + [g for g, _ in xfers] + [g for g, _ in props])
    return buf, n1 + len(pbuf), off, grp[:M1 + len(pm)]


def by_the_wire(a: Node, batch, where):
    """The batch through qb_dev_ingest_requests and, untouched, through the two
    step calls at leader ``a``; returns (the ingest, the requests' result, the
    proposal's)."""
    buf, nbytes, moff, grp = batch
    run = a.run
    ids = ql._to_dev(np.tile(np.array([1, 2, 3], np.uint64), G), np.uint64, DEV)
    rq = wire.ingest_requests(buf, nbytes, moff, grp, run.lg.t["off"], ids, max_reads=CFG.max_reads,
                              concat=True)
    rres = qr.leader_requests(run.lg, run.es, rq.request_in, out=run.out)   # first
    pres = qp.leader_propose(run.lg, run.es, a.ps, rq.propose_in)           # second
    torch.cuda.synchronize()
    assert (rq.status == wire.WIRE_OK).all(), (where, rq.status.cpu().numpy())
    return rq, rres, pres


def same(a: Node, b: Node, ra, rb, pa, pb, where):
    """Leader a (fed by the ingest) against leader b (fed hand-built columns):
    every table and every output of both calls."""
    ta, tb = a.tables(), b.tables()
    assert ta.keys() == tb.keys()
    for k in ta:
        assert np.array_equal(ta[k], tb[k]), (where, k, np.flatnonzero(ta[k] != tb[k])[:8])
    for k in Q.OUT_KEYS:
        assert torch.equal(getattr(ra, k), getattr(rb, k)), (where, k)
    assert ra.stats_dict() == rb.stats_dict(), where
    for k in ("pflags", "msg_type", "msg_index", "msg_log_term", "msg_n", "stats"):
        assert torch.equal(getattr(pa, k), getattr(pb, k)), (where, k)


def test_forwarded_requests_round_trip():
    rng = np.random.default_rng(31)
    logs = make_logs(rng)
    a, b, f = Node(logs, 0), Node(logs, 0), Node(logs, 1)
    ctx = lambda g, k: 1000 + 2 * g + k  # noqa: E731
    n_reads = [g % 3 for g in range(G)]
    xf = [g % 5 == 0 for g in range(G)]
    v2 = P.marshal_cc_v2(0, [(0, 9)])
    ents = {g: [P.ent(bytes(1 + g % 7)) for _ in range(1 + g % 2)] for g in range(0, G, 2)}
    ents[JOINT] = [P.ent(b"ab"), P.ent(v2, RW.ENTRY_CONF_CHANGE_V2), P.ent(b"")]

    # ---- the follower forwards all of it --------------------------------
    res = f.requests([[(ctx(g, k), NO) for k in range(n_reads[g])] for g in range(G)],
                     [2 if xf[g] else NO for g in range(G)], None, "follower requests")
    for g, r in enumerate(res):
        assert r.reads == [(R.RD_FORWARD, None)] * n_reads[g], g
        assert bool(r.qflags & R.QFLAG_FORWARD) == (n_reads[g] > 0 or xf[g]), g
    fin = PP.inputs([PR.PROP_ENTRIES if g in ents else PR.PROP_NONE for g in range(G)],
                    [len(ents.get(g, ())) for g in range(G)])
    _, pf = f.propose(fin, "follower propose")
    assert all(pf[g] == (PR.PFLAG_FORWARD if g in ents else 0) for g in range(G))

    # ---- round 1 at the leader: the ingest's columns against hand-built ones ----
    reads = [(g, ctx(g, k)) for k in range(2) for g in range(G) if k < n_reads[g]]
    xfers = [(g, THIRD_ID) for g in range(G) if xf[g]]
    props = sorted(ents.items())
    rq, ra, pa = by_the_wire(a, on_the_wire(reads, xfers, props), "round 1")
    rb = b.requests([[(ctx(g, k), 1) for k in range(n_reads[g])] for g in range(G)],
                    [2 if xf[g] else NO for g in range(G)], [TERM if xf[g] else 0 for g in range(G)],
                    "hand-built requests")
    payload = {g: sum(len(W.unmarshal("Entry", e).get(4, b"")) for e in es) for g, es in ents.items()}
    hand = PP.inputs([(PR.PROP_ENTRIES | (PR.PROP_CONF_CHANGE if g == JOINT else 0)) if g in ents
                      else PR.PROP_NONE for g in range(G)],
                     [len(ents.get(g, ())) for g in range(G)], [payload.get(g, 0) for g in range(G)],
                     [1 if g == JOINT else 0 for g in range(G)],
                     [len(v2) if g == JOINT else 0 for g in range(G)])
    pb, pf = b.propose(hand, "hand-built propose")
    same(a, b, ra, b.run.out, pa, pb, "round 1")
    # the ingest wrote what the hand wrote
    for k in ("action", "n_ents", "payload", "cc_at", "cc_payload"):
        got = getattr(rq.propose_in, k).cpu().numpy()[:G]
        assert np.array_equal(got.view(hand[k].dtype), hand[k]), k
    assert (rq.gflags.cpu().numpy()[:G] == [1 if n_reads[g] or xf[g] or g in ents else 0
                                            for g in range(G)]).all()
    # a transfer started ahead of the proposal drops it; the joint group refuses its conf change
    assert pf[JOINT] & PR.PFLAG_CC_REFUSED and pf[JOINT] & PR.PFLAG_APPENDED and not xf[JOINT]
    assert all(pf[g] == PR.PFLAG_DROPPED for g in ents if xf[g])

    # ---- the answers go back: MsgReadIndexResp, ingested at the follower ----
    st = ra.rd_status.cpu().numpy()
    idx = ql._to_np(ra.rd_index, np.uint64, CFG.max_reads * G)
    rd_k = rq.rd_k.cpu().numpy()
    at = [int(rd_k[i]) * G + g for i, (g, _) in enumerate(reads)]
    assert all(st[p] == R.RD_RESP for p in at) and len(at) > G // 2
    M = len(reads)
    cols = {"type": np.full(M, 16, np.uint8), "to": np.full(M, FOLLOWER_ID, np.uint64),
            "from": np.full(M, LEADER_ID, np.uint64), "term": np.full(M, TERM, np.uint64),
            "index": idx[at], "context": np.array([c for _, c in reads], np.uint64)}
    eb, eoff, est, _, enb = encode.encode_columns({k: ql._to_dev(v, v.dtype.type, DEV) for k, v in cols.items()},
                                                  M=M)
    back = wire.ingest_requests(eb, int(enb[0]), eoff, dev_u32([g for g, _ in reads]), f.run.lg.t["off"],
                                ql._to_dev(np.tile(np.array([1, 2, 3], np.uint64), G), np.uint64, DEV))
    torch.cuda.synchronize()
    assert int(est.max()) == encode.ENC_OK
    assert (back.kind == wire.RQ_READ_RESP).all() and (back.status == wire.WIRE_OK).all()
    assert np.array_equal(ql._to_np(back.index, np.uint64, M), idx[at])
    assert np.array_equal(ql._to_np(back.ctx, np.uint64, M), cols["context"])
    assert (back.term == TERM).all() and (back.frm == LEADER_ID).all()
    assert not back.gflags.any() and not back.request_in.n_reads.any()   # it takes no part in pass 2
    want_idx = [len(logs[g]) - 1 for g, _ in reads]                      # committed when the read came
    assert idx[at].tolist() == want_idx

    # ---- round 2: the joint group leaves, a few reads beside it --------
    leave = P.marshal_cc_v2()
    reads2 = [(g, 5000 + g) for g in range(1, G, 4)]
    rq2, ra2, pa2 = by_the_wire(a, on_the_wire(reads2, [], [(JOINT, [P.ent(leave, RW.ENTRY_CONF_CHANGE_V2)])]),
                                "round 2")
    r2 = {g: c for g, c in reads2}
    rb2 = b.requests([[(r2[g], 1)] if g in r2 else [] for g in range(G)], None, None, "hand-built requests 2")
    is_j = [g == JOINT for g in range(G)]
    hand2 = PP.inputs([(PR.PROP_ENTRIES | PR.PROP_CONF_CHANGE | PR.PROP_CC_LEAVE_JOINT) if j else PR.PROP_NONE
                       for j in is_j], [int(j) for j in is_j], [len(leave) * j for j in is_j],
                      [0] * G, [len(leave) * j for j in is_j])
    pb2, pf2 = b.propose(hand2, "hand-built propose 2")
    same(a, b, ra2, b.run.out, pa2, pb2, "round 2")
    assert int(rq2.propose_in.action[JOINT]) == hand2["action"][JOINT] and rb2 is not None
    assert pf2[JOINT] & PR.PFLAG_APPENDED and not pf2[JOINT] & PR.PFLAG_CC_REFUSED
    assert b.run.nodes[JOINT].prop.pending_conf_index == b.run.nodes[JOINT].prop.last
