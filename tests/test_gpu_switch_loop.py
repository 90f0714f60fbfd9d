"""The membership-change path on the device at 257 groups with no per-group
host code between the calls.  ``test_the_whole_chain`` runs qb_dev_leader_propose
(a conf-change entry) -> qb_dev_leader_step (the acks) -> qb_dev_conf_change ->
qb_dev_switch_config, then qb_dev_leader_propose and qb_dev_leader_tick on the
renumbered meta, over one set of device buffers, every stage against its own
Python reference (tests/propose_ref.py, oracle/leader_ref.py, the Changer's
expected output, tests/switch_ref.py, tests/tick_ref.py).
``test_conf_change_then_switch_config`` is the two middle calls alone, the
wrapper taking the ConfigTable ``change`` returned as it is (its
over-allocated tensors included).  In both, odd groups replay TestCommitAfterRemoveNode
(the removal lowers the quorum and the pending entry commits), even groups
confchange_v1_add_single (the new member is probed at once with the conf-change
entry).  The new member's ID ranks before the leader's in every fourth group,
so the own slot moves.  Each stage is compared with its Python reference: the
Changer's output with the expected config and initProgress, the switch with
tests/switch_ref.py on every array, output and counter."""
import numpy as np
import pytest

from tests import switch_pack as P, switch_ref as R

pytestmark = pytest.mark.gpu
G = 257
REPL = dict(state=R.REPLICATE, recent_active=True)


def _groups():
    old, want = [], []
    for g in range(G):
        b = 3 * g + 10
        if g % 2:       # leader b+1 of (b+1, b+2) removes b+2: 3 commits
            pr = {b + 1: dict(match=3, next=4, **REPL), b + 2: dict(match=2, next=4, **REPL)}
            kw = dict(self_id=b + 1, term=1, terms=[0, 1, 1, 1], committed=2)
            old.append(P.group([], [b + 1, b + 2], [b + 1, b + 2], progress=pr, **kw))
            want.append(P.group([b + 1, b + 2], [b + 1], [b + 1], progress=pr, **kw))
        else:           # leader b+1 alone adds a voter: Next = LastIndex = 4, Probe
            new = b if g % 4 == 0 else b + 2
            pr = {b + 1: dict(match=4, next=5, **REPL)}
            kw = dict(self_id=b + 1, term=1, terms=[1, 1, 1], first=3, committed=4)
            old.append(P.group([], [b + 1], [b + 1], progress=pr, **kw))
            want.append(P.group([b + 1], [b + 1, new], [b + 1, new],
                                progress={**pr, new: dict(match=0, next=4)}, **kw))
    return old, want


def test_conf_change_then_switch_config():
    import torch
    from etcd_amd.quorum import confchange as qcc, leader as ql
    from tests import switch_dev as D
    old_g, want_g = _groups()
    o, a = P.pack(old_g), P.pack(want_g)
    old = qcc.ConfigTable.from_numpy(o["off"], o["ids"], o["cfg"], np.zeros(G, np.uint32),
                                     {k: o[k] for k in P.SLOT_KEYS}, P.INFLIGHT_CAP, device=D.DEV)
    ops = [qcc.SIMPLE] * G
    ccs = [[(qcc.REMOVE_NODE, 3 * g + 12)] if g % 2 else
           [(qcc.ADD_NODE, 3 * g + 10 if g % 4 == 0 else 3 * g + 12)] for g in range(G)]
    new, err, _ = old.change(ops, ccs, o["last_index"])
    assert not err.any()
    # stage 1: the Changer's output is the expected config and Progress
    got = new.numpy()
    assert new.S == int(a["off"][-1])
    for k in ("off", "cfg", "ids", "match", "next", "pending_snapshot", "pstate", "infl_pos"):
        assert np.array_equal(got[k][:len(a[k])], a[k]), k
    a["infl_buf"] = got["infl_buf"].copy()      # (rings of fresh slots hold what the Changer left)
    # stage 2: the switch over the Changer's own tensors
    run = D.DeviceRun(a)
    run.old, run.new = old, new
    sf = run.switch(np.full(G, R.SW_SWITCH, np.uint8), "loop")
    odd = np.arange(G) % 2 == 1
    assert (sf[odd] == R.SWFLAG_SWITCHED | R.SWFLAG_COMMITTED | R.SWFLAG_SENT).all()
    assert (sf[~odd] == R.SWFLAG_SWITCHED | R.SWFLAG_SENT).all()
    assert (ql._to_np(run.lg.t["committed"], np.uint64, G)[odd] == 3).all()
    assert run.out.messages(1) == []
    # confchange_v1_add_single: 1->2 MsgApp Log:1/3 Commit:4 Entries:[1/4]
    assert run.out.messages(2) == [(R.MSG_APP, 1, 3, 1, 4, 1)]
    assert run.out.messages(0) == [(R.MSG_APP, 0, 3, 1, 4, 1)]      # the new member ranks first
    assert int(run.lg.t["meta"][0].item()) & 0xFF == 1                 # and the own slot moved
    assert run.lg.t["off"].data_ptr() == new.t["off"].data_ptr()       # the table runs on the new config
    torch.cuda.synchronize()


# ------------------------------------------------------------ the whole chain ---

def test_the_whole_chain():
    import torch
    from etcd_amd.quorum import confchange as qcc, leader as ql, propose as qp, switch as qs
    from oracle import leader_ref as L
    from tests import propose_pack as PP, propose_ref as PR, tick_ref as T
    from tests.test_gpu_propose import DEV, FILL_I64, DeviceRun
    cap = PP.INFLIGHT_CAP
    repl = lambda m: PP.progress(m, m + 1, L.STATE_REPLICATE, recent_active=True)  # noqa: E731
    nodes, old_ids, new_ids = [], [], []
    for g in range(G):
        b = 3 * g + 10
        if g % 2:       # TestCommitAfterRemoveNode: (b+1, b+2), 1 the leader's empty entry
            nodes.append(PP.make_node(2, 0b11, 0, 0, terms=[0, 1], term=1, committed=1,
                                      prs=[repl(1), repl(1)], self_id=b + 1))
            old_ids.append([b + 1, b + 2])
            new_ids.append([b + 1])
        else:           # confchange_v1_add_single: b+1 alone behind a snapshot at 2
            nodes.append(PP.make_node(1, 0b1, 0, 0, terms=[1, 1], first=3, term=1, committed=3,
                                      prs=[repl(3)], self_id=b + 1))
            old_ids.append([b + 1])
            new_ids.append(sorted([b + 1, b if g % 4 == 0 else b + 2]))
    odd = np.arange(G) % 2 == 1
    run = DeviceRun(nodes)

    # 1. the conf-change entry, then "hello" behind it where there is a peer
    cc = PR.PROP_ENTRIES | PR.PROP_CONF_CHANGE
    pf = run.propose(PP.inputs([cc] * G, [1] * G, [8] * G, [0] * G, [8] * G), "propose cc")
    assert (pf & PR.PFLAG_APPENDED).all() and not (pf & PR.PFLAG_CC_REFUSED).any()
    pf = run.propose(PP.inputs(np.where(odd, PR.PROP_ENTRIES, PR.PROP_NONE), [1] * G, [5] * G),
                     "propose hello")
    assert (pf[odd] & PR.PFLAG_APPENDED).all()

    # 2. the peer acknowledges the conf change: it commits, "hello" does not
    resps = [(g, L.Inbound(L.IN_APP_RESP, 1, 1, 2, False, 0, 0)) for g in range(G) if g % 2]
    for n in run.nodes:
        n.sync()
        n.group.msgs = []
    for i, (g, m) in enumerate(resps):
        assert run.nodes[g].group.step(m, i) == "applied"
    ib = ql.LeaderInbox.from_numpy(
        [g for g, _ in resps], [m.slot for _, m in resps], [m.kind for _, m in resps],
        np.array([m.index for _, m in resps], np.uint64),
        np.array([m.term for _, m in resps], np.uint64), [m.reject for _, m in resps],
        np.zeros(len(resps), np.uint64), np.zeros(len(resps), np.uint64), device=DEV)
    res = run.lg.step(ib)
    got = [[] for _ in range(G)]
    for m in res.msgs:
        got[int(m["group"])].append((int(m["type"]), int(m["to"]), int(m["index"]),
                                     int(m["log_term"]), int(m["commit"]), int(m["aux"])))
    assert got == [[m.key() for m in n.group.msgs] for n in run.nodes]
    run.check_state("leader step")
    a, e, p = PP.pack_nodes(run.nodes, cap)
    assert (a["committed"][odd] == 2).all() and (a["committed"][~odd] == 4).all()
    assert (a["last_index"][odd] == 3).all()

    # 3. the Changer over the table's own tensors; expected: kept slots carried,
    # the new one initProgress (Match 0, Next = LastIndex, Probe, RecentActive)
    t = run.lg.t
    S0 = run.lg.S
    flat = lambda rows: np.array([x for r in rows for x in r], np.uint64)  # noqa: E731
    old = qcc.ConfigTable(G, S0, cap, dict(
        {k: t[k] for k in ("off", "cfg", "match", "next", "pending_snapshot", "pstate", "infl_pos",
                           "infl_buf")},
        ext=torch.zeros(G, dtype=torch.int32, device=DEV), ids=ql._to_dev(flat(old_ids), np.uint64, DEV)))
    ccs = [[(qcc.REMOVE_NODE, old_ids[g][1])] if g % 2 else
           [(qcc.ADD_NODE, next(i for i in new_ids[g] if i not in old_ids[g]))] for g in range(G)]
    new, err, _ = old.change([qcc.SIMPLE] * G, ccs, a["last_index"])
    assert not err.any()
    sa = {k: a[k].copy() for k in ("meta", "term", "committed", "first_index", "last_index",
                                   "snap_index", "snap_term", "max_ents", "run_start", "run_term")}
    sa.update(old_off=a["off"].copy(), old_ids=flat(old_ids), ids=flat(new_ids),
              role=e["role"].copy(), self_id=e["self_id"].copy(), last_term=e["last_term"].copy(),
              votes=e["votes"].copy(), rq_meta=np.zeros(1, np.uint32))
    sa["off"] = np.concatenate([[0], np.cumsum([len(r) for r in new_ids])]).astype(np.uint32)
    sa["cfg"] = np.array([(1 << len(r)) - 1 for r in new_ids], np.uint32)
    S = int(sa["off"][-1])
    fresh = {"match": 0, "pending_snapshot": 0, "pstate": R.PROBE | R.RECENT_ACTIVE, "infl_pos": 0}
    for k in P.SLOT_KEYS:
        sa[k] = np.zeros(S, a[k].dtype)
    for g in range(G):
        for j, i in enumerate(new_ids[g]):
            d = int(sa["off"][g]) + j
            for k in P.SLOT_KEYS:
                if i in old_ids[g]:
                    sa[k][d] = a[k][int(a["off"][g]) + old_ids[g].index(i)]
                else:
                    sa[k][d] = a["last_index"][g] if k == "next" else fresh[k]
    gotn = new.numpy()
    assert new.S == S
    for k in ("off", "cfg", "ids") + P.SLOT_KEYS:
        assert np.array_equal(gotn[k][:len(sa[k])], sa[k]), k
    sa["infl_buf"] = gotn["infl_buf"].copy()    # (rings of fresh slots hold what the Changer left)

    # 4. switchToConfig: the removal commits "hello", the new member is probed
    action = np.full(G, R.SW_SWITCH, np.uint8)
    out = qs.SwitchResult(
        torch.full((G,), 0xA5, dtype=torch.uint8, device=DEV),
        torch.full((S0,), 0xA5, dtype=torch.uint8, device=DEV),
        torch.full((S,), 0xA5, dtype=torch.uint8, device=DEV),
        *[torch.full((S,), FILL_I64, dtype=torch.int64, device=DEV) for _ in range(3)],
        torch.zeros(len(qs.SWSTAT_NAMES), dtype=torch.int64, device=DEV))
    qs.switch_config(run.lg, run.es, old, new, ql._to_dev(action, np.uint8, DEV), out=out)
    want, st = R.new_out(G, S0, S), R.new_stats()
    sent = R.switch_config(sa, action, cap, 0, want, st)
    dev_a, dev_e = run.lg.numpy(), run.es.numpy()
    for k in ("meta", "committed", "off", "cfg", "infl_buf") + P.SLOT_KEYS:
        assert np.array_equal(dev_a[k], sa[k][:len(dev_a[k])]), ("switch", k)
    assert np.array_equal(dev_e["votes"], sa["votes"])
    for k, n_ in (("swflags", G), ("slot_map", S0), ("msg_type", S), ("msg_index", S),
                  ("msg_log_term", S), ("msg_n", S)):
        assert np.array_equal(ql._to_np(getattr(out, k), want[k].dtype, n_), want[k][:n_]), k
    assert out.stats_dict() == st
    sf = want["swflags"][:G]
    assert (sf[odd] == R.SWFLAG_SWITCHED | R.SWFLAG_COMMITTED | R.SWFLAG_SENT).all()
    assert (sa["committed"][odd] == 3).all()                    # TestCommitAfterRemoveNode
    assert (sf[~odd] == R.SWFLAG_SWITCHED | R.SWFLAG_SENT).all()
    for g in (0, 2):            # confchange_v1_add_single: MsgApp Log:1/3 Commit:4 Entries:[1/4]
        to = new_ids[g].index(next(i for i in new_ids[g] if i not in old_ids[g]))
        assert out.messages(g) == sent[g] == [(R.MSG_APP, to, 3, 1, 4, 1)]
    assert int(sa["meta"][0]) & 0xFF == 1 and int(sa["meta"][2]) & 0xFF == 0

    # 5. a proposal on the renumbered meta: the reference nodes are rebuilt from
    # the reference's arrays, the device goes on with the buffers it has
    e2 = dict(e, votes=sa["votes"])
    run.nodes = PP.nodes_from_arrays(dict(sa), e2, p, cap)
    run.off = sa["off"]
    run.out = qp.ProposeResult(
        torch.full((G,), 0xA5, dtype=torch.uint8, device=DEV),
        torch.full((S,), 0xA5, dtype=torch.uint8, device=DEV),
        *[torch.full((S,), FILL_I64, dtype=torch.int64, device=DEV) for _ in range(3)],
        run.out.stats)
    run.msg = PP.new_msg(S)
    run.check_state("behind the switch")
    pf = run.propose(PP.inputs([PR.PROP_ENTRIES] * G, [1] * G, [8] * G), "propose behind the switch")
    assert (pf & PR.PFLAG_APPENDED).all()
    assert (pf[odd] & PR.PFLAG_COMMITTED).all() and not (pf[~odd] & PR.PFLAG_COMMITTED).any()
    assert not any(run.sent)      # a lone voter has no peer; the new member's probe is in flight

    # 6. a tick that beats: a heartbeat for every slot but the (moved) own one
    res = run.lg.tick(run.state, 10, 1, True)
    tf = res.tflags.cpu().numpy()[:G]
    hb = ql._to_np(res.hb_commit, np.uint64, S)
    for g, n in enumerate(run.nodes):
        c = n.camp
        tn = T.TickNode(n.group, c.role, c.election_elapsed, c.heartbeat_elapsed, 0)
        assert T.tick(tn, 10, 1, True) == tf[g], g
        c.role, c.election_elapsed, c.heartbeat_elapsed = tn.role, tn.election_elapsed, tn.heartbeat_elapsed
        assert len(tn.msgs) == len(new_ids[g]) - 1
        for m in tn.msgs:
            assert int(hb[int(sa["off"][g]) + m.to]) == m.commit, (g, m)
            assert new_ids[g][m.to] != int(sa["self_id"][g])
    run.check_state("tick")
