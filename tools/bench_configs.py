#!/usr/bin/env python3
"""Throughput of every BASELINE config on one GPU (bench.py measures only
configs[1]; these are the parity-test configs, measured the same way).

  config 1  plumbing: BenchmarkMajorityConfig_CommittedIndex (bench_test.go:24-40),
            voters 1..11, CPU ns/op beside GPU ns per group
  config 3  16M groups ragged 3-9 voters + 0-2 learners (CSR)
  config 4  joint 5+5 (overlap 0-5), 8M groups = one GPU's shard of 64M
  config 5  streaming tracker: 16M 5-voter groups, one MsgAppResp per group
            per step on average (1% stale term), apply + commit advance

Prints one JSON line per config: groups/s (group-steps/s for config 5),
per-launch device time (HIP events around R back-to-back launches / R),
algorithmic GB/s and fraction of the 8 TB/s HBM peak.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import HBM_PEAK_GBS, HipEvents  # noqa: E402
from etcd_amd.quorum import batch  # noqa: E402

dev = torch.device("cuda", 0)


GPU_ONLY = False  # the command line's --gpu-only (functions take gpu_only= explicitly too)


def time_region(fn, reps, warm_s=0.3, regions=5):
    """Per-call device time: median over `regions` event-timed regions of
    `reps` back-to-back calls, after ~warm_s seconds of warm-up calls (a
    fresh box needs that long before its clocks settle: with 3 warm-up
    calls the first config measured up to 20 % slow)."""
    import time
    sp = torch.cuda.current_stream(dev).cuda_stream
    t0 = time.perf_counter()
    while True:
        fn()
        torch.cuda.synchronize()
        if time.perf_counter() - t0 >= warm_s:
            break
    ev = HipEvents(2)
    ts = []
    for _ in range(regions):
        torch.cuda.synchronize()
        ev.record(ev.ev[0], sp)
        for _ in range(reps):
            fn()
        ev.record(ev.ev[1], sp)
        torch.cuda.synchronize()
        ts.append(ev.elapsed_ms(0, 1) / 1e3 / reps)
    ev.close()
    return float(np.median(ts))


def cpu_rate(fn, groups, seconds=2.0):
    """groups/s of a CPU oracle call repeated for ~seconds."""
    import time
    reps, t0 = 0, time.perf_counter()
    while True:
        fn()
        reps += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return reps * groups / dt


def report(name, groups, t, algo_bytes, extra=None):
    gbs = algo_bytes / t / 1e9
    d = {"config": name, "groups_per_s": groups / t, "per_launch_us": t * 1e6,
         "algo_bytes_per_launch": algo_bytes, "algo_bytes_per_group": algo_bytes / groups,
         "achieved_GBs": gbs, "frac_hbm_peak": gbs / HBM_PEAK_GBS}
    if extra:
        d.update(extra)
    print(json.dumps(d), flush=True)


def plumbing_config(reps):
    """BASELINE configs[0]: BenchmarkMajorityConfig_CommittedIndex
    (quorum/bench_test.go:24-40), voters in {1,3,5,7,9,11}.  CPU: the
    faithful C restatement (map config + map AckedIndexer + insertion sort),
    one config called in a loop on 1 thread, ns/op.  GPU beside it: the same
    CommittedIndex over 16M groups of that width in one launch (fixed layout,
    CommittedIndex only), device ns per group."""
    import time
    from tests import oracle_c as oc
    lib = oc.load()
    G = 1 << 24
    for n in (1, 3, 5, 7, 9, 11):
        iters, t = 1 << 20, 0.0
        while True:
            t0 = time.perf_counter()
            lib.orc_bench_plumbing(n, iters, 0x5EED0001)
            t = time.perf_counter() - t0
            if t >= 0.5:
                break
            iters *= 4
        fg = batch.FixedGroups.synth(0x5EED0001, n, G, device=dev)
        c = torch.empty(G, dtype=torch.int64, device=dev)
        tg = time_region(lambda: fg.committed_vote(c, want_vote=False), reps)
        print(json.dumps({"config": f"plumbing voters={n}", "cpu_ns_per_op": t / iters * 1e9,
                          "cpu_kind": "port (faithful C restatement of majority.go, 1 thread)",
                          "gpu_ns_per_group": tg / G * 1e9, "gpu_groups_per_launch": G,
                          "gpu_achieved_GBs": G * (8 * n + 8) / tg / 1e9}), flush=True)
        del fg, c


def csr_config(kind, G, reps, *, reporter=None, gpu_only=None):
    reporter = reporter or report
    gpu_only = GPU_ONLY if gpu_only is None else gpu_only
    grp = batch.CsrGroups.synth(0x5EED0003 if kind == "ragged" else 0x5EED0004, kind, G,
                                device=dev)
    slots = int(grp.off[-1].item())
    c = torch.empty(G, dtype=torch.int64, device=dev)
    v = torch.empty(G, dtype=torch.uint8, device=dev)
    t = time_region(lambda: grp.committed_vote(c, v), reps)
    # off (4) + cfg (4) + votes (4) + match (8 s) + commit (8) + vote (1)
    algo = G * (4 + 4 + 4 + 8 + 1) + 8 * slots + 4
    if gpu_only:
        reporter(f"{kind} CSR", G, t, algo, {"mean_slots": slots / G})
        return
    # CPU beside it: the oracle's SoA C restatement on a bounded sample
    from tests import oracle_c as oc
    threads = max(1, min(16, os.cpu_count() or 1))
    Gs = 1 << 20
    off, m, cfg, votes = oc.gen_csr(0x5EED0003 if kind == "ragged" else 0x5EED0004, kind, Gs)
    cpu = cpu_rate(lambda: oc.csr_eval(off, m, cfg, votes, threads=threads), Gs)
    cpu1 = cpu_rate(lambda: oc.csr_eval(off, m, cfg, votes), Gs)
    reporter(f"{kind} CSR", G, t, algo, {"mean_slots": slots / G,
           "cpu_baseline": {"value": cpu, "unit": "groups/s", "cores": threads, "kind": "port",
                            "value_1thread": cpu1,
                            "sample": f"{Gs} groups, C SoA restatement (oracle)"}})


def tracker_config(G, reps, seed=55, E=64, warm_steps=4, regions=5, *, reporter=None,
                   gpu_only=None):
    """Config 5: streaming MsgAppResp batches.  The leader holds E new
    entries per step (its own match, slot 0, is already at the last one);
    batch k acknowledges index last + (k+1)·E − lag (lag < 96) for a random
    follower of a random group, 1 % stale-term — so every step raises
    matches and advances commits, as a live stream does (the same batch
    replayed would leave the state unchanged after its first application).
    Each timed region restores the start state (untimed), runs warm_steps
    batches, then times `reps` further distinct batches; median of regions."""
    reporter = reporter or report
    gpu_only = GPU_ONLY if gpu_only is None else gpu_only
    n = 5
    rng = np.random.default_rng(seed)
    tr = batch.FixedTracker(n, G, dev)
    fg = batch.FixedGroups.synth(0x5EED0005, n, G, device=dev, with_term_start=True)
    tr.match.copy_(fg.match)
    tr.term_start.copy_(fg.term_start)
    tr.term.fill_(7)
    tr.commit_advance()
    last = fg.match[0].clone()
    del fg
    nb = warm_steps + reps
    tr.match[0].copy_(last + nb * E)  # the leader's own match (raft.go:747-748 appendEntry)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    batches = []
    for k in range(nb):
        group = torch.randint(0, G, (G,), generator=gen, device=dev, dtype=torch.int32)
        slot = torch.randint(1, n, (G,), generator=gen, device=dev, dtype=torch.int32)
        lag = torch.randint(0, 96, (G,), generator=gen, device=dev, dtype=torch.int64)
        index = last[group.long()] + (k + 1) * E - lag
        term = torch.where(torch.rand(G, generator=gen, device=dev) < 0.01, 6, 7).to(torch.int64)
        batches.append(batch.AppRespBatch(group, slot.to(torch.uint8), index, term))
    snap = {k_: getattr(tr, k_).clone() for k_ in ("match", "committed", "active", "stepdown_at")}
    sp = torch.cuda.current_stream(dev).cuda_stream

    def restore():
        for k_, v_ in snap.items():
            getattr(tr, k_).copy_(v_)

    def stream_time(step):
        ev = HipEvents(2)
        ts = []
        for r in range(regions + 1):  # region 0 warms the clocks, not reported
            restore()
            for k in range(warm_steps):
                step(batches[k])
            torch.cuda.synchronize()
            ev.record(ev.ev[0], sp)
            for k in range(warm_steps, nb):
                step(batches[k])
            ev.record(ev.ev[1], sp)
            torch.cuda.synchronize()
            if r:
                ts.append(ev.elapsed_ms(0, 1) / 1e3 / reps)
        ev.close()
        return float(np.median(ts))

    def two_call(b):
        tr.apply_appresp(b)
        tr.commit_advance()

    t_two = t_apply = t_commit = float("nan")
    if not gpu_only:  # A/B runs time the bucketed step alone
        t_two = stream_time(two_call)
        t_apply = stream_time(lambda b: tr.apply_appresp(b))
        t_commit = time_region(lambda: tr.commit_advance(), reps)
    t = stream_time(lambda b: tr.step(b))
    adv = torch.zeros(G, dtype=torch.uint8, device=dev)
    restore()
    for k in range(nb - 1):
        tr.step(batches[k])
    tr.step(batches[nb - 1], adv)
    advanced_last = int(adv.sum().item())
    applied_last = tr.stats_dict()["applied"]
    del batches
    # record 21 B + match RMW 16 B per message; commit advance
    # reads match 40 + term_start 8 + committed 8, writes committed 8 per group
    algo = G * (21 + 16) + G * 64
    # CPU beside it: the sequential one-record-at-a-time oracle (the Go
    # stepLeader loop restated) on a bounded sample, 1 thread
    if gpu_only:
        reporter("streaming tracker (bucketed step)", G, t, algo, {"unit": "group-steps/s"})
        return
    from tests import oracle_c as oc
    Gs = 1 << 20
    m0, _, _, ts0 = oc.gen_fixed(0x5EED0005, n, Gs)
    st = {"match": m0, "active": np.zeros(Gs, np.uint16), "term": np.full(Gs, 7, np.uint64),
          "term_start": ts0, "committed": np.zeros(Gs, np.uint64),
          "stepped_down": np.zeros(Gs, np.uint8)}
    oc.commit_all(n, st["match"], ts0, st["committed"])
    grp_ = rng.integers(0, Gs, size=Gs).astype(np.uint32)
    flg = rng.integers(1, n, size=Gs).astype(np.uint8)
    lag = rng.integers(0, 96, size=Gs).astype(np.uint64)
    lst = m0[0][grp_]
    idx = np.where(lag < lst, lst - lag, np.uint64(0))
    trm = np.where(rng.random(Gs) < 0.01, 6, 7).astype(np.uint64)
    cpu1 = cpu_rate(lambda: oc.appresp_sequential(n, Gs, (grp_, flg, idx, trm), st), Gs)
    reporter("streaming tracker (bucketed step)", G, t, algo,
           {"two_call_us": t_two * 1e6, "atomic_apply_us": t_apply * 1e6,
            "workload": f"{G} groups x 5 voters, {G} records per step (streaming: {E} new "
                        f"entries per step), 1% stale-term; last step: {applied_last} applied, "
                        f"{advanced_last} commits advanced",
            "commit_advance_us": t_commit * 1e6, "unit": "group-steps/s",
            "cpu_baseline": {"value": cpu1, "unit": "group-steps/s", "cores": 1, "kind": "port",
                             "sample": f"{Gs} records on {Gs} groups, sequential C restatement"}})


def wire_tracker_tick(G, nb, E=64, seed=77, dev_=None):
    """The composed per-tick workload (VERDICT r4 Missing 3): G 5-voter groups
    (FIXED layout, leader term 20007 since B = 2^35), nb ticks of G MsgAppResp
    each, encoded as gogoproto bytes on the device (wire.encode_appresp), from
    a random follower of a random group, 1 % stale-term (20006); tick k acks
    last + (k+1)·E − lag.  Returns (tracker, snapshot, ticks, rows, off, ids):
    tick = (buf, nbytes, msg_off, msg_group, direct AppRespBatch)."""
    from etcd_amd.quorum import wire
    d = dev_ or dev
    n = 5
    B = 1 << 35
    gen = torch.Generator(device=d)
    gen.manual_seed(seed)
    tr = batch.FixedTracker(n, G, d)
    last = B + 1024 + torch.randint(0, 1 << 20, (G,), generator=gen, device=d, dtype=torch.int64)
    tr.match[0].copy_(last + nb * E)  # the leader's own match (raft.go:747-748 appendEntry)
    for s_ in range(1, n):
        tr.match[s_].copy_(last - torch.randint(0, 200, (G,), generator=gen, device=d,
                                                dtype=torch.int64))
    tr.term.fill_(20007)
    tr.term_start.fill_(B)
    tr.commit_advance()
    off = torch.arange(0, n * G + 1, n, dtype=torch.int32, device=d)
    gg = torch.arange(G, dtype=torch.int64, device=d)
    ids = (16384 + torch.arange(n, dtype=torch.int64, device=d)[None, :] * 200000
           + (gg % 100000)[:, None]).reshape(-1)  # ascending per group
    rows = wire.group_rows(off, ids)
    ticks = []
    for k in range(nb):
        group = torch.randint(0, G, (G,), generator=gen, device=d, dtype=torch.int64)
        slot = torch.randint(1, n, (G,), generator=gen, device=d, dtype=torch.int64)
        lag = torch.randint(0, 96, (G,), generator=gen, device=d, dtype=torch.int64)
        index = last[group] + (k + 1) * E - lag
        term = torch.where(torch.rand(G, generator=gen, device=d) < 0.01, 20006, 20007)
        to = ids[group * n]
        frm = ids[group * n + slot]
        rej = torch.zeros(G, dtype=torch.bool, device=d)
        buf, nbytes, moff = wire.encode_appresp(to, frm, term, index, rej)
        direct = batch.AppRespBatch(group.to(torch.int32), slot.to(torch.uint8), index,
                                    term.to(torch.int64))
        ticks.append((buf, nbytes, moff, group.to(torch.int32), direct))
    snap = {k_: getattr(tr, k_).clone() for k_ in ("match", "committed", "active", "stepdown_at")}
    return tr, snap, ticks, rows, off, ids


def wire_tracker_csr_tick(G, nb, E=64, seed=79, dev_=None):
    """The composed workload over the CSR tracker (configs[2]'s ragged groups:
    3-9 voters + 0-2 learners, BASELINE configs[4]'s streaming step): G groups,
    nb ticks of G device-encoded MsgAppResp from a random non-leader slot of a
    random group, leader term 20007 (1 % stale 20006), indexes past 2^35 (6-byte
    varints); slot IDs ascending per group (3-byte varints).  Returns (tracker,
    snapshot, ticks, rows, off, ids) as wire_tracker_tick."""
    import bench
    from etcd_amd.quorum import wire
    d = dev_ or dev
    B = 1 << 35
    grp = batch.CsrGroups.synth(bench.CSR_SEED["ragged"], "ragged", G, device=d)
    tr = batch.CsrTracker(grp.off, grp.cfg, max_slots=grp.max_slots, device=d)
    del grp
    gen = torch.Generator(device=d)
    gen.manual_seed(seed)
    sizes = (tr.off[1:] - tr.off[:-1]).long()
    first = tr.off[:-1].long()
    gidx = torch.repeat_interleave(torch.arange(G, device=d), sizes)
    # the leader (slot 0) at last, followers up to 200 behind (6-byte varints)
    last = B + 1024 + torch.randint(0, 1 << 20, (G,), generator=gen, device=d, dtype=torch.int64)
    tr.match.copy_(last[gidx] - torch.randint(0, 200, (tr.S,), generator=gen, device=d,
                                              dtype=torch.int64))
    tr.match[first] = last
    tr.term.fill_(20007)
    tr.term_start.copy_(last - 64)
    tr.commit_advance()
    sl = torch.arange(tr.S, device=d) - first[gidx]
    ids = 16384 + sl * 100000 + (gidx % 100000)  # ascending per group
    rows = wire.group_rows(tr.off, ids)
    ticks = []
    for k in range(nb):
        group = torch.randint(0, G, (G,), generator=gen, device=d, dtype=torch.int64)
        r_ = torch.randint(0, 1 << 30, (G,), generator=gen, device=d, dtype=torch.int64)
        slot = 1 + r_ % (sizes[group] - 1)
        lag = torch.randint(0, 96, (G,), generator=gen, device=d, dtype=torch.int64)
        index = last[group] + (k + 1) * E - lag
        term = torch.where(torch.rand(G, generator=gen, device=d) < 0.01, 20006, 20007)
        rej = torch.zeros(G, dtype=torch.bool, device=d)
        buf, nbytes, moff = wire.encode_appresp(ids[first[group]], ids[first[group] + slot], term,
                                                index, rej)
        direct = batch.AppRespBatch(group.to(torch.int32), slot.to(torch.uint8), index,
                                    term.to(torch.int64))
        ticks.append((buf, nbytes, moff, group.to(torch.int32), direct))
    tr.match[first] = last + nb * E  # the leader appended nb * E entries
    snap = {k_: getattr(tr, k_).clone() for k_ in ("match", "committed", "active", "stepdown_at")}
    return tr, snap, ticks, rows, tr.off, ids


def wire_tracker_config(G, reps, warm=4, regions=3, *, reporter=None, gpu_only=None,
                        fused_only=False, csr=False):
    """Composed row: wire bytes -> tracker tick, per tick (rafthttp/stream.go:466
    decode -> raft.go:1106-1259 stepLeader MsgAppResp -> maybeCommit), G
    groups and G messages per tick, in one call (round 6:
    qb_dev_ingest_fixed_tracker_step — the decoder writes the tracker step's
    level-1 buckets, no record columns between them); beside it the chain of
    round 5 (qb_dev_ingest_messages_rows -> records -> qb_dev_fixed_tracker_step)
    and its two halves.  Parity in the row (size-independent): every status
    OK and the tracker state after the ticks through the one call equals the
    state the direct step (same columns, no wire) reaches, and so does the
    chain's (its decoded columns equal the encoded ones) — bit-exact.  The GPU
    suite checks both against the C oracles (tests/test_gpu_wire.py,
    tests/test_gpu_wire_tracker.py)."""
    reporter = reporter or report
    from etcd_amd.quorum import wire
    nb = warm + reps
    tr, snap, ticks, rows, off, ids = (wire_tracker_csr_tick if csr else wire_tracker_tick)(G, nb)
    sp = torch.cuda.current_stream(dev).cuda_stream

    def restore():
        for k_, v_ in snap.items():
            getattr(tr, k_).copy_(v_)

    def chain(tk):
        ib, _, _ = wire.ingest(tk[0], tk[1], tk[2], tk[3], off, ids, rows=rows)
        tr.step(batch.AppRespBatch(ib.group, ib.flags, ib.index, ib.term))

    def fused(tk):
        wire.ingest_tracker_step(tr, tk[0], tk[1], tk[2], tk[3], rows=rows, ids=ids)

    def timed(fn):
        ev = HipEvents(2)
        ts = []
        for r in range(regions + 1):
            restore()
            for k in range(warm):
                fn(ticks[k])
            torch.cuda.synchronize()
            ev.record(ev.ev[0], sp)
            for k in range(warm, nb):
                fn(ticks[k])
            ev.record(ev.ev[1], sp)
            torch.cuda.synchronize()
            if r:
                ts.append(ev.elapsed_ms(0, 1) / 1e3 / reps)
        ev.close()
        return float(np.median(ts))
    t = timed(fused)
    if fused_only:  # development A/B: the one call alone
        t_chain = t_ingest = t_step = float("nan")
    else:
        t_chain = timed(chain)
        t_ingest = timed(lambda tk: wire.ingest(tk[0], tk[1], tk[2], tk[3], off, ids, rows=rows))
        t_step = timed(lambda tk: tr.step(tk[4]))
    # parity: the one call and the chain against the direct step over every tick
    bad = 0
    restore()
    for tk in ticks:
        status = wire.ingest_tracker_step(tr, tk[0], tk[1], tk[2], tk[3], rows=rows, ids=ids)
        bad += int((status != 0).sum())
    via_fused = {k_: getattr(tr, k_).clone() for k_ in snap}
    restore()
    for tk in ticks:
        ib, status, _ = wire.ingest(tk[0], tk[1], tk[2], tk[3], off, ids, rows=rows)
        d = tk[4]
        bad += int((status != 0).sum()) + int((ib.group != d.group).sum())
        bad += int((ib.flags != d.flags).sum()) + int((ib.index != d.index).sum())
        bad += int((ib.term != d.term).sum())
        tr.step(batch.AppRespBatch(ib.group, ib.flags, ib.index, ib.term))
    via_wire = {k_: getattr(tr, k_).clone() for k_ in snap}
    restore()
    for tk in ticks:
        tr.step(tk[4])
    for k_ in snap:
        bad += int((getattr(tr, k_) != via_wire[k_]).sum())
        bad += int((getattr(tr, k_) != via_fused[k_]).sum())
    nbytes = ticks[0][1]
    del ticks
    # algorithmic bytes per message: its wire bytes, msg_off 8, envelope group
    # 4, the group's slot IDs 40 (wire row), its status byte 1; the tracker's
    # match RMW 16 and the commit advance 64 per group (configs[4] row) — the
    # decoded records are intermediate, not algorithmic
    if csr:  # the CSR step's row (configs[4] CSR: 117 B per group-step; slot IDs 8 B each)
        sl = float((off[-1].item()) / G)
        algo = nbytes + G * (8 + 4 + 8 * sl + 1) + G * (117 - 21)
    else:
        algo = nbytes + G * (8 + 4 + 40 + 1) + G * (16 + 64)
    reporter("wire -> tracker-csr tick (composed)" if csr else "wire -> tracker tick (composed)",
             G, t, algo,
             {"unit": "group-steps/s",
              "form": "one call (qb_dev_ingest_%s_tracker_step)" % ("csr" if csr else "fixed"),
              "chain_us": t_chain * 1e6, "chain_ingest_us": t_ingest * 1e6,
              "chain_tracker_step_us": t_step * 1e6,
              "bytes_per_message": nbytes / G,
              "parity": "bit-exact" if bad == 0 else f"MISMATCH {bad}",
              "parity_check": f"{nb} ticks of {G} messages: every status OK; tracker state "
                              "(match, committed, active, stepdown_at) through the one call == "
                              "through the chain == the direct step's; the chain's decoded "
                              "columns == the encoded columns"})
    if bad:
        raise AssertionError(f"wire -> tracker tick: {bad} mismatches")


def leader_row_parity(kind, Gs=1 << 18):
    """The row's own parity (bench next_rows): the same workload generator at
    Gs groups through both entry points (the group-ordered array and the
    outbox), every state array, message, step-down entry and group flag
    against the C oracle (oracle/leader_oracle.c, the stepLeader loop one
    record at a time); the streaming leader for two consecutive batches.
    Returns "bit-exact" or the mismatching fields."""
    from etcd_amd.quorum.leader import (readindex_inbox, streaming_inbox, synth_readindex,
                                        synth_streaming)
    from tests import oracle_c as oc
    bad = []
    forms = (False, True, "read_states") if kind == "readindex" else (False, True)
    for outbox in forms:
        name = {False: "ordered", True: "outbox", "read_states": "outbox+read_states"}[outbox]
        if kind == "leader":
            lg, base = synth_streaming(Gs, device=dev)
            inboxes = [streaming_inbox(Gs, base, k, device=dev) for k in range(2)]
            Q, cap = 0, 6 * Gs
        else:
            lg, last_ctx, _ = synth_readindex(Gs, 4, device=dev)
            inboxes = [readindex_inbox(Gs, last_ctx, device=dev)]
            Q, cap = 4, 8 * Gs
        host = {k: v.copy() for k, v in lg.numpy().items()}
        for k, ib in enumerate(inboxes):
            if outbox == "read_states":
                res = lg.step_outbox(ib, read_states=True)
            else:
                res = lg.step_outbox(ib) if outbox else lg.step(ib, msg_cap=cap)
            rec = {"group": ib.group.cpu().numpy().view(np.uint32), "flags": ib.flags.cpu().numpy(),
                   "index": ib.index.cpu().numpy().view(np.uint64),
                   "term": ib.term.cpu().numpy().view(np.uint64),
                   "hint": ib.hint.cpu().numpy().view(np.uint64),
                   "log_term": ib.log_term.cpu().numpy().view(np.uint64)}
            msgs, total, sd, gf, _ = oc.leader_step(host, lg.inflight_cap, Q, 0, rec, threads=16,
                                                    msg_cap=cap)
            dev_state = lg.numpy()
            bad += [f"{name} step {k}: {n}" for n in host
                    if not np.array_equal(dev_state[n], host[n])]
            if outbox == "read_states":  # the local answers as ReadStates, the rest as messages
                local = msgs["type"] == 255
                roff = np.zeros(Gs + 1, np.int64)
                roff[1:] = np.cumsum(np.bincount(msgs["group"][local], minlength=Gs))
                if not (local.any() and total == len(msgs)
                        and np.array_equal(res.read_states["index"], msgs["index"][local])
                        and np.array_equal(res.read_states["ctx"], msgs["aux"][local])
                        and np.array_equal(res.read_off, roff)):
                    bad.append(f"{name} step {k}: read states")
                msgs = msgs[~local]
                total = len(msgs)
            if res.msg_total != total or not np.array_equal(res.msgs.view(np.uint8),
                                                            msgs.view(np.uint8)):
                bad.append(f"{name} step {k}: messages")
            if not (np.array_equal(res.stepdown_at, sd) and np.array_equal(res.gflags, gf)):
                bad.append(f"{name} step {k}: stepdown / flags")
        del lg
    torch.cuda.empty_cache()
    return "bit-exact" if not bad else "MISMATCH " + "; ".join(bad[:6])


def leader_config(G, reps, warm=4, shuffle=True, *, reporter=None, gpu_only=None):
    """§8f rows 1-2: the leader inbox step (qb_dev_leader_step) on streaming
    MsgAppResp batches (one per group per step), group-steps/s."""
    reporter = reporter or report
    gpu_only = GPU_ONLY if gpu_only is None else gpu_only
    from etcd_amd.quorum.leader import synth_streaming, streaming_inbox
    lg, base = synth_streaming(G, device=dev)
    steps = warm + reps
    inboxes = [streaming_inbox(G, base, k, device=dev, shuffle=shuffle) for k in range(steps)]
    stats = torch.zeros(8, dtype=torch.int64, device=dev)
    sp = torch.cuda.current_stream(dev).cuda_stream
    snap = {k: v.clone() for k, v in lg.t.items()}

    def timed(step):
        # the same start state and the same `steps` batches for each form
        for k_, v_ in snap.items():
            lg.t[k_].copy_(v_)
        for k in range(warm):
            step(inboxes[k])
        torch.cuda.synchronize()
        stats.zero_()
        ev = HipEvents(2)
        ev.record(ev.ev[0], sp)
        for k in range(warm, steps):
            step(inboxes[k])
        ev.record(ev.ev[1], sp)
        torch.cuda.synchronize()
        dt = ev.elapsed_ms(0, 1) / 1e3 / reps
        ev.close()
        return dt, stats.cpu().tolist()
    # the group-ordered array (qb_dev_leader_step: step, scan, copy) and the
    # per-group outbox the step writes (qb_dev_leader_step_outbox)
    t_ord, st = timed(lambda ib: lg.step(ib, msg_cap=6 * G, stats=stats, fetch=False))
    t, st_ob = timed(lambda ib: lg.step_outbox(ib, stats=stats, fetch=False))
    assert st_ob[6] == st[6], "outbox and ordered forms generated different message counts"
    msgs = st[6] / reps
    # per group-step: record 21 B; group state read 84 B (off 4, cfg 4, meta 4,
    # term/committed/first/last/snap/snap_term/max_ents 56, run 16) + commit
    # and meta written 12 B; 5 slots x (match, next, psnap 24 + pstate 1 +
    # infl_pos 4) read 145 B; the acking follower's freed window entry 8 B and
    # match/next/pstate/infl_pos written 21 B; the record grouping's scan 8 B
    # per group; messages: the outbox form writes each 40 B message once and
    # a 4 B count per group; the ordered form stores, re-reads and writes
    # each (40 B x 3) and scans the counts (8 B per group).
    base = G * (21 + 84 + 12 + 145 + 8 + 21 + 8)
    algo = base + G * 4 + msgs * 40
    algo_ord = base + G * 8 + msgs * 40 * 3
    ordered = {"ordered_us": t_ord * 1e6, "ordered_algo_bytes": algo_ord,
               "ordered_frac": algo_ord / t_ord / 1e9 / HBM_PEAK_GBS,
               "form": "qb_dev_leader_step_outbox (per-group outbox); ordered_* = "
                       "qb_dev_leader_step (group-ordered array)"}
    if not shuffle or gpu_only:
        extra = {"unit": "group-steps/s", "msgs_per_step": msgs, **ordered}
        if shuffle and reporter is not report:  # the default run's next_rows: the row's own parity
            extra["parity"] = leader_row_parity("leader")
            extra["parity_check"] = ("the same stream at 256K groups, two batches, ordered and "
                                     "outbox forms vs the C oracle: state, messages, step-downs")
        reporter("leader inbox step" + ("" if shuffle else ", records in group order (lab)"), G, t,
                 algo, extra)
        return
    # CPU beside it: the C restatement (oracle/leader_oracle.c, the Go
    # stepLeader loop one record at a time) on a bounded sample of the same
    # workload, 16 threads (groups partitioned) and 1 thread.
    import time
    from tests import oracle_c as oc
    Gs = 1 << 20
    lgc, basec = synth_streaming(Gs, device="cpu")
    cpu = {}
    for threads in (16, 1):
        host = {k: v.copy() for k, v in lgc.numpy().items()}
        t0 = time.perf_counter()
        n_steps = 0
        while True:
            ib = streaming_inbox(Gs, basec, n_steps, device="cpu")
            rec = {"group": ib.group.numpy().view(np.uint32), "flags": ib.flags.numpy(),
                   "index": ib.index.numpy().view(np.uint64),
                   "term": ib.term.numpy().view(np.uint64),
                   "hint": ib.hint.numpy().view(np.uint64),
                   "log_term": ib.log_term.numpy().view(np.uint64)}
            t1 = time.perf_counter()
            oc.leader_step(host, 32, 0, 0, rec, threads=threads, msg_cap=6 * Gs)
            n_steps += 1
            cpu.setdefault(threads, 0.0)
            cpu[threads] += time.perf_counter() - t1
            if time.perf_counter() - t0 > 6 or n_steps >= 24:
                break
        cpu[threads] = n_steps * Gs / cpu[threads]
    reporter("leader inbox step (streaming MsgAppResp)", G, t, algo,
           {"unit": "group-steps/s", "msgs_per_step": msgs,
            "applied_per_step": st[0] / reps, "inflight_cap": 32, "voters": 5,
            "cpu_baseline": {"value": cpu[16], "unit": "group-steps/s", "cores": 16,
                             "kind": "port", "value_1thread": cpu[1],
                             "sample": f"{Gs} groups x consecutive steps of the same workload, "
                                       "C restatement of stepLeader (oracle/leader_oracle.c)"}})


def wire_config(M, reps, G=None, rows=False, *, reporter=None, gpu_only=None):
    """§8f row 3: wire ingest of M gogoproto-encoded responses (MsgAppResp +
    10% MsgHeartbeatResp with read contexts) to M/4 5-voter leaders (G given:
    a development variant with a small, cache-resident group table)."""
    reporter = reporter or report
    gpu_only = GPU_ONLY if gpu_only is None else gpu_only
    from etcd_amd.quorum import wire
    from tests import oracle_c as oc
    G = G or M // 4
    buf, moff, grp, off, ids = wire.synth_response_stream(M, G)
    d_buf = torch.from_numpy(buf).to(dev)
    d_moff = torch.from_numpy(moff.view(np.int64)).to(dev)
    d_grp = torch.from_numpy(grp.view(np.int32)).to(dev)
    d_off = torch.from_numpy(off.view(np.int32)).to(dev)
    d_ids = torch.from_numpy(ids.view(np.int64)).to(dev)
    nb = int(moff[-1])
    d_rows = wire.group_rows(d_off, d_ids) if rows else None  # once per config
    t = time_region(lambda: wire.ingest(d_buf, nb, d_moff, d_grp, d_off, d_ids, rows=d_rows),
                    reps)
    # bytes read: message bytes + offset 8 + envelope group 4 + the group's
    # slot IDs 40 (5 x u64, read once per message); written: group 4, flags
    # 1, index/term/hint/log_term 32, status 1, type 1
    algo = nb + M * (8 + 4 + 40) + M * (4 + 1 + 32 + 1 + 1)
    if gpu_only:
        extra = {"unit": "messages/s", "bytes_per_message": nb / M}
        if reporter is not report:  # the default run's next_rows: the row's own parity
            ib, status, mtype = wire.ingest(d_buf, nb, d_moff, d_grp, d_off, d_ids, rows=d_rows)
            want = oc.ingest(buf, moff, grp, off, ids, threads=16)
            got = {"group": ib.group.cpu().numpy().view(np.uint32), "flags": ib.flags.cpu().numpy(),
                   "index": ib.index.cpu().numpy().view(np.uint64)[:M],
                   "term": ib.term.cpu().numpy().view(np.uint64)[:M],
                   "hint": ib.hint.cpu().numpy().view(np.uint64)[:M],
                   "log_term": ib.log_term.cpu().numpy().view(np.uint64)[:M],
                   "status": status.cpu().numpy()}
            bad = [n for n in got if not np.array_equal(got[n][:M], want[n])]
            extra["parity"] = "bit-exact" if not bad else "MISMATCH " + ", ".join(bad)
            extra["parity_check"] = (f"all {M} messages decoded by the device and by the C "
                                     "restatement of Message.Unmarshal + ingest "
                                     "(oracle/wire_oracle.c): every record column and status")
        reporter("wire ingest" + (" (group rows)" if rows else ""), M, t, algo, extra)
        return
    import time
    Ms = 1 << 22
    cpu = {}
    for threads in (16, 1):
        reps_c, t0 = 0, time.perf_counter()
        while True:
            oc.ingest(buf[: int(moff[Ms])], moff[: Ms + 1], grp[:Ms], off, ids, threads=threads)
            reps_c += 1
            if time.perf_counter() - t0 > 4:
                break
        cpu[threads] = reps_c * Ms / (time.perf_counter() - t0)
    reporter("wire ingest (raftpb.Message -> leader inbox)" + (", group rows" if rows else ""),
           M, t, algo,
           {"unit": "messages/s", "bytes_per_message": nb / M,
            "input_GBs": nb / t / 1e9,
            "cpu_baseline": {"value": cpu[16], "unit": "messages/s", "cores": 16, "kind": "port",
                             "value_1thread": cpu[1],
                             "sample": f"{Ms} messages of the same stream, C restatement of "
                                       "gogoproto Message.Unmarshal + ingest (oracle/wire_oracle.c)"}})


def _confchange_row_parity(table, op, cc_off, cc_type, cc_node, last, t, K):
    """The conf change row's expected result, checked whole on the device:
    every group's Simple(AddLearnerNode 6) over voters 1-5."""
    from etcd_amd.quorum.leader import PR_RECENT_ACTIVE
    nt, err, _ = table.change_soa(op, cc_off, cc_type, cc_node, last, fetch_errors=False)
    G = table.G
    S = 6 * G
    bad = []
    ar = torch.arange(S, device=dev)
    slot, g = ar % 6, ar // 6
    carried = slot < 5
    src = g * 5 + slot.clamp(max=4)
    checks = {
        "err": bool((err != 0).any()),
        "off": not torch.equal(nt.t["off"].long()[: G + 1],
                               torch.arange(0, S + 1, 6, device=dev)),
        "ids": not torch.equal(nt.t["ids"][:S], slot + 1),
        "cfg": not torch.equal(nt.t["cfg"][:G], t["cfg"]),
        "ext": not torch.equal(nt.t["ext"][:G], t["ext"]),
        "match": not torch.equal(nt.t["match"][:S], torch.where(carried, t["match"][src], 0)),
        "next": not torch.equal(nt.t["next"][:S], torch.where(carried, t["next"][src], last[g])),
        "pending_snapshot": not torch.equal(nt.t["pending_snapshot"][:S],
                                            torch.where(carried, t["pending_snapshot"][src], 0)),
        "pstate": not torch.equal(nt.t["pstate"][:S].long(),
                                  torch.where(carried, t["pstate"][src].long(),
                                              torch.full_like(ar, PR_RECENT_ACTIVE))),
        "infl_pos": not torch.equal(nt.t["infl_pos"][:S].long(),
                                    torch.where(carried, t["infl_pos"][src].long(), 0)),
        "infl_buf": not torch.equal(nt.t["infl_buf"][: S * K].view(S, K),
                                    torch.where(carried[:, None], t["infl_buf"].view(-1, K)[src], 0)),
    }
    bad = [k for k, v in checks.items() if v]
    del nt
    return "bit-exact" if not bad else "MISMATCH " + ", ".join(bad)


def confchange_config(G, reps, *, reporter=None, gpu_only=None):
    """§8f row 4: one Changer.Simple(AddLearnerNode) per group over G 5-voter
    groups (Progress carried for 5 slots, initialised for the new one),
    groups/s; CPU beside it: the Python restatement on a small sample."""
    reporter = reporter or report
    gpu_only = GPU_ONLY if gpu_only is None else gpu_only
    import time
    from etcd_amd.quorum.confchange import ConfigTable, ADD_LEARNER, SIMPLE
    from oracle import confchange_ref as CC
    K = 4
    S = 5 * G
    off = torch.arange(0, S + 1, 5, dtype=torch.int32, device=dev)
    ids = (torch.arange(S, dtype=torch.int64, device=dev) % 5) + 1
    t = {"off": off, "ids": ids,
         "cfg": torch.full((G,), 0x1F, dtype=torch.int32, device=dev),
         "ext": torch.zeros(G, dtype=torch.int32, device=dev),
         "match": torch.arange(S, dtype=torch.int64, device=dev),
         "next": torch.arange(S, dtype=torch.int64, device=dev) + 1,
         "pending_snapshot": torch.zeros(S, dtype=torch.int64, device=dev),
         "pstate": torch.full((S,), 1 | 8, dtype=torch.uint8, device=dev),
         "infl_pos": torch.zeros(S, dtype=torch.int32, device=dev),
         "infl_buf": torch.zeros(S * K, dtype=torch.int64, device=dev)}
    table = ConfigTable(G, S, K, t)
    op = torch.full((G,), SIMPLE, dtype=torch.uint8, device=dev)
    cc_off = torch.arange(G + 1, dtype=torch.int32, device=dev)
    cc_type = torch.full((G,), ADD_LEARNER, dtype=torch.uint8, device=dev)
    cc_node = torch.full((G,), 6, dtype=torch.int64, device=dev)
    last = torch.full((G,), 100, dtype=torch.int64, device=dev)
    tt = time_region(lambda: table.change_soa(op, cc_off, cc_type, cc_node, last,
                                              fetch_errors=False), reps)
    # read: off 4, ids 40, cfg/ext 8, op 1, cc_off 4, cc 9, last 8, Progress
    # 5 x (8+8+8+1+4+K*8); written: new_off 4, ids 48, cfg/ext 8, Progress
    # 6 x (29 + K*8), err 1, err_id 8
    pr = 29 + 8 * K
    algo = G * (4 + 40 + 8 + 1 + 4 + 9 + 8 + 5 * pr + 4 + 48 + 8 + 6 * pr + 9)
    if gpu_only:
        extra = {"unit": "groups/s"}
        if reporter is not report:  # the default run's next_rows: the row's own parity
            extra["parity"] = _confchange_row_parity(table, op, cc_off, cc_type, cc_node, last, t, K)
            extra["parity_check"] = (f"all {G} groups: Simple(AddLearnerNode 6) on voters 1-5 gives "
                                     "slots 1-6, the voter mask unchanged, slots 1-5's Progress "
                                     "and rings carried, slot 6 initProgress (confchange.go:"
                                     "258-281), no error — checked on the device")
        reporter("conf change", G, tt, algo, extra)
        return
    n = 20000
    trs = []
    for _ in range(n):
        tr = CC.Tracker.empty(K)
        tr.voters_in = {1, 2, 3, 4, 5}
        tr.prs = {i: CC.Pr(match=i, next=i + 1, state=1, recent_active=True) for i in range(1, 6)}
        trs.append(tr)
    t0 = time.perf_counter()
    for tr in trs:
        CC.Changer(tr, 100).simple([(CC.ADD_LEARNER, 6)])
    cpu1 = n / (time.perf_counter() - t0)
    reporter("conf change (Simple AddLearner, 5 -> 6 slots)", G, tt, algo,
           {"unit": "groups/s", "cpu_baseline": {
               "value": cpu1, "unit": "groups/s", "cores": 1, "kind": "port",
               "sample": f"{n} groups, Python restatement of confchange.Changer (oracle)"}})


def readindex_config(G, reps, Q=4, *, reporter=None, gpu_only=None):
    """§8f row 2: ReadIndex acks — two heartbeat responses per leader carrying
    the latest read context; the quorum releases all Q pending reads
    (MsgReadIndexResp / ReadState).  The read queues are restored before each
    step outside the timed launches (new MsgReadIndex requests are the
    host's).  Also CheckQuorum: QuorumActive over 16M CSR groups."""
    reporter = reporter or report
    gpu_only = GPU_ONLY if gpu_only is None else gpu_only
    from etcd_amd.quorum.leader import synth_readindex, readindex_inbox
    lg, last_ctx, pristine = synth_readindex(G, Q, device=dev)
    inboxes = [readindex_inbox(G, last_ctx, device=dev) for _ in range(reps + 2)]
    stats = torch.zeros(8, dtype=torch.int64, device=dev)
    sp = torch.cuda.current_stream(dev).cuda_stream

    def timed(step):
        ev = HipEvents(2)
        times = []
        for k in range(reps + 2):
            for name, t0 in pristine.items():
                lg.t[name].copy_(t0)
            if k == 2:
                stats.zero_()
            ev.record(ev.ev[0], sp)
            step(inboxes[k])
            ev.record(ev.ev[1], sp)
            torch.cuda.synchronize()
            if k >= 2:
                times.append(ev.elapsed_ms(0, 1) / 1e3)
        ev.close()
        return float(np.median(times)), stats.cpu().tolist()
    t_ord, st = timed(lambda ib: lg.step(ib, msg_cap=8 * G, stats=stats, fetch=False))
    t_msg, st_ob = timed(lambda ib: lg.step_outbox(ib, stats=stats, fetch=False))
    assert st_ob[6] == st[6], "outbox and ordered forms generated different message counts"
    # the row's form: the outbox with its ReadState area — a local read's
    # answer is a ReadState (raft.go:1737-1745, Ready.ReadStates), not a message
    t, st_rs = timed(lambda ib: lg.step_outbox(ib, stats=stats, fetch=False, read_states=True))
    local_reads = (st[6] - st_rs[6]) / reps  # the ReadStates per step (out of the messages)
    # per group-step: 2 records 2 x 21 B, group state 84 B, 5 slots x 29 B,
    # read queue Q x 20 B read + written, the grouping scan 8 B; then the
    # answers: the row's form 40 B per message + 16 B per ReadState + two 4 B
    # counts per group; every answer a message (messages_*) 40 B each + a 4 B
    # count; the ordered form 40 B x 3 + the count scan 8 B per group
    base = G * (42 + 84 + 145 + Q * 20 * 2 + 8)
    algo = base + G * 8 + (st_rs[6] / reps) * 40 + local_reads * 16
    algo_msg = base + G * (4 + Q * 40)
    algo_ord = base + G * (8 + Q * 40 * 3)
    ordered = {"messages_us": t_msg * 1e6, "messages_algo_bytes": algo_msg,
               "messages_frac": algo_msg / t_msg / 1e9 / HBM_PEAK_GBS,
               "ordered_us": t_ord * 1e6, "ordered_algo_bytes": algo_ord,
               "ordered_frac": algo_ord / t_ord / 1e9 / HBM_PEAK_GBS,
               "read_states_per_step": local_reads,
               "form": "qb_dev_leader_step_outbox with its ReadState area (local answers as "
                       "16-byte ReadStates, follower answers as MsgReadIndexResp); messages_* = "
                       "the same outbox with every answer a message (rounds 4-5's row); "
                       "ordered_* = qb_dev_leader_step (group-ordered array)"}
    # CheckQuorum: QuorumActive over 16M groups (cfg u32 + active u16 -> u8)
    grp = batch.CsrGroups.synth(0x5EED0003, "ragged", 1 << 24, device=dev)
    active = torch.randint(-(1 << 15), 1 << 15, (1 << 24,), dtype=torch.int16, device=dev)
    tq = time_region(lambda: grp.quorum_active(active), 20)
    cq = {"read_queue": Q, "check_quorum_16M_us": tq * 1e6,
          "check_quorum_groups_per_s": (1 << 24) / tq,
          "check_quorum_GBs": (1 << 24) * 7 / tq / 1e9}
    if gpu_only:
        extra = {"unit": "group-steps/s", "reads_released_per_step": st[6] / reps, **cq, **ordered}
        if reporter is not report:  # the default run's next_rows: the row's own parity
            extra["parity"] = leader_row_parity("readindex")
            extra["parity_check"] = ("the same workload at 256K groups, ordered, outbox and "
                                     "outbox + ReadState forms vs the C oracle: queues, released "
                                     "reads, every message and ReadState")
        reporter("ReadIndex acks (leader step, heartbeat responses)", G, t, algo, extra)
        return
    # CPU beside it: the C restatement on 1M groups of the same workload
    import time
    from tests import oracle_c as oc
    Gs = 1 << 20
    lgc, ctxc, _ = synth_readindex(Gs, Q, device="cpu")
    ibc = readindex_inbox(Gs, ctxc, device="cpu")
    recc = {"group": ibc.group.numpy().view(np.uint32), "flags": ibc.flags.numpy(),
            "index": ibc.index.numpy().view(np.uint64), "term": ibc.term.numpy().view(np.uint64),
            "hint": ibc.hint.numpy().view(np.uint64),
            "log_term": ibc.log_term.numpy().view(np.uint64)}
    cpu = {}
    for threads in (16, 1):
        host = {k_: v.copy() for k_, v in lgc.numpy().items()}
        t1 = time.perf_counter()
        oc.leader_step(host, lgc.inflight_cap, Q, 0, recc, threads=threads, msg_cap=8 * Gs)
        cpu[threads] = Gs / (time.perf_counter() - t1)
    reporter("ReadIndex acks (leader step, heartbeat responses)", G, t, algo,
           {"unit": "group-steps/s", "reads_released_per_step": st[6] / reps, **ordered,
            "cpu_baseline": {"value": cpu[16], "unit": "group-steps/s", "cores": 16,
                             "kind": "port", "value_1thread": cpu[1],
                             "sample": f"{Gs} groups, one step, C restatement (oracle)"},
            **cq})


def tick_config(G, reps, *, reporter=None):
    """The batched raft tick (qb_dev_leader_tick): G five-voter leader groups
    of the synth_streaming state with etcd's defaults (ElectionTick 10,
    HeartbeatTick 1, CheckQuorum): every tick broadcasts, every tenth also
    sweeps.  A sample is ten consecutive ticks from zeroed counters — nine beat
    ticks and one that sweeps and beats — with one event per tick; the
    RecentActive bits the sweep clears and the counters are restored between
    samples, outside the timed ticks (the responses that set them again are
    the leader step's).  Parity: the same table at the same size with seeded
    RecentActive bits, counters, transfers and a share of non-leaders, ten
    ticks against the numpy restatement (tests/tick_pack.py np_tick, itself
    checked against tests/tick_ref.py in tests/test_tick_ref.py)."""
    reporter = reporter or report
    from etcd_amd.quorum import tick as qt
    from etcd_amd.quorum.leader import _to_np, synth_streaming
    from tests import tick_pack as P
    ET, HT, CQ, n, TICKS = 10, 1, 1, 5, 10
    lg, _ = synth_streaming(G, W=1, D=1, n=n, device=dev)
    S = lg.S
    z32 = lambda: torch.zeros(G, dtype=torch.int32, device=dev)  # noqa: E731
    state = qt.TickState(torch.full((G,), qt.ROLE_LEADER | qt.ROLE_PROMOTABLE, dtype=torch.uint8,
                                    device=dev), z32(), z32(),
                         torch.full((G,), 15, dtype=torch.int32, device=dev))
    pstate0 = lg.t["pstate"].clone()
    out = lg.tick(state, ET, HT, True)   # (the mirror's argument checks, once)
    sp = torch.cuda.current_stream(dev).cuda_stream
    # the timed calls go to the C ABI with the struct built once: the mirror's
    # per-call checks cost about as much host time as the kernel runs
    import ctypes as C
    from etcd_amd import _lib
    tg = qt.TickGroupsC(G=G, readq_cap=0, election_timeout=ET, heartbeat_timeout=HT,
                        check_quorum=CQ, rq_ctx=None,
                        **{k: lg.t[k].data_ptr() for k in ("off", "cfg", "meta", "committed", "match",
                                                           "pstate")},
                        role=state.role.data_ptr(),
                        election_elapsed=state.election_elapsed.data_ptr(),
                        heartbeat_elapsed=state.heartbeat_elapsed.data_ptr(),
                        rand_timeout=state.rand_timeout.data_ptr())
    fn = _lib.fn("qb_dev_leader_tick")
    args = (C.byref(tg), out.tflags.data_ptr(), out.hb_commit.data_ptr(), out.hb_ctx.data_ptr(),
            out.stats.data_ptr(), sp)

    def tick():
        _lib.check(fn(*args), "qb_dev_leader_tick")

    def restore():
        lg.t["pstate"].copy_(pstate0)
        state.election_elapsed.zero_()
        state.heartbeat_elapsed.zero_()

    def sample(ev):
        restore()
        torch.cuda.synchronize()
        for k in range(TICKS):
            ev.record(ev.ev[k], sp)
            tick()
        ev.record(ev.ev[TICKS], sp)
        torch.cuda.synchronize()
        return [ev.elapsed_ms(k, k + 1) / 1e3 for k in range(TICKS)]
    import time
    ev = HipEvents(TICKS + 1)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3:  # warm-up: clocks settle (time_region)
        sample(ev)
    out.stats.zero_()
    per = np.array([sample(ev) for _ in range(reps)])
    ev.close()
    st = out.stats_dict()
    assert st["beats"] == reps * TICKS * G and st["check_quorum"] == reps * G, st
    assert st["stepped_down"] == 0 and st["heartbeats"] == reps * TICKS * G * (n - 1), st
    t_tick = float(np.median(per.sum(axis=1))) / TICKS
    t_beat = float(np.median(per[:, :TICKS - 1]))
    t_sweep = float(np.median(per[:, TICKS - 1]))
    # per group and beat tick: off 4, role 1, both counters read and written
    # 16, meta 4, committed 8, tflags 1, hb_ctx 8 = 42 B, and per peer slot
    # match 8 in + hb_commit 8 out (the leader's own slot is not read);
    # the sweep tick adds cfg 4, the pstate bytes read (n) and the n - 1
    # cleared ones written
    beat_b = 42 + (n - 1) * 16
    sweep_b = beat_b + 4 + n + (n - 1)
    algo = G * (beat_b * (TICKS - 1) + sweep_b) / TICKS
    extra = {"unit": "group-ticks/s", "ticks_per_sample": TICKS, "samples": reps,
             "beat_tick_us": t_beat * 1e6, "beat_tick_bytes_per_group": beat_b,
             "beat_tick_frac": G * beat_b / t_beat / 1e9 / HBM_PEAK_GBS,
             "sweep_tick_us": t_sweep * 1e6, "sweep_tick_bytes_per_group": sweep_b,
             "sweep_tick_frac": G * sweep_b / t_sweep / 1e9 / HBM_PEAK_GBS,
             "election_tick": ET, "heartbeat_tick": HT, "check_quorum": CQ,
             "timing": "one HIP event per tick, median over samples of 10 consecutive ticks; "
                       "per_launch_us = median sample / 10"}
    # parity at this size
    gen = torch.Generator(device=dev).manual_seed(0x71C4)
    rnd = lambda hi, k: torch.randint(0, hi, (k,), generator=gen, device=dev)  # noqa: E731
    lg.t["pstate"].copy_((1 | (rnd(2, S) << 3)).to(torch.uint8))
    lg.t["meta"].copy_((lg.t["meta"] & ~0xFF00
                        | torch.where(rnd(8, G) == 0, rnd(n, G), torch.full((G,), 0xFF, device=dev))
                        << 8).to(torch.int32))
    role = torch.where(rnd(16, G) == 0, rnd(4, G), torch.full((G,), 2, device=dev)) | (rnd(2, G) << 7)
    state.role.copy_(role.to(torch.uint8))
    state.election_elapsed.copy_(rnd(ET + 6, G).to(torch.int32))
    state.heartbeat_elapsed.copy_(rnd(3, G).to(torch.int32))
    state.rand_timeout.copy_((ET + rnd(ET, G)).to(torch.int32))
    a = {k: _to_np(lg.t[k], dt).copy() for k, dt in (
        ("off", np.uint32), ("cfg", np.uint32), ("meta", np.uint32), ("committed", np.uint64),
        ("match", np.uint64), ("pstate", np.uint8))}
    t = {k: v.copy() for k, v in state.numpy(G).items()}
    fill = P.FILL - (1 << 64)
    out.hb_commit.fill_(fill)
    out.hb_ctx.fill_(fill)
    out.stats.zero_()
    hc, hx = np.full(S, P.FILL, np.uint64), np.full(G, P.FILL, np.uint64)
    want_st = {k: 0 for k in qt.TSTAT_NAMES}
    ok = True
    for k in range(TICKS):
        tick()
        tf, st1 = P.np_tick(a, t, 0, ET, HT, CQ, hc, hx)
        for key, v in st1.items():
            want_st[key] += v
        ok = ok and np.array_equal(out.tflags.cpu().numpy()[:G], tf)
    got_t = state.numpy(G)
    ok = (ok and all(np.array_equal(got_t[key], t[key]) for key in t)
          and np.array_equal(_to_np(lg.t["meta"], np.uint32, G), a["meta"])
          and np.array_equal(_to_np(lg.t["pstate"], np.uint8, S), a["pstate"])
          and np.array_equal(_to_np(out.hb_commit, np.uint64, S), hc)
          and np.array_equal(_to_np(out.hb_ctx, np.uint64, G), hx)
          and out.stats_dict() == want_st)
    extra["parity"] = bool(ok)
    extra["parity_check"] = (f"{G} groups, seeded RecentActive bits / counters / transfers / roles, "
                             f"{TICKS} ticks vs the numpy restatement of tests/tick_ref.py: tflags "
                             "every tick; counters, role, meta, pstate, hb_commit and hb_ctx "
                             "(untouched elements included) and the stats after the last: "
                             f"{want_st}")
    reporter("raft tick (heartbeats, CheckQuorum sweep, election timers)", G, t_tick, algo, extra)
    assert ok, "tick parity failed"


def follower_config(G, reps, *, reporter=None):
    """The batched follower step (qb_dev_follower_step): G follower groups
    (term 7, leader 1 known, CheckQuorum and PreVote on, ElectionTick 10).
    Heartbeat sample: M = G same-term MsgHeartbeat, one per group in shuffled
    arrival order, Commit one past the previous sample's (inside lastIndex), so
    every group commits and answers; electionElapsed is put back to 1 between
    samples (a tick passed), outside the timed call.  Storm sample: the lease
    has run out (electionElapsed 10); M = 2 G records in shuffled order, per
    group one MsgPreVote and then one MsgVote at term 8 from an up-to-date
    candidate: both granted, the vote through becomeFollower; the state is
    restored between samples, outside the timed call.  Parity at this size:
    tests/follower_ref.py over the records of every 1024th group (4096
    groups; exact, because groups are independent) — their state, responses,
    gflags and stop_at after one call of each sample."""
    reporter = reporter or report
    import ctypes as C
    from etcd_amd import _lib
    from etcd_amd.quorum import follower as qf, tick as qt
    from etcd_amd.quorum.leader import _to_np
    from tests import follower_ref as F
    ET, TERM = 10, 7
    i64 = lambda v: torch.full((G,), v, dtype=torch.int64, device=dev)  # noqa: E731
    g = torch.arange(G, dtype=torch.int64, device=dev)
    base = 1000 + (g * 37) % 1000
    t = {"term": i64(TERM), "vote": i64(1), "lead": i64(1), "committed": base.clone(),
         "last_index": base + 4096, "last_term": i64(TERM)}
    state = qt.TickState(torch.full((G,), qt.ROLE_PROMOTABLE, dtype=torch.uint8, device=dev),
                         torch.ones(G, dtype=torch.int32, device=dev),
                         torch.zeros(G, dtype=torch.int32, device=dev),
                         torch.full((G,), 15, dtype=torch.int32, device=dev))
    fg = qf.FollowerGroups(G, ET, True, True, t, state)
    pristine = {k: v.clone() for k, v in t.items()}

    def inbox_of(grp, flags, frm, term, index, aux):
        ib = qf.FollowerInbox(grp.to(torch.int32), flags.to(torch.uint8), frm, term, index, aux)
        ib._m = int(grp.numel())
        return ib
    # heartbeats: one per group, shuffled
    hg = torch.randperm(G, device=dev)
    hb = inbox_of(hg, torch.zeros_like(hg), torch.ones_like(hg), torch.full_like(hg, TERM),
                  base[hg] + 1, torch.zeros_like(hg))
    # storm: two per group, shuffled; the group's first is the MsgPreVote
    sg = torch.randperm(2 * G, device=dev) % G
    order = torch.argsort(sg, stable=True)
    rank = torch.empty_like(order)
    rank[order] = torch.arange(2 * G, device=dev) % 2
    storm = inbox_of(sg, torch.where(rank == 0, qf.FIN_PREVOTE, qf.FIN_VOTE),
                     torch.full_like(sg, 2), torch.full_like(sg, TERM + 1), (base + 4096)[sg],
                     torch.full_like(sg, TERM))
    res_hb = qf.follower_step(fg, hb)       # (the mirror's argument checks, once each)
    res_st = qf.follower_step(fg, storm)
    sp = torch.cuda.current_stream(dev).cuda_stream
    fgc = qf.FollowerGroupsC(G=G, election_timeout=ET, check_quorum=1, pre_vote=1, reserved=0,
                             role=state.role.data_ptr(),
                             election_elapsed=state.election_elapsed.data_ptr(),
                             heartbeat_elapsed=state.heartbeat_elapsed.data_ptr(),
                             **{k: v.data_ptr() for k, v in t.items()})
    fn = _lib.fn("qb_dev_follower_step")

    def caller(ib, res):
        ibc = qf.FollowerInboxC(M=ib.M, group=ib.group.data_ptr(), flags=ib.flags.data_ptr(),
                                term=ib.term.data_ptr(), index=ib.index.data_ptr(),
                                aux=ib.aux.data_ptr())
        setattr(ibc, "from", ib.frm.data_ptr())
        args = (C.byref(fgc), C.byref(ibc), res.resp_type.data_ptr(), res.resp_term.data_ptr(),
                res.stop_at.data_ptr(), res.gflags.data_ptr(), res.stats.data_ptr(),
                res.workspace.data_ptr(), res.workspace.numel() * 8, sp)
        return lambda: _lib.check(fn(*args), "qb_dev_follower_step")
    call_hb, call_st = caller(hb, res_hb), caller(storm, res_st)

    def restore(ee):
        for k, v in pristine.items():
            t[k].copy_(v)
        state.role.fill_(qt.ROLE_PROMOTABLE)
        state.election_elapsed.fill_(ee)
        state.heartbeat_elapsed.zero_()

    def timed(call, prepare, n):
        ev = HipEvents(2)
        ts = []
        for k in range(n):
            prepare(k)
            torch.cuda.synchronize()
            ev.record(ev.ev[0], sp)
            call()
            ev.record(ev.ev[1], sp)
            torch.cuda.synchronize()
            ts.append(ev.elapsed_ms(0, 1) / 1e3)
        ev.close()
        return ts

    def prep_hb(k):
        if k % 4000 == 0:   # Commit stays inside lastIndex = base + 4096
            restore(1)
            hb.index.copy_(base[hg])
        hb.index.add_(1)
        state.election_elapsed.fill_(1)
    timed(call_hb, prep_hb, 5)              # warm-up
    res_hb.stats.zero_()
    restore(1)
    hb.index.copy_(base[hg])
    t_hb = float(np.median(timed(call_hb, lambda k: prep_hb(k + 1), reps)))
    st = res_hb.stats_dict()
    assert st["heartbeats"] == reps * G and sum(st.values()) == reps * G, st
    timed(call_st, lambda k: restore(ET), 5)
    res_st.stats.zero_()
    t_st = float(np.median(timed(call_st, lambda k: restore(ET), reps)))
    st = res_st.stats_dict()
    assert st["granted"] == 2 * reps * G and st["became_follower"] == reps * G, st
    # algorithmic bytes.  Heartbeat, per record: group 4, flags 1, from 8, term
    # 8, Commit 8 in, resp_type 1 + resp_term 8 out = 38; per group: term 8,
    # lead 8, committed 8 in + 8 out, last_index 8, role 1, electionElapsed 4
    # in + 4 out, gflags 1, stop_at 4 = 54.  Storm, per record: the heartbeat's
    # 29 in + LogTerm 8, 9 out = 46, two per group; per group: term, vote and
    # lead 8 in + 8 out each, last_index 8, last_term 8, role 1,
    # electionElapsed 4 + 4, heartbeatElapsed 4 out, gflags 1, stop_at 4 = 82.
    hb_b, st_b = 38 + 54, 2 * 46 + 82
    extra = {"unit": "groups/s", "samples": reps, "records_per_group": 1,
             "heartbeat_us": t_hb * 1e6, "heartbeat_bytes_per_group": hb_b,
             "heartbeat_frac": G * hb_b / t_hb / 1e9 / HBM_PEAK_GBS,
             "storm_us": t_st * 1e6, "storm_bytes_per_group": st_b, "storm_records": 2 * G,
             "storm_frac": G * st_b / t_st / 1e9 / HBM_PEAK_GBS,
             "election_tick": ET, "check_quorum": 1, "pre_vote": 1,
             "timing": "one HIP event pair per call, median over the samples; state and "
                       "counters restored outside the timed call"}

    # parity at this size over every 1024th group
    def parity(ib, call, res, ee, what):
        restore(ee)
        if ib is hb:
            hb.index.copy_(base[hg] + 1)
        res.stats.zero_()
        torch.cuda.synchronize()
        grp = _to_np(ib.group, np.uint32, ib.M)
        sel = np.flatnonzero(grp % 1024 == 5)
        sub = np.unique(grp[sel])
        before = {k: _to_np(v, np.uint64, G)[sub].copy() for k, v in t.items()}
        sb = {k: v[sub].copy() for k, v in state.numpy(G).items()}
        cols = {k: _to_np(getattr(ib, k), dt, ib.M)[sel] for k, dt in (
            ("flags", np.uint8), ("frm", np.uint64), ("term", np.uint64), ("index", np.uint64),
            ("aux", np.uint64))}
        call()
        torch.cuda.synchronize()
        nodes = [F.Node(*(int(before[k][j]) for k in ("term", "vote", "lead", "committed",
                                                       "last_index", "last_term")),
                        int(sb["role"][j]), int(sb["election_elapsed"][j]),
                        int(sb["heartbeat_elapsed"][j])) for j in range(len(sub))]
        where = {int(gg): j for j, gg in enumerate(sub)}
        recs = [(where[int(grp[i])], F.Rec(int(cols["flags"][k]) & 7, int(cols["frm"][k]),
                                           int(cols["term"][k]), int(cols["index"][k]),
                                           int(cols["aux"][k]), bool(cols["flags"][k] & 0x80)))
                for k, i in enumerate(sel)]
        rt, rterm, stop, gf, _ = F.step_batch(nodes, recs, F.Config(ET, True, True))
        stop = [int(sel[s]) if s != F.NO_STOP else s for s in stop]
        after = fg.numpy()
        ok = all(np.array_equal(after[k][sub], np.array([getattr(n, k) for n in nodes],
                                                        after[k].dtype)) for k in after)
        ok = (ok and np.array_equal(_to_np(res.resp_type, np.uint8, ib.M)[sel], np.array(rt, np.uint8))
              and np.array_equal(_to_np(res.resp_term, np.uint64, ib.M)[sel],
                                 np.array(rterm, np.uint64))
              and np.array_equal(_to_np(res.stop_at, np.uint32, G)[sub], np.array(stop, np.uint32))
              and np.array_equal(_to_np(res.gflags, np.uint8, G)[sub], np.array(gf, np.uint8)))
        extra[f"parity_{what}"] = bool(ok)
        return ok, len(sub), len(sel)
    ok_h, ng, nr_h = parity(hb, call_hb, res_hb, 1, "heartbeat")
    ok_s, _, nr_s = parity(storm, call_st, res_st, ET, "storm")
    extra["parity"] = bool(ok_h and ok_s)
    extra["parity_check"] = (f"tests/follower_ref.py over the records of {ng} groups (every 1024th) "
                             f"of the {G}: {nr_h} heartbeat / {nr_s} storm records; state, "
                             "resp_type, resp_term, stop_at and gflags")
    reporter("follower step (heartbeats; pre-vote + vote storm)", G, t_hb, G * hb_b, extra)
    assert ok_h and ok_s, "follower parity failed"


def follower_log_config(G, reps, *, reporter=None):
    """The batched follower log step (qb_dev_follower_log_step): G follower
    groups (term 7, leader 1 known, CheckQuorum and PreVote on, ElectionTick
    10), each log [last - 100, last] of term 7 (one term run), committed 50
    below its end.  (a) steady replication: M = G same-term MsgApp in shuffled
    arrival order, each at Index = last_index with one run of 64 entries of
    term 7 and Commit 32 past the old end: every group appends, commits and
    answers, and no record reads or writes the run table.  (b) the same plus
    one heartbeat per group behind its MsgApp (Commit 48 past the old end: in
    range only with the new lastIndex), M = 2 G.  The state is restored
    between samples, outside the timed call.  Parity at this size:
    tests/append_ref.py over the records of every 1024th group (4096 groups;
    exact, because groups are independent) — their state, log, responses,
    app_from, gflags and stop_at after one call of each sample."""
    reporter = reporter or report
    import ctypes as C
    from etcd_amd import _lib
    from etcd_amd.quorum import follower as qf, tick as qt
    from etcd_amd.quorum.leader import _to_np
    from tests import append_ref as A, follower_ref as F
    ET, TERM, ENTS = 10, 7, 64
    i64 = lambda v: torch.full((G,), v, dtype=torch.int64, device=dev)  # noqa: E731
    g = torch.arange(G, dtype=torch.int64, device=dev)
    last = 5096 + (g * 37) % 1000
    t = {"term": i64(TERM), "vote": i64(1), "lead": i64(1), "committed": last - 50,
         "last_index": last.clone(), "last_term": i64(TERM)}
    state = qt.TickState(torch.full((G,), qt.ROLE_PROMOTABLE, dtype=torch.uint8, device=dev),
                         torch.ones(G, dtype=torch.int32, device=dev),
                         torch.zeros(G, dtype=torch.int32, device=dev),
                         torch.full((G,), 15, dtype=torch.int32, device=dev))
    fg = qf.FollowerGroups(G, ET, True, True, t, state)
    run_start = torch.zeros(qf.MAX_RUNS * G, dtype=torch.int64, device=dev)
    run_term = torch.zeros(qf.MAX_RUNS * G, dtype=torch.int64, device=dev)
    run_start[:G] = last - 100
    run_term[:G] = TERM
    lg = qf.FollowerLog(G, torch.full((G,), 1 << 16, dtype=torch.int32, device=dev), last - 99,
                        run_start, run_term)
    lg.validate(fg)
    pristine = {k: v.clone() for k, v in t.items()}
    pristine_log = (lg.meta.clone(), run_start.clone(), run_term.clone())

    def sample(per_group):
        """per_group records per group in shuffled arrival order; the group's
        first is its MsgApp, the second (if any) its heartbeat."""
        M = per_group * G
        sg = torch.randperm(M, device=dev) % G
        order = torch.argsort(sg, stable=True)
        rank = torch.empty_like(order)
        rank[order] = torch.arange(M, device=dev) % per_group
        is_app = rank == 0
        ib = qf.FollowerInbox(sg.to(torch.int32),
                              torch.where(is_app, qf.FIN_APP, qf.FIN_HEARTBEAT).to(torch.uint8),
                              torch.ones_like(sg), torch.full_like(sg, TERM),
                              torch.where(is_app, last[sg], last[sg] + 48),
                              torch.where(is_app, TERM, 0))
        ib._m = M
        off = torch.zeros(M + 1, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(is_app.to(torch.int64), 0)
        app = qf.FollowerAppInbox(torch.where(is_app, last[sg] + 32, 0), off.to(torch.int32),
                                  i64(TERM), torch.full((G,), ENTS, dtype=torch.int32, device=dev), G)
        return ib, app
    sp = torch.cuda.current_stream(dev).cuda_stream
    fgc = qf.FollowerGroupsC(G=G, election_timeout=ET, check_quorum=1, pre_vote=1, reserved=0,
                             role=state.role.data_ptr(),
                             election_elapsed=state.election_elapsed.data_ptr(),
                             heartbeat_elapsed=state.heartbeat_elapsed.data_ptr(),
                             **{k: v.data_ptr() for k, v in t.items()})
    lgc = qf.FollowerLogC(meta=lg.meta.data_ptr(), first_index=lg.first_index.data_ptr(),
                          last_index=t["last_index"].data_ptr(), last_term=t["last_term"].data_ptr(),
                          run_start=run_start.data_ptr(), run_term=run_term.data_ptr())
    fn = _lib.fn("qb_dev_follower_log_step")

    def restore():
        for k, v in pristine.items():
            t[k].copy_(v)
        lg.meta.copy_(pristine_log[0])
        run_start.copy_(pristine_log[1])
        run_term.copy_(pristine_log[2])
        state.role.fill_(qt.ROLE_PROMOTABLE)
        state.election_elapsed.fill_(1)
        state.heartbeat_elapsed.zero_()

    def caller(ib, app, res):
        ibc = qf.FollowerInboxC(M=ib.M, group=ib.group.data_ptr(), flags=ib.flags.data_ptr(),
                                term=ib.term.data_ptr(), index=ib.index.data_ptr(),
                                aux=ib.aux.data_ptr())
        setattr(ibc, "from", ib.frm.data_ptr())
        apc = qf.FollowerAppInboxC(commit=app.commit.data_ptr(), ent_off=app.ent_off.data_ptr(),
                                   ent_term=app.ent_term.data_ptr(), ent_len=app.ent_len.data_ptr(),
                                   E=app.E)
        aoc = qf.FollowerAppOutC(resp_index=res.resp_index.data_ptr(),
                                 resp_hint=res.resp_hint.data_ptr(),
                                 resp_log_term=res.resp_log_term.data_ptr(),
                                 app_from=res.app_from.data_ptr())
        args = (C.byref(fgc), C.byref(lgc), C.byref(ibc), C.byref(apc), res.resp_type.data_ptr(),
                res.resp_term.data_ptr(), C.byref(aoc), res.stop_at.data_ptr(),
                res.gflags.data_ptr(), res.stats.data_ptr(), res.workspace.data_ptr(),
                res.workspace.numel() * 8, sp)
        keep = (ibc, apc, aoc)
        return lambda: (keep, _lib.check(fn(*args), "qb_dev_follower_log_step"))

    def timed(call, n):
        ev = HipEvents(2)
        ts = []
        for _ in range(n):
            restore()
            torch.cuda.synchronize()
            ev.record(ev.ev[0], sp)
            call()
            ev.record(ev.ev[1], sp)
            torch.cuda.synchronize()
            ts.append(ev.elapsed_ms(0, 1) / 1e3)
        ev.close()
        return ts

    def parity(ib, app, call, res):
        restore()
        res.stats.zero_()
        torch.cuda.synchronize()
        grp = _to_np(ib.group, np.uint32, ib.M)
        sel = np.flatnonzero(grp % 1024 == 5)
        sub = np.unique(grp[sel])
        before = {k: _to_np(v, np.uint64, G)[sub].copy() for k, v in t.items()}
        sb = {k: v[sub].copy() for k, v in state.numpy(G).items()}
        first = _to_np(lg.first_index, np.uint64, G)[sub]
        cols = {k: _to_np(getattr(ib, k), dt, ib.M)[sel] for k, dt in (
            ("flags", np.uint8), ("frm", np.uint64), ("term", np.uint64), ("index", np.uint64),
            ("aux", np.uint64))}
        commit = _to_np(app.commit, np.uint64, ib.M)[sel]
        call()
        torch.cuda.synchronize()
        nodes = []
        for j in range(len(sub)):
            n = A.new_node([TERM] * (int(before["last_index"][j]) - int(first[j]) + 2), int(first[j]),
                           term=int(before["term"][j]), vote=int(before["vote"][j]),
                           lead=int(before["lead"][j]), committed=int(before["committed"][j]),
                           role=int(sb["role"][j]), election_elapsed=int(sb["election_elapsed"][j]),
                           heartbeat_elapsed=int(sb["heartbeat_elapsed"][j]))
            assert n.last_index == int(before["last_index"][j])
            nodes.append(n)
        where = {int(gg): j for j, gg in enumerate(sub)}
        recs = []
        for k, i in enumerate(sel):
            kind = int(cols["flags"][k]) & 7
            a = (kind, int(cols["frm"][k]), int(cols["term"][k]), int(cols["index"][k]),
                 int(cols["aux"][k]), False)
            recs.append((where[int(grp[i])],
                         A.AppRec(*a, int(commit[k]), [TERM] * ENTS) if kind == A.APP else F.Rec(*a)))
        o = A.step_batch(nodes, recs, F.Config(ET, True, True))
        stop = [int(sel[s]) if s != F.NO_STOP else s for s in o["stop_at"]]
        after = fg.numpy()
        ok = all(np.array_equal(after[k][sub], np.array([getattr(n, k) for n in nodes],
                                                        after[k].dtype)) for k in after)
        la = lg.numpy()
        ok = ok and all(A.runs_of(n.terms, n.first_index) ==
                        ([int(la["run_start"][0, gg])], [int(la["run_term"][0, gg])])
                        and int(la["meta"][gg]) == 1 << 16 for n, gg in zip(nodes, sub))
        for k, dt in (("resp_type", np.uint8), ("resp_term", np.uint64), ("resp_index", np.uint64),
                      ("app_from", np.uint64)):
            ok = ok and np.array_equal(_to_np(getattr(res, k), dt, ib.M)[sel], np.array(o[k], dt))
        ok = (ok and np.array_equal(_to_np(res.stop_at, np.uint32, G)[sub], np.array(stop, np.uint32))
              and np.array_equal(_to_np(res.gflags, np.uint8, G)[sub], np.array(o["gflags"], np.uint8)))
        return bool(ok), len(sub), len(sel)

    out = {}
    for what, per_group in (("app", 1), ("app_hb", 2)):
        ib, app = sample(per_group)
        restore()
        res = qf.follower_log_step(fg, lg, ib, app)   # (the mirror's argument checks, once)
        call = caller(ib, app, res)
        timed(call, 5)                                # warm-up
        res.stats.zero_()
        tm = float(np.median(timed(call, reps)))
        st = res.stats_dict()
        assert st["app_accepted"] == reps * G and st["entries_appended"] == reps * G * ENTS, st
        assert st["heartbeats"] == (per_group - 1) * reps * G and st["after_stop"] == 0, st
        out[what] = (tm,) + parity(ib, app, call, res)
    # arithmetic bytes (not counters).  MsgApp, per record: group 4, flags 1,
    # from 8, term 8, Index 8, LogTerm 8, Commit 8, ent_off 2 x 4, the run's
    # term 8 and length 4 in; resp_type 1, resp_term 8, resp_index 8, app_from
    # 8 out = 98.  Per group: term 8, vote 8, lead 8, last_term 8, role 1 in;
    # committed and last_index 8 in + 8 out each, electionElapsed 4 + 4,
    # gflags 1, stop_at 4 = 78.  The heartbeat behind it, per record: 4 + 1 +
    # 8 + 8 + 8 + 8 in, Commit 8 and ent_off 8 read with every record, the four
    # response columns 25 out = 78.
    a_b, b_b = 98 + 78, 98 + 78 + 78
    (t_a, ok_a, ng, nr_a), (t_b, ok_b, _, nr_b) = out["app"], out["app_hb"]
    extra = {"unit": "groups/s", "samples": reps, "entries_per_app": ENTS,
             "app_us": t_a * 1e6, "app_bytes_per_group": a_b,
             "app_tbs": G * a_b / t_a / 1e12, "app_frac": G * a_b / t_a / 1e9 / HBM_PEAK_GBS,
             "app_hb_us": t_b * 1e6, "app_hb_bytes_per_group": b_b, "app_hb_records": 2 * G,
             "app_hb_tbs": G * b_b / t_b / 1e12,
             "app_hb_frac": G * b_b / t_b / 1e9 / HBM_PEAK_GBS,
             "bytes": "arithmetic (the columns a record and a group touch), not counters; the "
                      "grouping passes' workspace traffic is not counted",
             "election_tick": ET, "check_quorum": 1, "pre_vote": 1,
             "parity_app": ok_a, "parity_app_hb": ok_b, "parity": bool(ok_a and ok_b),
             "parity_check": (f"tests/append_ref.py over the records of {ng} groups (every 1024th) "
                              f"of the {G}: {nr_a} / {nr_b} records; state, run table, meta, "
                              "resp_type, resp_term, resp_index, app_from, stop_at and gflags"),
             "timing": "one HIP event pair per call, median over the samples; state and log "
                       "restored outside the timed call"}
    reporter("follower log step (steady MsgApp; MsgApp + heartbeat)", G, t_a, G * a_b, extra)
    assert ok_a and ok_b, "follower-log parity failed"


def campaign_config(G, reps, *, reporter=None):
    """The batched campaign (qb_dev_campaign): G five-voter groups of the
    synth_streaming table held by a follower (own slot 0), PreVote on.
    Sample (a): every group gets QB_CAMP_HUP — becomePreCandidate, own vote,
    four MsgPreVote: group words only, no slot phase.  Sample (b): every
    group is a candidate and gets QB_CAMP_WON — becomeLeader + bcastAppend:
    reset rewrites all five slots.  One HIP event pair per call, median over
    the samples after warm-up; role, lead and votes are restored between
    samples outside the timed call.  Parity: one more call at the same size
    with seeded roles, promotable bits, terms and actions, every 1024th
    group against tests/campaign_ref.py."""
    reporter = reporter or report
    import ctypes as C
    import importlib
    import time
    from etcd_amd import _lib
    from etcd_amd.quorum import tick as qt
    from etcd_amd.quorum.leader import _to_np, synth_streaming
    from tests import campaign_pack as P, campaign_ref as R
    qc = importlib.import_module("etcd_amd.quorum.campaign")
    n = 5
    lg, _ = synth_streaming(G, W=1, D=1, n=n, device=dev)
    S = lg.S
    z32 = lambda: torch.zeros(G, dtype=torch.int32, device=dev)  # noqa: E731
    state = qt.TickState(torch.full((G,), qt.ROLE_FOLLOWER | qt.ROLE_PROMOTABLE, dtype=torch.uint8,
                                    device=dev), z32(), z32(),
                         torch.full((G,), 15, dtype=torch.int32, device=dev))
    lg.t["meta"].fill_(0xFF00 | (1 << 16))  # own slot 0, no transferee, one term run
    es = qc.ElectionState.for_table(lg, state, np.arange(1, G + 1, dtype=np.uint64),
                                    np.zeros(G, np.uint64), np.zeros(G, np.uint64),
                                    np.full(G, 7, np.uint64), 10, True, True)
    action = torch.zeros(G, dtype=torch.uint8, device=dev)
    out = lg.campaign(es, action)   # (the mirror's argument checks, once; all QB_CAMP_NONE)
    sp = torch.cuda.current_stream(dev).cuda_stream
    ft = es.follower.t
    cg = qc.CampaignGroupsC(
        G=G, pre_vote=1, reserved=0, self_id=es.self_id.data_ptr(), votes=es.votes.data_ptr(),
        role=state.role.data_ptr(), election_elapsed=state.election_elapsed.data_ptr(),
        heartbeat_elapsed=state.heartbeat_elapsed.data_ptr(),
        **{k: lg.t[k].data_ptr() for k in ("off", "cfg", "meta", "match", "next",
                                           "pending_snapshot", "pstate", "infl_pos")},
        **{k: ft[k].data_ptr() for k in ("term", "vote", "lead", "committed", "last_index",
                                         "last_term")})
    fn = _lib.fn("qb_dev_campaign")
    args = (C.byref(cg), action.data_ptr(), out.cflags.data_ptr(), out.req_type.data_ptr(),
            out.req_term.data_ptr(), out.req_mask.data_ptr(), out.stats.data_ptr(), sp)

    def call():
        _lib.check(fn(*args), "qb_dev_campaign")
    term0 = ft["term"].clone()

    def timed(role, act):
        def restore():
            state.role.fill_(role | qt.ROLE_PROMOTABLE)
            ft["lead"].zero_()
            ft["vote"].zero_()
            ft["term"].copy_(term0)
            es.votes.zero_()
            action.fill_(act)

        def sample(ev):
            restore()
            torch.cuda.synchronize()
            ev.record(ev.ev[0], sp)
            call()
            ev.record(ev.ev[1], sp)
            torch.cuda.synchronize()
            return ev.elapsed_ms(0, 1) / 1e3
        ev = HipEvents(2)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.3:  # warm-up: clocks settle (time_region)
            sample(ev)
        out.stats.zero_()
        per = [sample(ev) for _ in range(reps)]
        ev.close()
        return float(np.median(per)), out.stats_dict()
    t_hup, st = timed(qt.ROLE_FOLLOWER, qc.CAMP_HUP)
    assert st["pre_campaigns"] == reps * G and st["vote_requests"] == reps * G * (n - 1), st
    assert st["campaigns"] == 0 and st["became_leader"] == 0, st
    t_won, st = timed(qt.ROLE_CANDIDATE, qc.CAMP_WON)
    assert st["became_leader"] == reps * G and st["vote_requests"] == 0, st
    # per group, read by every acting group: action 1, role 1, meta 4, cfg 4,
    # off 4, term / vote / committed / self_id / last_index 40 = 54 B.
    # (a) writes votes 4, role 1, lead 8, cflags 1, req_type 1, req_term 8,
    # req_mask 2 = 25 B; (b) writes both counters 8, votes 4, role 1, lead 8,
    # cflags 1, req_type 1 = 23 B (meta, term, vote and committed do not
    # change here) and per slot match 8, next 8, pending_snapshot 8, pstate 1,
    # infl_pos 4 = 29 B
    hup_b = 54 + 25
    won_b = 54 + 23 + n * 29
    extra = {"unit": "groups/s", "samples": reps, "pre_vote": 1,
             "hup_us": t_hup * 1e6, "hup_bytes_per_group": hup_b,
             "hup_TBs": G * hup_b / t_hup / 1e12,
             "hup_frac": G * hup_b / t_hup / 1e9 / HBM_PEAK_GBS,
             "won_us": t_won * 1e6, "won_bytes_per_group": won_b,
             "won_TBs": G * won_b / t_won / 1e12,
             "won_frac": G * won_b / t_won / 1e9 / HBM_PEAK_GBS,
             "timing": "one HIP event pair per call, median over the samples; per_launch_us = "
                       "sample (b), every group WON as candidate (reset + bcastAppend)"}
    # parity at this size
    gen = torch.Generator(device=dev).manual_seed(0xCA3F)
    rnd = lambda hi, k: torch.randint(0, hi, (k,), generator=gen, device=dev)  # noqa: E731
    state.role.copy_((rnd(4, G) | (torch.where(rnd(8, G) == 0, 0, 1) << 7)).to(torch.uint8))
    ft["term"].copy_(term0 + rnd(3, G))
    ft["vote"].copy_(rnd(3, G))
    ft["lead"].copy_(rnd(3, G))
    es.votes.copy_((rnd(32, G) * 0x10001).to(torch.int32))
    state.election_elapsed.copy_(rnd(20, G).to(torch.int32))
    state.heartbeat_elapsed.copy_(rnd(3, G).to(torch.int32))
    lg.t["meta"].copy_((lg.t["meta"] & ~0xFFFF | rnd(n + 1, G)
                        | torch.where(rnd(4, G) == 0, rnd(n, G), torch.full((G,), 0xFF, device=dev))
                        << 8).to(torch.int32))
    action.copy_((rnd(5, G) | (torch.where(rnd(4, G) == 0, 1, 0) << 7)).to(torch.uint8))
    sub = np.arange(0, G, 1024)
    slots = (sub[:, None] * n + np.arange(n)[None, :]).ravel()

    def gather():
        a = {k: _to_np(lg.t[k], dt)[sub].copy() for k, dt in (
            ("cfg", np.uint32), ("meta", np.uint32), ("term", np.uint64), ("committed", np.uint64),
            ("last_index", np.uint64))}
        a.update({k: _to_np(lg.t[k], dt)[slots].copy() for k, dt in (
            ("match", np.uint64), ("next", np.uint64), ("pending_snapshot", np.uint64),
            ("pstate", np.uint8), ("infl_pos", np.uint32), ("infl_buf", np.uint64))})
        a["off"] = np.arange(len(sub) + 1, dtype=np.uint32) * n
        a.update({k: np.zeros(0, dt) for k, dt in (("rq_ctx", np.uint64), ("rq_index", np.uint64),
                                                   ("rq_meta", np.uint32))})
        e = {k: v[sub].copy() for k, v in es.numpy().items()}
        return a, e
    a0, e0 = gather()
    nodes = [P.make_node(n, int(a0["cfg"][i]) & 0xFFFF, int(a0["cfg"][i]) >> 16,
                         int(a0["meta"][i]) & 0xFF, self_id=int(e0["self_id"][i]),
                         last_index=int(a0["last_index"][i]), last_term=int(e0["last_term"][i]))
             for i in range(len(sub))]
    P.unpack_into(nodes, a0, e0, 0, 1)   # (this table's rings hold one entry)
    fill = P.FILL - (1 << 64)
    out.req_term.fill_(fill)
    out.req_mask.fill_(0xA5A5 - (1 << 16))
    out.stats.zero_()
    act_h = action.cpu().numpy()
    call()
    torch.cuda.synchronize()
    rterm, rmask = np.full(len(sub), P.FILL, np.uint64), np.full(len(sub), 0xA5A5, np.uint16)
    cf, rt, _ = P.ref_campaign(nodes, act_h[sub], True, rterm, rmask)
    want_a, want_e = P.pack_nodes(nodes, 0, 1)
    a1, e1 = gather()
    keys = ("meta", "term", "committed", "match", "next", "pending_snapshot", "pstate", "infl_pos",
            "infl_buf")
    ok = (all(np.array_equal(a1[k], want_a[k]) for k in keys)
          and all(np.array_equal(e1[k], want_e[k]) for k in want_e)
          and np.array_equal(out.cflags.cpu().numpy()[sub], cf)
          and np.array_equal(out.req_type.cpu().numpy()[sub], rt)
          and np.array_equal(_to_np(out.req_term, np.uint64, G)[sub], rterm)
          and np.array_equal(_to_np(out.req_mask, np.uint16, G)[sub], rmask))
    st = out.stats_dict()
    ok = ok and sum(st[k] for k in ("pre_campaigns", "became_leader", "became_follower",
                                    "ignored_leader", "ignored_pending_conf", "ignored_role")) > 0
    extra["parity"] = bool(ok)
    extra["parity_check"] = (f"tests/campaign_ref.py over {len(sub)} groups (every 1024th) of the "
                             f"{G} with seeded roles, own slots, terms, votes and actions: state, "
                             f"Progress, cflags and req_* (untouched elements included); the "
                             f"call's stats: {st}")
    reporter("campaign (MsgHup pre-campaign; WON: becomeLeader + bcastAppend)", G, t_won,
             G * won_b, extra)
    assert ok, "campaign parity failed"


def propose_config(G, reps, *, reporter=None):
    """The batched proposal (qb_dev_leader_propose): G five-voter leader groups
    of the synth_streaming table (own slot 0, the leader's term on top of the
    log, rings of 4, 64 entries per MsgApp).  Sample (a): the steady proposal —
    64 entries per group, every peer replicating with an empty ring at
    next = last + 1: four MsgApp of 64 entries, OptimisticUpdate and
    Inflights.Add per peer, no run table touched.  Sample (b): every peer
    probing and unpaused: four MsgApp, ProbeSent set.  One HIP event pair per
    call, median over the samples after warm-up; last_index, the own match,
    next, pstate, infl_pos and uncommitted_size are restored between samples
    outside the timed call.  Parity: one more call at the same size with seeded
    roles, actions, entry counts, conf changes, sizes and peer Progress, every
    1024th group against tests/propose_ref.py."""
    reporter = reporter or report
    import ctypes as C
    import importlib
    import time
    from etcd_amd import _lib
    from etcd_amd.quorum import propose as qp, tick as qt
    from etcd_amd.quorum.leader import MAX_RUNS, _to_np, synth_streaming
    from tests import propose_pack as P, propose_ref as R
    qc = importlib.import_module("etcd_amd.quorum.campaign")
    n, W, D, NE = 5, 4, 64, 64
    lg, _ = synth_streaming(G, W=W, D=D, n=n, device=dev)
    S = lg.S
    z32 = lambda: torch.zeros(G, dtype=torch.int32, device=dev)  # noqa: E731
    z64 = lambda: torch.zeros(G, dtype=torch.int64, device=dev)  # noqa: E731
    state = qt.TickState(torch.full((G,), qt.ROLE_LEADER | qt.ROLE_PROMOTABLE, dtype=torch.uint8,
                                    device=dev), z32(), z32(), z32())
    lg.t["meta"].fill_(0xFF00 | (1 << 16))  # own slot 0, no transferee, one term run
    es = qc.ElectionState.for_table(lg, state, np.arange(1, G + 1, dtype=np.uint64),
                                    np.zeros(G, np.uint64), np.arange(1, G + 1, dtype=np.uint64),
                                    np.full(G, 7, np.uint64), 10, True, True)
    ps = qp.ProposeState(z64(), z64(), z64())
    own = torch.arange(S, device=dev) % n == 0
    lg.t["match"] = torch.where(own, lg.t["next"] - 1, lg.t["match"])
    lg.t["infl_pos"].zero_()
    ib = qp.ProposeInbox(torch.zeros(G, dtype=torch.uint8, device=dev),
                         torch.full((G,), NE, dtype=torch.int32, device=dev),
                         torch.full((G,), 8 * NE, dtype=torch.int64, device=dev), z32(), z64())
    LIMIT = 1 << 30
    out = qp.leader_propose(lg, es, ps, ib, max_uncommitted_size=LIMIT)  # (the mirror's checks, once)
    sp = torch.cuda.current_stream(dev).cuda_stream
    ft = es.follower.t
    ptr = {k: lg.t[k].data_ptr() for k in ("off", "cfg", "first_index", "snap_index", "snap_term",
                                           "max_ents", "meta", "run_start", "run_term", "match",
                                           "next", "pending_snapshot", "pstate", "infl_pos",
                                           "infl_buf")}
    ptr.update({k: ft[k].data_ptr() for k in ("term", "lead", "committed", "last_index",
                                              "last_term")})
    pg = qp.ProposeGroupsC(G=G, inflight_cap=W, disable_proposal_forwarding=0,
                           max_uncommitted_size=LIMIT, role=state.role.data_ptr(),
                           applied=ps.applied.data_ptr(),
                           uncommitted_size=ps.uncommitted_size.data_ptr(),
                           pending_conf_index=ps.pending_conf_index.data_ptr(), **ptr)
    pin = qp.ProposeInC(action=ib.action.data_ptr(), n_ents=ib.n_ents.data_ptr(),
                        payload=ib.payload.data_ptr(), cc_at=ib.cc_at.data_ptr(),
                        cc_payload=ib.cc_payload.data_ptr())
    pout = qp.ProposeOutC(pflags=out.pflags.data_ptr(), msg_type=out.msg_type.data_ptr(),
                          msg_index=out.msg_index.data_ptr(),
                          msg_log_term=out.msg_log_term.data_ptr(), msg_n=out.msg_n.data_ptr())
    fn = _lib.fn("qb_dev_leader_propose")
    args = (C.byref(pg), C.byref(pin), C.byref(pout), out.stats.data_ptr(), sp)

    def call():
        _lib.check(fn(*args), "qb_dev_leader_propose")
    keep = {k: lg.t[k].clone() for k in ("match", "next", "last_index")}
    PR_REPL, PR_PROBE = 1 | 8, 0 | 8   # RecentActive set

    def timed(peer_state):
        pstate0 = torch.where(own, torch.full_like(lg.t["pstate"], PR_REPL),
                              torch.full_like(lg.t["pstate"], peer_state))

        def restore():
            for k, v in keep.items():
                lg.t[k].copy_(v)
            lg.t["pstate"].copy_(pstate0)
            lg.t["infl_pos"].zero_()
            ps.uncommitted_size.zero_()
            ib.action.fill_(qp.PROP_ENTRIES)

        def sample(ev):
            restore()
            torch.cuda.synchronize()
            ev.record(ev.ev[0], sp)
            call()
            ev.record(ev.ev[1], sp)
            torch.cuda.synchronize()
            return ev.elapsed_ms(0, 1) / 1e3
        ev = HipEvents(2)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.3:  # warm-up: clocks settle (time_region)
            sample(ev)
        out.stats.zero_()
        per = [sample(ev) for _ in range(reps)]
        ev.close()
        return float(np.median(per)), out.stats_dict()
    t_repl, st = timed(PR_REPL)
    assert st["proposals"] == reps * G and st["entries"] == reps * G * NE, st
    assert st["msg_app"] == reps * G * (n - 1) and st["commits"] == 0 and st["drop_size"] == 0, st
    assert bool((lg.t["infl_pos"].view(G, n)[:, 1:] == 1 << 16).all())   # one MsgApp in every ring
    t_probe, st = timed(PR_PROBE)
    assert st["proposals"] == reps * G and st["msg_app"] == reps * G * (n - 1), st
    assert bool((lg.t["pstate"].view(G, n)[:, 1:] == (PR_PROBE | 4)).all())  # ProbeSent
    # per group, read by every proposing group: action 1, role 1, meta 4, cfg 4,
    # off 4, term / last_index / last_term / committed 32, n_ents 4, payload 8,
    # uncommitted_size 8, max_ents 8, first_index 8 = 82 B; written: last_index 8,
    # uncommitted_size 8, pflags 1 = 17 B.  Every slot's match is read for
    # maybeCommit (8 B); the own slot: next 8 read and written, pstate 1 read,
    # match 8 written, msg_type 1 = 26 B.  A peer, read: next 8, pstate 1,
    # infl_pos 4; written: msg_type 1, msg_index / msg_log_term / msg_n 24, and
    # (a) next 8, infl_pos 4, infl_buf 8 = 58 B, (b) pstate 1 = 39 B.
    repl_b = 82 + 17 + n * 8 + 26 + (n - 1) * 58
    probe_b = 82 + 17 + n * 8 + 26 + (n - 1) * 39
    extra = {"unit": "groups/s", "samples": reps, "entries_per_proposal": NE, "inflight_cap": W,
             "replicate_us": t_repl * 1e6, "replicate_bytes_per_group": repl_b,
             "replicate_TBs": G * repl_b / t_repl / 1e12,
             "replicate_frac": G * repl_b / t_repl / 1e9 / HBM_PEAK_GBS,
             "probe_us": t_probe * 1e6, "probe_bytes_per_group": probe_b,
             "probe_TBs": G * probe_b / t_probe / 1e12,
             "probe_frac": G * probe_b / t_probe / 1e9 / HBM_PEAK_GBS,
             "timing": "one HIP event pair per call, median over the samples; per_launch_us = "
                       "sample (a), every peer replicating"}
    # parity at this size
    for k, v in keep.items():
        lg.t[k].copy_(v)
    gen = torch.Generator(device=dev).manual_seed(0x9805E)
    rnd = lambda hi, k: torch.randint(0, hi, (k,), generator=gen, device=dev)  # noqa: E731
    state.role.copy_((torch.where(rnd(4, G) == 0, rnd(4, G), torch.full((G,), 2, device=dev))
                      | (1 << 7)).to(torch.uint8))
    ft["lead"].copy_(rnd(2, G) * 9)
    ft["term"].copy_(ft["term"] + torch.where(rnd(8, G) == 0, 1, 0))    # some need a new run
    lg.t["meta"].copy_((lg.t["meta"] & ~0xFFFF | rnd(n + 1, G)
                        | torch.where(rnd(16, G) == 0, rnd(n, G), torch.full((G,), 0xFF, device=dev))
                        << 8).to(torch.int32))
    gs = torch.arange(S, device=dev) // n
    last = keep["last_index"][gs]
    lg.t["next"].copy_(torch.where(own, keep["next"], last + 1 - rnd(200, S)))
    lg.t["match"].copy_(torch.where(own, keep["match"], last - 200 + rnd(201, S)))
    lg.t["pstate"].copy_(torch.where(own, torch.full((S,), PR_REPL, device=dev),
                                     rnd(3, S) | rnd(4, S) << 2).to(torch.uint8))
    lg.t["infl_pos"].copy_((rnd(W, S) | rnd(W + 1, S) << 16).to(torch.int32))
    ps.applied.copy_(rnd(4, G))
    ps.pending_conf_index.copy_(rnd(6, G))
    ps.uncommitted_size.copy_(torch.where(rnd(2, G) == 0, 0, LIMIT - rnd(1024, G)))
    ib.action.copy_((rnd(3, G) | torch.where(rnd(4, G) == 0, rnd(4, G) << 6, 0)).to(torch.uint8))
    ib.n_ents.copy_(rnd(65, G).to(torch.int32))
    ib.cc_at.copy_(rnd(70, G).to(torch.int32))
    ib.cc_payload.copy_(rnd(300, G))
    ib.payload.copy_(ib.cc_payload + rnd(700, G))
    sub = np.arange(0, G, 1024)
    slots = (sub[:, None] * n + np.arange(n)[None, :]).ravel()
    rows = (np.arange(MAX_RUNS)[:, None] * G + sub[None, :]).ravel()
    ring = (slots[:, None] * W + np.arange(W)[None, :]).ravel()

    def gather():
        a = {k: _to_np(lg.t[k], dt)[sub].copy() for k, dt in (
            ("cfg", np.uint32), ("meta", np.uint32), ("term", np.uint64), ("committed", np.uint64),
            ("first_index", np.uint64), ("last_index", np.uint64), ("snap_index", np.uint64),
            ("snap_term", np.uint64), ("max_ents", np.uint64))}
        a.update({k: _to_np(lg.t[k], np.uint64)[rows].copy() for k in ("run_start", "run_term")})
        a.update({k: _to_np(lg.t[k], dt)[slots].copy() for k, dt in (
            ("match", np.uint64), ("next", np.uint64), ("pending_snapshot", np.uint64),
            ("pstate", np.uint8), ("infl_pos", np.uint32))})
        a["infl_buf"] = _to_np(lg.t["infl_buf"], np.uint64)[ring].copy()
        a["off"] = np.arange(len(sub) + 1, dtype=np.uint32) * n
        a.update({k: np.zeros(0, dt) for k, dt in (("rq_ctx", np.uint64), ("rq_index", np.uint64),
                                                   ("rq_meta", np.uint32))})
        e = {k: v[sub].copy() for k, v in es.numpy().items()}
        p = {k: v[sub].copy() for k, v in ps.numpy(G).items()}
        return a, e, p
    a0, e0, p0 = gather()
    nodes = P.nodes_from_arrays(a0, e0, p0, W)
    inp = {k: _to_np(getattr(ib, k), dt, G)[sub].copy() for k, dt in (
        ("action", np.uint8), ("n_ents", np.uint32), ("payload", np.uint64), ("cc_at", np.uint32),
        ("cc_payload", np.uint64))}
    fill = P.FILL - (1 << 64)
    out.msg_type.fill_(P.FILL8)
    for t_ in (out.msg_index, out.msg_log_term, out.msg_n):
        t_.fill_(fill)
    out.stats.zero_()
    call()
    torch.cuda.synchronize()
    msg = P.new_msg(len(slots))
    pf, _, _ = P.ref_propose(nodes, inp, R.Config(max_uncommitted_size=LIMIT), a0["off"], msg)
    want_a, want_e, want_p = P.pack_nodes(nodes, W)
    a1, e1, p1 = gather()
    keys = ("meta", "committed", "last_index", "run_start", "run_term", "match", "next",
            "pending_snapshot", "pstate", "infl_pos", "infl_buf")
    ok = (all(np.array_equal(a1[k], want_a[k]) for k in keys)
          and all(np.array_equal(e1[k], want_e[k]) for k in want_e)
          and all(np.array_equal(p1[k], want_p[k]) for k in want_p)
          and np.array_equal(out.pflags.cpu().numpy()[sub], pf)
          and all(np.array_equal(_to_np(getattr(out, k), msg[k].dtype, S)[slots], msg[k])
                  for k in msg))
    st = out.stats_dict()
    ok = ok and all(st[k] > 0 for k in ("proposals", "leader_entries", "drop_size", "cc_accepted",
                                        "cc_refused", "msg_app", "commits", "forwarded"))
    extra["parity"] = bool(ok)
    extra["parity_check"] = (f"tests/propose_ref.py over {len(sub)} groups (every 1024th) of the "
                             f"{G} with seeded roles, own slots, terms, peer Progress, actions, "
                             f"entry counts, conf changes and sizes: state, Progress, rings, run "
                             f"tables, pflags and msg_* (untouched elements included); the call's "
                             f"stats: {st}")
    reporter("propose (64-entry MsgProp, appendEntry + bcastAppend; peers replicating)", G, t_repl,
             G * repl_b, extra)
    assert ok, "propose parity failed"


def switch_config_row(G, reps, *, reporter=None):
    """The batched switchToConfig (qb_dev_switch_config) at the propose row's
    G.  Dense: every group a five-voter leader (own slot 0, peers replicating
    at next = last + 1) that adds one voter whose ID ranks third, so three old
    slots move; no commit, the new member alone is probed (one MsgApp of one
    entry, ProbeSent).  Sparse: the same table with one group in a hundred
    acting.  One HIP event pair per call, median over the samples after
    warm-up; meta, the new member's pstate and the outputs are restored
    between samples outside the timed call.  Parity: the dense call's every
    1024th group against tests/switch_ref.py."""
    reporter = reporter or report
    import ctypes as C
    import importlib
    import time
    from etcd_amd import _lib
    from etcd_amd.quorum import confchange as qcc, switch as qs, tick as qt
    from etcd_amd.quorum.leader import MAX_RUNS, _to_np, synth_streaming
    from tests import switch_ref as R
    qc = importlib.import_module("etcd_amd.quorum.campaign")
    n0, n, W, D, NEW = 5, 6, 4, 64, 2
    lg, _ = synth_streaming(G, W=W, D=D, n=n, device=dev)
    S0, S = n0 * G, lg.S
    z32 = lambda: torch.zeros(G, dtype=torch.int32, device=dev)  # noqa: E731
    state = qt.TickState(torch.full((G,), qt.ROLE_LEADER | qt.ROLE_PROMOTABLE, dtype=torch.uint8,
                                    device=dev), z32(), z32(), z32())
    lg.t["meta"].fill_(0xFF00 | (1 << 16))  # own slot 0, no transferee, one term run
    g64 = torch.arange(G, dtype=torch.int64, device=dev)
    es = qc.ElectionState.for_table(lg, state, (np.arange(G, dtype=np.uint64) * 10 + 1),
                                    np.zeros(G, np.uint64), np.zeros(G, np.uint64),
                                    np.full(G, 7, np.uint64), 10, True, True)
    slot = torch.arange(S, device=dev) % n
    last = lg.t["last_index"][torch.arange(S, device=dev) // n]
    fresh = slot == NEW                                     # initProgress: Probe at Next = last
    lg.t["match"] = torch.where(fresh, 0, torch.where(slot == 0, last, lg.t["match"]))
    lg.t["next"] = torch.where(fresh, last, last + 1)
    lg.t["infl_pos"].zero_()
    pstate0 = torch.where(fresh, 0 | 8, 1 | 8).to(torch.uint8)
    lg.t["pstate"].copy_(pstate0)
    ids = (g64[:, None] * 10 + 1 + torch.arange(n, device=dev)[None, :]).reshape(-1)
    keep = torch.tensor([0, 1, 3, 4, 5], device=dev)
    old_ids = (g64[:, None] * 10 + 1 + keep[None, :]).reshape(-1)
    old = qcc.ConfigTable(G, S0, W, {"off": (torch.arange(G + 1, device=dev) * n0).to(torch.int32),
                                     "ids": old_ids})
    new = qcc.ConfigTable(G, S, W, dict(lg.t, ids=ids))
    action = torch.full((G,), qs.SW_SWITCH, dtype=torch.uint8, device=dev)
    sg, so, out = qs.switch_args(lg, es, old, new, action)   # (the mirror's checks, once)
    sp = torch.cuda.current_stream(dev).cuda_stream
    fn = _lib.fn("qb_dev_switch_config")
    args = (C.byref(sg), action.data_ptr(), C.byref(so), out.stats.data_ptr(), sp)
    meta0 = lg.t["meta"].clone()

    def timed():
        def sample(ev):
            lg.t["meta"].copy_(meta0)
            lg.t["pstate"].copy_(pstate0)
            torch.cuda.synchronize()
            ev.record(ev.ev[0], sp)
            _lib.check(fn(*args), "qb_dev_switch_config")
            ev.record(ev.ev[1], sp)
            torch.cuda.synchronize()
            return ev.elapsed_ms(0, 1) / 1e3
        ev = HipEvents(2)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.3:  # warm-up: clocks settle (time_region)
            sample(ev)
        out.stats.zero_()
        per = [sample(ev) for _ in range(reps)]
        ev.close()
        return float(np.median(per)), out.stats_dict()
    t_dense, st = timed()
    assert st["switched"] == reps * G and st["probed"] == reps * G and st["msg_app"] == reps * G, st
    assert st["commits"] == 0 and st["host"] == 0, st
    # parity of the dense call, every 1024th group
    sub = np.arange(0, G, 1024)
    slots = (sub[:, None] * n + np.arange(n)[None, :]).ravel()
    oslots = (sub[:, None] * n0 + np.arange(n0)[None, :]).ravel()
    rows = (np.arange(MAX_RUNS)[:, None] * G + sub[None, :]).ravel()
    ft = es.follower.t

    def gather():
        a = {k: _to_np(lg.t[k], dt)[sub].copy() for k, dt in (
            ("cfg", np.uint32), ("meta", np.uint32), ("first_index", np.uint64),
            ("snap_index", np.uint64), ("snap_term", np.uint64), ("max_ents", np.uint64))}
        a.update({k: _to_np(ft[k], np.uint64)[sub].copy() for k in ("term", "committed",
                                                                    "last_index", "last_term")})
        a.update({k: _to_np(lg.t[k], np.uint64)[rows].copy() for k in ("run_start", "run_term")})
        a.update({k: _to_np(lg.t[k], dt)[slots].copy() for k, dt in (
            ("match", np.uint64), ("next", np.uint64), ("pending_snapshot", np.uint64),
            ("pstate", np.uint8), ("infl_pos", np.uint32))})
        a["infl_buf"] = _to_np(lg.t["infl_buf"], np.uint64)[
            (slots[:, None] * W + np.arange(W)[None, :]).ravel()].copy()
        a["off"] = np.arange(len(sub) + 1, dtype=np.uint32) * n
        a["old_off"] = np.arange(len(sub) + 1, dtype=np.uint32) * n0
        a["ids"], a["old_ids"] = _to_np(ids, np.uint64)[slots], _to_np(old_ids, np.uint64)[oslots]
        a["self_id"] = _to_np(es.self_id, np.uint64)[sub].copy()
        a["role"] = state.role.cpu().numpy()[sub].copy()
        a["votes"] = _to_np(es.votes, np.uint32)[sub].copy()
        a["rq_meta"] = np.zeros(1, np.uint32)
        return a
    lg.t["meta"].copy_(meta0)
    lg.t["pstate"].copy_(pstate0)
    a0 = gather()
    fill = R.FILL - (1 << 64)
    for t_ in (out.swflags, out.slot_map, out.msg_type):
        t_.fill_(R.FILL8)
    for t_ in (out.msg_index, out.msg_log_term, out.msg_n):
        t_.fill_(fill)
    _lib.check(fn(*args), "qb_dev_switch_config")
    torch.cuda.synchronize()
    want = R.new_out(len(sub), len(oslots), len(slots))
    R.switch_config(a0, np.full(len(sub), R.SW_SWITCH, np.uint8), W, 0, want, R.new_stats())
    a1 = gather()
    ok = all(np.array_equal(a1[k], a0[k]) for k in a0)
    got = {"swflags": out.swflags.cpu().numpy()[sub], "slot_map": out.slot_map.cpu().numpy()[oslots],
           "msg_type": out.msg_type.cpu().numpy()[slots]}
    got.update({k: _to_np(getattr(out, k), np.uint64)[slots]
                for k in ("msg_index", "msg_log_term", "msg_n")})
    ok = ok and all(np.array_equal(got[k], want[k][:len(got[k])]) for k in got)
    # sparse: one group in a hundred acts
    action.copy_(torch.where(g64 % 100 == 0, qs.SW_SWITCH, qs.SW_NONE).to(torch.uint8))
    t_sparse, st = timed()
    acting = int((np.arange(G) % 100 == 0).sum())
    assert st["switched"] == reps * acting and st["msg_app"] == reps * acting, st
    # per acting group, read: action 1, old_off / off 8, cfg 4, meta 4, role 1,
    # self_id / term / committed / first / last / last_term / max_ents 56, votes
    # 4, the ID lists (5 + 6) * 8 = 88, match 6 * 8 = 48; written: swflags 1,
    # slot_map 5, meta 0 (unchanged) = 220 B.  Per new slot, read: next 8,
    # pstate 1, infl_pos 4; written: msg_type 1 = 14 B; the new member's
    # message adds the run row 16 read and msg_* 24, pstate 1 written = 41 B.
    dense_b = 220 + n * 14 + 41
    extra = {"unit": "groups/s", "samples": reps, "inflight_cap": W,
             "dense_us": t_dense * 1e6, "dense_bytes_per_group": dense_b,
             "dense_TBs": G * dense_b / t_dense / 1e12,
             "dense_frac": G * dense_b / t_dense / 1e9 / HBM_PEAK_GBS,
             "sparse_us": t_sparse * 1e6, "sparse_acting_groups": acting,
             "parity": bool(ok),
             "parity_check": f"tests/switch_ref.py over {len(sub)} groups (every 1024th) of the "
                             f"dense call: meta, committed, votes, Progress, rings, swflags, "
                             f"slot_map and msg_* (untouched elements included)",
             "timing": "one HIP event pair per call, median over the samples; per_launch_us = "
                       "the dense case, every group adding one voter to five"}
    reporter("switch-config (switchToConfig behind an added voter: renumber, maybeCommit, probe)",
             G, t_dense, G * dense_b, extra)
    assert ok, "switch-config parity failed"


def requests_config(G, reps, *, reporter=None):
    """The batched requests (qb_dev_leader_requests): G five-voter leader groups
    of the synth_streaming table (own slot 0, one term run, committed inside
    it) with a read queue of 4 rows.  Sample (a): one local ReadOnlySafe read
    per group against an empty queue — the row is written, the count grows and
    four hb_commit go out.  Sample (b): the same plus a transfer to a
    caught-up peer (slot 1): transferee set, election_elapsed zeroed,
    MsgTimeoutNow.  One HIP event pair per call, median over the samples after
    warm-up; meta (queue count, transferee), election_elapsed and the Progress
    columns are put back between samples outside the timed call.  Parity: one
    more call at the same size with seeded roles, own slots, terms, queues,
    peer Progress and requests, every 1024th group against
    tests/request_ref.py."""
    reporter = reporter or report
    import ctypes as C
    import importlib
    import time
    from etcd_amd import _lib
    from etcd_amd.quorum import request as qr, tick as qt
    from etcd_amd.quorum.leader import MAX_RUNS, _to_np, synth_streaming
    from tests import request_pack as Q, request_ref as R
    qc = importlib.import_module("etcd_amd.quorum.campaign")
    n, W, D, QC, MR = 5, 4, 64, 4, 2
    lg, _ = synth_streaming(G, W=W, D=D, n=n, device=dev)
    S = lg.S
    lg.readq_cap = QC
    lg.t["rq_ctx"] = torch.zeros(G * QC, dtype=torch.int64, device=dev)
    lg.t["rq_index"] = torch.zeros(G * QC, dtype=torch.int64, device=dev)
    lg.t["rq_meta"] = torch.zeros(G * QC, dtype=torch.int32, device=dev)
    z32 = lambda: torch.zeros(G, dtype=torch.int32, device=dev)  # noqa: E731
    state = qt.TickState(torch.full((G,), qt.ROLE_LEADER | qt.ROLE_PROMOTABLE, dtype=torch.uint8,
                                    device=dev), z32(), z32(), z32())
    lg.t["meta"].fill_(0xFF00 | (1 << 16))  # own slot 0, no transferee, one term run, queue empty
    es = qc.ElectionState.for_table(lg, state, np.arange(1, G + 1, dtype=np.uint64),
                                    np.zeros(G, np.uint64), np.arange(1, G + 1, dtype=np.uint64),
                                    np.full(G, 7, np.uint64), 10, True, True)
    slot = torch.arange(S, device=dev) % n
    own = slot == 0
    gs = torch.arange(S, device=dev) // n
    last = lg.t["last_index"][gs]
    lg.t["match"] = torch.where(slot <= 1, last, lg.t["match"])   # slot 1 is caught up
    ib = qr.RequestInbox(MR, torch.ones(G, dtype=torch.uint8, device=dev),
                         torch.arange(1, MR * G + 1, dtype=torch.int64, device=dev),
                         torch.full((MR * G,), 0xFF, dtype=torch.uint8, device=dev),
                         torch.full((G,), 0xFF, dtype=torch.uint8, device=dev),
                         torch.zeros(G, dtype=torch.int64, device=dev))
    out = qr.new_result(G, S, MR, dev)
    rg, rin, rout = qr.request_structs(lg, es, ib, out)  # (the mirror's checks, once)
    sp = torch.cuda.current_stream(dev).cuda_stream
    fn = _lib.fn("qb_dev_leader_requests")
    args = (C.byref(rg), C.byref(rin), C.byref(rout), out.stats.data_ptr(), sp)

    def call():
        _lib.check(fn(*args), "qb_dev_leader_requests")
    keys = ("meta", "match", "next", "pending_snapshot", "pstate", "infl_pos")
    keep = {k: lg.t[k].clone() for k in keys}

    def timed(xf):
        ib.xf_from.fill_(xf)

        def restore():
            for k, v in keep.items():
                lg.t[k].copy_(v)
            state.election_elapsed.fill_(3)

        def sample(ev):
            restore()
            torch.cuda.synchronize()
            ev.record(ev.ev[0], sp)
            call()
            ev.record(ev.ev[1], sp)
            torch.cuda.synchronize()
            return ev.elapsed_ms(0, 1) / 1e3
        ev = HipEvents(2)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.3:  # warm-up: clocks settle (time_region)
            sample(ev)
        out.stats.zero_()
        per = [sample(ev) for _ in range(reps)]
        ev.close()
        return float(np.median(per)), out.stats_dict()
    t_read, st = timed(0xFF)
    assert st["bcast"] == reps * G and st["bcast_groups"] == reps * G and st["xf_started"] == 0, st
    assert bool(((lg.t["meta"] >> 20) & 0x1F == 1).all())
    assert bool((out.hb_commit.view(G, n)[:, 2:] == lg.t["committed"][:, None]).all())
    t_both, st = timed(1)
    assert st["bcast"] == reps * G and st["xf_timeout_now"] == reps * G, st
    assert bool((state.election_elapsed == 0).all()) and bool(((lg.t["meta"] >> 8) & 0xFF == 1).all())
    # per group, sample (a).  Read: n_reads 1, xf_from 1, role 1, meta 4, cfg 4,
    # off 4, term / lead / committed / first_index / last_index / last_term 48,
    # rd_ctx 8, rd_from 1 = 72 B; written: the queue row 8 + 8 + 4, meta 4,
    # rd_status 1, qflags 1, xf_type 1 = 27 B; per peer: match 8 read, hb_commit
    # 8 written = 16 B.  Sample (b) adds xf_term 8 and the transferee's match 8
    # read, election_elapsed 4 written.
    read_b = 72 + 27 + (n - 1) * 16
    both_b = read_b + 20
    extra = {"unit": "groups/s", "samples": reps, "readq_cap": QC, "max_reads": MR,
             "read_us": t_read * 1e6, "read_bytes_per_group": read_b,
             "read_TBs": G * read_b / t_read / 1e12,
             "read_frac": G * read_b / t_read / 1e9 / HBM_PEAK_GBS,
             "read_transfer_us": t_both * 1e6, "read_transfer_bytes_per_group": both_b,
             "read_transfer_TBs": G * both_b / t_both / 1e12,
             "read_transfer_frac": G * both_b / t_both / 1e9 / HBM_PEAK_GBS,
             "timing": "one HIP event pair per call, median over the samples; per_launch_us = "
                       "sample (a), one local safe read per group"}
    # parity at this size
    for k, v in keep.items():
        lg.t[k].copy_(v)
    gen = torch.Generator(device=dev).manual_seed(0x4EAD5)
    rnd = lambda hi, k: torch.randint(0, hi, (k,), generator=gen, device=dev)  # noqa: E731
    ft = es.follower.t
    state.role.copy_((torch.where(rnd(4, G) == 0, rnd(4, G), torch.full((G,), 2, device=dev))
                      | (1 << 7)).to(torch.uint8))
    state.election_elapsed.copy_(rnd(9, G).to(torch.int32))
    ft["lead"].copy_(rnd(2, G) * 9)
    ft["term"].copy_(ft["term"] + torch.where(rnd(8, G) == 0, 1, 0))    # some have nothing committed
    one = torch.ones(G, dtype=torch.int64, device=dev)
    lg.t["cfg"].copy_(torch.where(rnd(16, G) == 0, one << rnd(n, G),    # singletons, learners
                                  torch.where(rnd(8, G) == 0, 0b01111, 0b11111)).to(torch.int32))
    nq = rnd(QC + 1, G)
    lg.t["meta"].copy_((rnd(n + 1, G) | (1 << 16) | nq << 20 | rnd(2, G) << 25
                        | torch.where(rnd(8, G) == 0, rnd(n, G), torch.full((G,), 0xFF, device=dev))
                        << 8).to(torch.int32))
    k_ = torch.arange(G * QC, device=dev) % QC
    livek = k_ < nq.repeat_interleave(QC)
    fill = Q.FILL - (1 << 64)
    lg.t["rq_ctx"].copy_(torch.where(livek, 100 + k_, fill))
    lg.t["rq_index"].copy_(torch.where(livek, rnd(1000, G * QC), fill))
    lg.t["rq_meta"].copy_(torch.where(livek, rnd(1 << n, G * QC) | (rnd(2, G * QC) * 0xFF) << 16,
                                      Q.FILL32 - (1 << 32)).to(torch.int32))
    lg.t["next"].copy_(torch.where(own, keep["next"],
                                   torch.where(rnd(16, S) == 0, lg.t["first_index"][gs] - 5,
                                               last + 1 - rnd(200, S))))   # (some behind the log)
    lg.t["match"].copy_(torch.where(own | (rnd(3, S) == 0), last, last - 200 + rnd(201, S)))
    lg.t["pstate"].copy_(torch.where(own, torch.full((S,), 1 | 8, device=dev),
                                     rnd(3, S) | rnd(4, S) << 2).to(torch.uint8))
    lg.t["infl_pos"].copy_((rnd(W, S) | rnd(W + 1, S) << 16).to(torch.int32))
    ib.n_reads.copy_(rnd(MR + 2, G).to(torch.uint8))
    pool = torch.tensor([0, 100, 101, 102, 103, 200, 201, 202], device=dev)
    ib.rd_ctx.copy_(pool[rnd(len(pool), MR * G)])
    frm = torch.tensor([0xFF, 0xFF, 0, 1, n - 1, n, 0xFE], device=dev)
    ib.rd_from.copy_(frm[rnd(len(frm), MR * G)].to(torch.uint8))
    xfr = torch.tensor([0xFF, 0xFF, 0, 1, 2, 3, 4, n], device=dev)
    ib.xf_from.copy_(xfr[rnd(len(xfr), G)].to(torch.uint8))
    ib.xf_term.copy_(torch.where(rnd(2, G) == 0, 0, ft["term"] - 1 + rnd(3, G)))
    sub = np.arange(0, G, 1024)
    slots = (sub[:, None] * n + np.arange(n)[None, :]).ravel()
    rows = (np.arange(MAX_RUNS)[:, None] * G + sub[None, :]).ravel()
    ring = (slots[:, None] * W + np.arange(W)[None, :]).ravel()
    qrows = (sub[:, None] * QC + np.arange(QC)[None, :]).ravel()
    rdrows = (np.arange(MR)[:, None] * G + sub[None, :]).ravel()

    def gather():
        a = {k: _to_np(lg.t[k], dt)[sub].copy() for k, dt in (
            ("cfg", np.uint32), ("meta", np.uint32), ("term", np.uint64), ("committed", np.uint64),
            ("first_index", np.uint64), ("last_index", np.uint64), ("snap_index", np.uint64),
            ("snap_term", np.uint64), ("max_ents", np.uint64))}
        a.update({k: _to_np(lg.t[k], np.uint64)[rows].copy() for k in ("run_start", "run_term")})
        a.update({k: _to_np(lg.t[k], dt)[slots].copy() for k, dt in (
            ("match", np.uint64), ("next", np.uint64), ("pending_snapshot", np.uint64),
            ("pstate", np.uint8), ("infl_pos", np.uint32))})
        a["infl_buf"] = _to_np(lg.t["infl_buf"], np.uint64)[ring].copy()
        a.update({k: _to_np(lg.t[k], dt)[qrows].copy() for k, dt in (
            ("rq_ctx", np.uint64), ("rq_index", np.uint64), ("rq_meta", np.uint32))})
        a["off"] = np.arange(len(sub) + 1, dtype=np.uint32) * n
        e = {k: v[sub].copy() for k, v in es.numpy().items()}
        return a, e
    a0, e0 = gather()
    nodes = Q.nodes_from_arrays(a0, e0, QC, W)
    inp = {"n_reads": ib.n_reads.cpu().numpy()[sub].copy(),
           "rd_ctx": _to_np(ib.rd_ctx, np.uint64)[rdrows].copy(),
           "rd_from": ib.rd_from.cpu().numpy()[rdrows].copy(),
           "xf_from": ib.xf_from.cpu().numpy()[sub].copy(),
           "xf_term": _to_np(ib.xf_term, np.uint64)[sub].copy()}
    for t_ in (out.rd_status, out.xf_type, out.qflags):
        t_.fill_(Q.FILL8)
    for t_ in (out.rd_index, out.hb_commit, out.xf_index, out.xf_log_term, out.xf_n):
        t_.fill_(fill)
    out.stats.zero_()
    call()
    torch.cuda.synchronize()
    want = Q.new_out(len(sub), len(slots), MR)
    Q.ref_requests(nodes, inp, R.Config(R.SAFE, QC, MR), a0["off"], want)
    want_a, want_e = Q.pack_nodes(nodes, QC, W)
    a1, e1 = gather()
    where = {"rd_status": rdrows, "rd_index": rdrows, "hb_commit": slots}
    ok = (all(np.array_equal(a1[k], want_a[k]) for k in (
              "meta", "committed", "match", "next", "pending_snapshot", "pstate", "infl_pos",
              "infl_buf", "rq_ctx", "rq_index", "rq_meta"))
          and all(np.array_equal(e1[k], want_e[k]) for k in want_e)
          and all(np.array_equal(_to_np(getattr(out, k), w.dtype)[where.get(k, sub)], w)
                  for k, w in want.items()))
    st = out.stats_dict()
    ok = ok and all(v > 0 for v in st.values())   # every outcome was reached
    extra["parity"] = bool(ok)
    extra["parity_check"] = (f"tests/request_ref.py over {len(sub)} groups (every 1024th) of the "
                             f"{G} with seeded roles, own slots, configs, terms, queues, peer "
                             f"Progress, reads and transfers: meta, the queue rows, Progress, rings, "
                             f"the election state, rd_* / hb_commit / xf_* / qflags (untouched "
                             f"elements included); the call's stats: {st}")
    reporter("requests (one safe MsgReadIndex per group: queue row + heartbeats)", G, t_read,
             G * read_b, extra)
    assert ok, "requests parity failed"


def ready_config(G, reps, *, reporter=None):
    """Ready + Advance (qb_dev_ready, qb_dev_advance) over G five-voter leader
    groups of the synth_streaming table.  Two samples: 1 % of the groups ready
    (every 100th) and all of them; a ready group has one unstable entry, one
    committed entry to apply, a HardState whose commit moved and messages
    pending.  A sample is one accepting qb_dev_ready with room for every group
    and one qb_dev_advance over the list it wrote, the list's columns handed
    back as they are (the host's I/O between the two is not modelled), behind
    which every group is idle again.  HIP events before, between and behind
    the two calls, median over the samples after warm-up; the eleven state
    columns are put back between samples outside the timed calls; calls
    straight to the C ABI.  Parity: one more Ready and Advance at the same size
    over seeded state — the flags and the compaction of all G groups against
    numpy, every 1024th group against tests/ready_ref.py."""
    reporter = reporter or report
    import ctypes as C
    import importlib
    import time
    from etcd_amd import _lib
    from etcd_amd.quorum import tick as qt
    from etcd_amd.quorum.leader import MAX_RUNS, synth_streaming
    from tests import ready_pack as P, ready_ref as R
    qc = importlib.import_module("etcd_amd.quorum.campaign")
    qy = importlib.import_module("etcd_amd.quorum.ready")
    n = 5
    lg, _ = synth_streaming(G, W=4, D=64, n=n, device=dev)
    z32 = lambda: torch.zeros(G, dtype=torch.int32, device=dev)  # noqa: E731
    z64 = lambda: torch.zeros(G, dtype=torch.int64, device=dev)  # noqa: E731
    tstate = qt.TickState(torch.full((G,), qt.ROLE_LEADER | qt.ROLE_PROMOTABLE, dtype=torch.uint8,
                                     device=dev), z32(), z32(), z32())
    es = qc.ElectionState.for_table(lg, tstate, np.arange(1, G + 1, dtype=np.uint64),
                                    np.ones(G, np.uint64), np.ones(G, np.uint64),
                                    np.full(G, 7, np.uint64), 10, True, True)
    ft, t = es.follower.t, lg.t
    shared = {"term": ft["term"], "vote": ft["vote"], "committed": ft["committed"],
              "lead": ft["lead"], "role": tstate.role, "first_index": t["first_index"],
              "last_index": ft["last_index"], "last_term": ft["last_term"], "meta": t["meta"],
              "run_start": t["run_start"], "run_term": t["run_term"], "pending_conf_index": z64(),
              "ext": z32()}
    st = qy.ReadyState.new_raw_node(shared, ft["committed"].clone(), z64())
    s = st.t
    idle = {k: s[k].clone() for k in P.STATE}
    out = qy.new_ready_result(G, G, dev)
    pay = torch.full((G,), 8, dtype=torch.int64, device=dev)
    recs = qy.AdvanceRecords(G, {"adv_gid": out.cols["ready_gid"], "hs_term": out.cols["hs_term"],
                                 "hs_vote": out.cols["hs_vote"], "hs_commit": out.cols["hs_commit"],
                                 "applied_to": out.cols["apply_hi"], "applied_payload": pay,
                                 "stable_index": out.cols["ent_hi"],
                                 "stable_term": out.cols["ent_last_term"],
                                 "stable_snap": out.cols["snap_index"]})
    ares = qy.AdvanceResult(torch.zeros(G, dtype=torch.uint8, device=dev),
                            torch.zeros(len(qy.ASTAT_NAMES), dtype=torch.int64, device=dev))
    qy.ready(st, accept=False, out=out)       # (the mirror's checks and the workspace, once)
    qy.advance(st, qy.AdvanceRecords(0, recs.t), out=ares)
    out.stats.zero_()
    rg = st.struct()
    ro = qy.ReadyOutC(rflags=out.rflags.data_ptr(), ready_count=out.ready_count.data_ptr(),
                      **{k: out.cols[k].data_ptr() for k in qy._LIST})
    ai = qy.AdvanceInC(**{k: recs.t[k].data_ptr() for k in qy._ADV})
    sp = torch.cuda.current_stream(dev).cuda_stream
    f_ready, f_adv = _lib.fn("qb_dev_ready"), _lib.fn("qb_dev_advance")
    ws = st._ws

    def call_ready(accept, cap):
        _lib.check(f_ready(C.byref(rg), accept, cap, C.byref(ro), out.stats.data_ptr(),
                           ws.data_ptr(), ws.numel(), sp), "qb_dev_ready")

    def call_advance(A):
        _lib.check(f_adv(C.byref(rg), A, C.byref(ai), ares.aflags.data_ptr(),
                         ares.stats.data_ptr(), sp), "qb_dev_advance")

    def timed(every):
        g = torch.arange(G, device=dev)
        on = g % every == 0
        Rn = int(on.sum().item())
        work = {k: v.clone() for k, v in idle.items()}
        work["unstable_offset"] = torch.where(on, ft["last_index"], idle["unstable_offset"])
        work["applied"] = torch.where(on, ft["committed"] - 1, idle["applied"])
        work["prev_commit"] = torch.where(on, ft["committed"] - 1, idle["prev_commit"])
        work["pending"] = on.to(torch.uint8) * qy.RDP_MSGS
        work["uncommitted_size"] = on.to(torch.int64) * 16

        def sample(ev):
            for k, v in work.items():
                s[k].copy_(v)
            torch.cuda.synchronize()
            ev.record(ev.ev[0], sp)
            call_ready(1, G)
            ev.record(ev.ev[1], sp)
            call_advance(Rn)
            ev.record(ev.ev[2], sp)
            torch.cuda.synchronize()
            return ev.elapsed_ms(0, 1) / 1e3, ev.elapsed_ms(1, 2) / 1e3
        ev = HipEvents(3)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.3:  # warm-up: clocks settle (time_region)
            sample(ev)
        out.stats.zero_()
        ares.stats.zero_()
        per = [sample(ev) for _ in range(reps)]
        ev.close()
        rs, as_ = out.stats_dict(), ares.stats_dict()
        assert int(out.ready_count.cpu()[0]) == Rn and rs["listed"] == reps * Rn, rs
        assert rs["entries"] == rs["committed"] == rs["hard"] == rs["msgs"] == reps * Rn, rs
        assert as_["stable"] == as_["applied"] == as_["hardstate"] == reps * Rn, as_
        assert all(bool((s[k] == idle[k]).all()) for k in P.STATE if k != "uncommitted_size")
        call_ready(0, G)                       # behind the Advance nothing is ready
        assert int(out.ready_count.cpu()[0]) == 0
        return (float(np.median([a for a, _ in per])), float(np.median([b for _, b in per])), Rn)

    # Bytes per group, the columns each launch touches (not a traffic counter).
    # R1: 13 u64 columns + role, prev_role, pending read, rflags written.
    r1_b = 13 * 8 + 3 + 2
    # R2: rflags read per group; per listed group of these samples lead 8, role
    # 1, committed 8, applied 8, first_index 8, term 8, vote 8, unstable_offset
    # 8, last_index 8, last_term 8 read, the record (4 + 2 + 10 * 8 + 1)
    # and pending written.
    r2_b, r2_rec = 2, 73 + 87 + 1
    # Advance, per record: the nine columns 68 read, aflags 1 written; applied,
    # committed, uncommitted_size, unstable_offset, last_index, last_term read
    # 48; prev_* 24, applied 8, uncommitted_size 8, unstable_offset 8 written.
    adv_rec = 68 + 1 + 48 + 48
    rows = {}
    for name, every in (("all", 1), ("one_percent", 100)):
        t_r, t_a, Rn = timed(every)
        b = G * (r1_b + r2_b) + Rn * (r2_rec + adv_rec)
        rows[name] = {"ready_groups": Rn, "ready_us": t_r * 1e6, "advance_us": t_a * 1e6,
                      "ready_advance_us": (t_r + t_a) * 1e6, "bytes": b,
                      "TBs": b / (t_r + t_a) / 1e12,
                      "frac": b / (t_r + t_a) / 1e9 / HBM_PEAK_GBS}
    extra = {"unit": "groups/s", "samples": reps,
             "bytes_per_group": {"k_ready_flags": r1_b, "k_ready_write": r2_b,
                                 "k_ready_write_per_listed": r2_rec, "k_advance_per_record": adv_rec},
             "timing": "HIP events before, between and behind qb_dev_ready and qb_dev_advance, "
                       "median over the samples; per_launch_us = ready + advance, every group "
                       "ready", **{f"{k}_{f}": v for k, r in rows.items() for f, v in r.items()}}

    # ---- parity at this size over seeded state ---------------------------
    gen = torch.Generator(device=dev).manual_seed(0x4EAD7)
    rnd = lambda hi: torch.randint(0, hi, (G,), generator=gen, device=dev)  # noqa: E731
    for k, v in idle.items():
        s[k].copy_(v)
    act = rnd(4) == 0
    w = lambda a, b: torch.where(act, a, b)  # noqa: E731
    last, com = ft["last_index"], ft["committed"]
    s["applied"].copy_(w(com - rnd(3), idle["applied"]))
    s["unstable_offset"].copy_(w(torch.where(rnd(64) == 0, last + 3, last + 1 - rnd(3)),
                                 idle["unstable_offset"]))
    s["prev_commit"].copy_(w(com - rnd(2), idle["prev_commit"]))
    s["prev_term"].copy_(w(ft["term"] - (rnd(16) == 0).long(), idle["prev_term"]))
    s["prev_lead"].copy_(w(ft["lead"] + (rnd(8) == 0).long(), idle["prev_lead"]))
    s["prev_role"].copy_(w(torch.where(rnd(8) == 0, 1, 2), z64() + 2).to(torch.uint8))
    s["pending"].copy_(w(torch.where(rnd(4) == 0, rnd(4), z64()), z64()).to(torch.uint8))
    s["usnap_index"].copy_(w(torch.where(rnd(32) == 0, 5 + rnd(3), z64()), idle["usnap_index"]))
    s["usnap_term"].copy_(torch.where(s["usnap_index"] != 0, 7, 0))
    s["uncommitted_size"].copy_(w(rnd(3) * 8, idle["uncommitted_size"]))
    st.t["ext"].copy_((rnd(16) == 0).to(torch.int32) << 16)     # AutoLeave, the change pending
    st.t["pending_conf_index"].copy_(com)                       # at the commit index
    sub = np.arange(0, G, 1024)
    rows_ = (np.arange(MAX_RUNS)[:, None] * G + sub[None, :]).ravel()

    def gather():
        a = st.numpy()
        return {k: (v[rows_] if k.startswith("run_") else v[sub]).copy() for k, v in a.items()}
    nodes = P.nodes_from_arrays(gather())
    call_ready(0, G)
    count = int(out.ready_count.cpu()[0])
    cap = count - 5
    for c_ in out.cols.values():
        c_.fill_(255 if c_.dtype == torch.uint8 else -1)
    out.stats.zero_()
    ares.stats.zero_()
    call_ready(1, cap)
    call_advance(cap)
    torch.cuda.synchronize()
    rf = out.rflags.cpu().numpy().view(np.uint16)[:G]
    rdy = np.flatnonzero(rf & ~np.uint16(R.RDF_MUST_SYNC | R.RDF_DEFERRED))
    cols = {k: out.cols[k].cpu().numpy().view(dt) for k, dt in P.LIST.items()}
    ok = (len(rdy) == count == int(out.ready_count.cpu()[0])
          and np.array_equal(cols["ready_gid"][:cap], rdy[:cap].astype(np.uint32))
          and np.array_equal(cols["rd_flags"][:cap], rf[rdy[:cap]])
          and bool((cols["ready_gid"][cap:] == 0xFFFFFFFF).all())
          and np.array_equal(np.flatnonzero(rf & R.RDF_DEFERRED), rdy[cap:]))
    # every 1024th group against the restatement: its flags, its record, its
    # Advance (groups are independent but for the list position and the cap)
    pos = np.searchsorted(rdy, sub)
    recs_ref = []
    for i, (g, nd) in enumerate(zip(sub, nodes)):
        f, rd = R.ready_flags(nd)
        listed = bool(f & ~R.RDF_MUST_SYNC) and pos[i] < cap
        if f & ~R.RDF_MUST_SYNC and not listed:
            f |= R.RDF_DEFERRED
        ok = ok and int(rf[g]) == f
        if not listed:
            continue
        _, rr, _, _ = R.ready_call([nd], True, 1)
        r = rr[0]
        p = int(pos[i])
        got = tuple(int(cols[k][p]) for k in ("hs_term", "hs_vote", "hs_commit", "ent_lo", "ent_hi",
                                              "ent_last_term", "apply_lo", "apply_hi", "snap_index",
                                              "lead", "role"))
        ok = ok and got == r.hs + r.ent + r.apply + (r.snap_index, r.lead, r.role)
        fl = R.advance(nd, R.AdvanceRecord(0, r.hs, r.apply[1], 8, r.ent[1], r.ent[2],
                                           r.snap_index))
        ok = ok and int(ares.aflags[p].item()) == fl
    want = P.pack_nodes(nodes)
    got = gather()
    ok = ok and all(np.array_equal(got[k], want[k]) for k in P.STATE)
    rs, as_ = out.stats_dict(), ares.stats_dict()
    ok = ok and all(v > 0 for v in rs.values()) and rs["listed"] == cap and rs["deferred"] == 5
    ok = ok and all(as_[k] > 0 for k in ("hardstate", "applied", "stable", "snap_stable",
                                         "auto_leave"))
    extra["parity"] = bool(ok)
    extra["parity_check"] = (f"all {G} groups' flags compacted against numpy ({count} ready, the "
                             f"last 5 deferred); tests/ready_ref.py over {len(sub)} groups (every "
                             f"1024th): rflags, the record, aflags and the eleven state columns "
                             f"behind Ready + Advance; stats: {rs} {as_}")
    reporter("ready + advance (every group ready: one entry to persist, one to apply)", G,
             (rows["all"]["ready_us"] + rows["all"]["advance_us"]) / 1e6, rows["all"]["bytes"], extra)
    assert ok, "ready parity failed"


def snapshot_config(G, reps, *, reporter=None):
    """The batched MsgSnap step (qb_dev_follower_snapshot) over G follower
    groups of the synth_streaming table (node 2 of five voters, leader 1
    known, one term run).  Every record is a same-term MsgSnap from the leader
    100 past the group's last index with a five-voter ConfState: it restores.
    Row (a): a record for every group; row (b): for every 100th.  Records
    arrive in shuffled group order, as the follower rows' do; (a) is also
    timed in ascending order, the order qb_dev_advance's row has.  One HIP
    event pair per call, median over the samples after warm-up; the eighteen
    state columns are put back between samples outside the timed call; calls
    straight to the C ABI.  Parity at this size: tests/snapshot_ref.py over
    every 1024th group after one call of row (a) — sflags, the response and
    every state column — and the whole batch's counters."""
    reporter = reporter or report
    import ctypes as C
    import importlib
    import time
    from etcd_amd import _lib
    from etcd_amd.quorum import follower as qf, snapshot as qs, tick as qt
    from etcd_amd.quorum.leader import MAX_RUNS, synth_streaming
    from tests import snapshot_pack as P, snapshot_ref as S
    qy = importlib.import_module("etcd_amd.quorum.ready")
    n, ET = 5, 10
    lg, _ = synth_streaming(G, W=4, D=64, n=n, device=dev)
    t = lg.t
    i64 = lambda v: torch.full((G,), v, dtype=torch.int64, device=dev)  # noqa: E731
    z32 = lambda: torch.zeros(G, dtype=torch.int32, device=dev)  # noqa: E731
    tstate = qt.TickState(torch.full((G,), qt.ROLE_PROMOTABLE, dtype=torch.uint8, device=dev),
                          torch.ones(G, dtype=torch.int32, device=dev), z32(), z32())
    ft = {"term": t["term"], "vote": i64(1), "lead": i64(1), "committed": t["committed"],
          "last_index": t["last_index"], "last_term": i64(7)}
    fg = qf.FollowerGroups(G, ET, True, True, ft, tstate)
    flog = qf.FollowerLog(G, t["meta"], t["first_index"], t["run_start"], t["run_term"])
    ready = qy.ReadyState(G, {"unstable_offset": t["last_index"] + 1, "usnap_index": i64(0),
                              "usnap_term": i64(0),
                              "pending": torch.zeros(G, dtype=torch.uint8, device=dev)})
    self_id = i64(2)
    cols = {"self_id": self_id, **ft, "role": tstate.role,
            "election_elapsed": tstate.election_elapsed,
            "heartbeat_elapsed": tstate.heartbeat_elapsed, "first_index": t["first_index"],
            "meta": t["meta"], "run_start": t["run_start"], "run_term": t["run_term"],
            **ready.t}
    assert set(cols) == set(P.STATE)
    pristine = {k: v.clone() for k, v in cols.items()}
    sp = torch.cuda.current_stream(dev).cuda_stream
    fn = _lib.fn("qb_dev_follower_snapshot")

    def inbox_of(groups):
        """One restoring MsgSnap per group of ``groups`` (a device tensor)."""
        Rn = int(groups.numel())
        ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev).repeat(Rn)
        tt = {"group": groups.to(torch.int32), "from": torch.ones_like(groups),
              "term": pristine["term"][groups], "snap_index": pristine["last_index"][groups] + 100,
              "snap_term": torch.full_like(groups, 8),
              "cs_off": (torch.arange(Rn + 1, dtype=torch.int64, device=dev) * n).to(torch.int32),
              "cs_id": ids, "cs_set": torch.zeros(Rn * n, dtype=torch.uint8, device=dev)}
        return qs.SnapshotInbox(Rn, Rn * n, tt)

    def caller(ib, res):
        qs.follower_snapshot(fg, flog, ready, self_id, ib, out=res, check_distinct=False)  # the checks, once
        sg = qs.SnapshotGroupsC(G=G, election_timeout=ET, check_quorum=1, pre_vote=1, reserved=0,
                                **{k: cols[k].data_ptr() for k in qs._GROUP_FIELDS})
        ibc = qs.SnapshotInboxC(R=ib.R, C=ib.C, **{k: v.data_ptr() for k, v in ib.t.items()})
        so = qs.SnapshotOutC(sflags=res.sflags.data_ptr(), resp_type=res.resp_type.data_ptr(),
                             resp_term=res.resp_term.data_ptr(), resp_index=res.resp_index.data_ptr())
        keep = (sg, ibc, so)
        return lambda: _lib.check(fn(C.byref(keep[0]), C.byref(keep[1]), C.byref(keep[2]),
                                     res.stats.data_ptr(), sp), "qb_dev_follower_snapshot")

    def put_back():
        for k, v in pristine.items():
            cols[k].copy_(v)

    def timed(groups):
        ib = inbox_of(groups)
        res = qs.new_snapshot_result(ib.R, dev)
        call = caller(ib, res)

        def sample(ev):
            put_back()
            torch.cuda.synchronize()
            ev.record(ev.ev[0], sp)
            call()
            ev.record(ev.ev[1], sp)
            torch.cuda.synchronize()
            return ev.elapsed_ms(0, 1) / 1e3
        ev = HipEvents(2)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.3:  # warm-up: clocks settle (time_region)
            sample(ev)
        res.stats.zero_()
        ts = [sample(ev) for _ in range(reps)]
        ev.close()
        st = res.stats_dict()
        assert st["restored"] == reps * ib.R and sum(st.values()) == reps * ib.R, st
        return float(np.median(ts)), ib, res, call

    # Bytes per restoring record, the columns the launch touches (not a traffic
    # counter).  The record: group 4, from / term / snap_index / snap_term 32,
    # cs_off 4, five IDs and their list bytes 45 read; sflags 2, resp_type 1,
    # resp_term 8, resp_index 8 written = 104.  Its group: term, committed,
    # self_id, last_index 32, role 1, meta 4, pending 1 read = 38; lead 8,
    # election_elapsed 4, role 1, committed 8, unstable_offset 8, usnap_index 8,
    # usnap_term 8, last_index 8, last_term 8, first_index 8, run_start 8,
    # run_term 8, pending 1 written = 94 (meta already holds one run).
    rec_b, grp_b = 104, 38 + 94
    every = torch.arange(G, device=dev)
    shuffled = torch.randperm(G, device=dev)
    hundredth = every[every % 100 == 0]
    rows = {}
    for name, groups in (("all", shuffled), ("one_percent", hundredth[torch.randperm(
            int(hundredth.numel()), device=dev)]), ("all_ascending", every)):
        tm, ib, res, call = timed(groups)
        b = ib.R * (rec_b + grp_b)
        rows[name] = {"records": ib.R, "us": tm * 1e6, "bytes": b, "TBs": b / tm / 1e12,
                      "frac": b / tm / 1e9 / HBM_PEAK_GBS}
        if name == "all":
            keep = (ib, res, call)
    extra = {"unit": "groups/s", "samples": reps, "bytes_per_record": rec_b + grp_b,
             "timing": "one HIP event pair per call, median over the samples; the state put back "
                       "outside the timed call; per_launch_us = every group, shuffled",
             **{f"{k}_{f}": v for k, r in rows.items() for f, v in r.items()}}

    # ---- parity at this size: one call of row (a) from the pristine state ----
    ib, res, call = keep
    put_back()
    res.stats.zero_()
    torch.cuda.synchronize()
    sub = np.arange(0, G, 1024)
    rows_ = (np.arange(MAX_RUNS)[:, None] * G + sub[None, :]).ravel()

    def gather():
        out = {}
        for k, dt in P.STATE.items():
            a = cols[k].cpu().numpy().view(dt)
            out[k] = (a[rows_] if k in P.ROWS else a[sub]).copy()
        return out
    before = gather()
    call()
    torch.cuda.synchronize()
    after = gather()
    nodes = P.nodes_from_arrays(before)
    grp = ib.t["group"].cpu().numpy().view(np.uint32)
    pos = np.flatnonzero(grp % 1024 == 0)
    where = {int(g): j for j, g in enumerate(sub)}
    rc = {k: ib.t[k].cpu().numpy().view(dt)[pos] for k, dt in (
        ("from", np.uint64), ("term", np.uint64), ("snap_index", np.uint64),
        ("snap_term", np.uint64))}
    recs = [(where[int(grp[i])], S.Snap(int(rc["from"][k]), int(rc["term"][k]),
                                        int(rc["snap_index"][k]), int(rc["snap_term"][k]),
                                        {"voters": list(range(1, n + 1))}))
            for k, i in enumerate(pos)]
    ref = S.snapshot_call(nodes, recs)
    want = P.pack_nodes(nodes, base=before)
    ok = all(np.array_equal(after[k], want[k]) for k in P.STATE)
    got = {"sflags": res.sflags, "resp_type": res.resp_type, "resp_term": res.resp_term,
           "resp_index": res.resp_index}
    ok = ok and all(np.array_equal(got[k].cpu().numpy().view(dt)[pos], np.array(ref[k], dt))
                    for k, dt in P.OUT.items())
    st = res.stats_dict()
    ok = ok and st == dict(S.new_stats(), restored=G) and ref["stats"]["restored"] == len(sub)
    extra["parity"] = bool(ok)
    extra["parity_check"] = (f"tests/snapshot_ref.py over {len(sub)} groups (every 1024th) of the "
                             f"{G}: sflags, the response and the eighteen state columns behind one "
                             f"call of row (a); the batch's counters: {st}")
    reporter("follower snapshot (every group restores; shuffled arrival order)", G,
             rows["all"]["us"] / 1e6, rows["all"]["bytes"], extra)
    assert ok, "snapshot parity failed"


def encode_config(G, reps, *, reporter=None):
    """The batched Message.Marshal (qb_dev_encode_*), three workloads: (a) the
    heartbeats of G five-voter leader groups through the slot form (every
    group beats, one in ten with a read context: 4G messages and G own
    slots); (b) 4G general columns (MsgAppResp on encode_appresp's domain); (c)
    a list of the leader step's shape, four MsgApp with entries per group in
    group order.  Beside them, in the same session, the decode-side yardstick:
    qb_dev_ingest_messages over (b)'s device bytes and offsets (the streaming
    yardstick, qb_dev_advance with every group ready, is the ready row: run
    ``--only encode,ready``).  One HIP event pair per call, median over the
    samples after warm-up; calls straight to the C ABI.  Parity at this size:
    tests/encode_ref.py over every 1024th message of each workload — bytes,
    offsets, status, ent_at — and the batch's counters."""
    reporter = reporter or report
    import ctypes as C
    import time
    from etcd_amd import _lib
    from etcd_amd.quorum import encode as qe, wire
    from etcd_amd.quorum.leader import MSG_DTYPE
    from tests import encode_ref as E
    n = 5
    S, M = n * G, 4 * G
    sp = torch.cuda.current_stream(dev).cuda_stream
    ar = lambda k: torch.arange(k, dtype=torch.int64, device=dev)  # noqa: E731
    gg, ss = ar(G).repeat_interleave(n), ar(n).repeat(G)
    ids = 16384 + ss * 200000 + gg % 100000
    off = (ar(G + 1) * n).to(torch.int32)
    self_id = 16384 + ar(G) % 100000
    term = torch.full((G,), 20000, dtype=torch.int64, device=dev)
    committed = (1 << 35) + ar(G) * 64
    groups = qe.EncodeGroups(off, ids, self_id, term, S)
    gen = torch.Generator(device=dev).manual_seed(0xE7C0DE)
    rnd = lambda k, hi: torch.randint(0, hi, (k,), generator=gen, dtype=torch.int64, device=dev)  # noqa: E731
    hb_commit = committed.repeat_interleave(n) - rnd(S, 64)
    hb_ctx = torch.where(rnd(G, 10) == 0, (1 << 56) + rnd(G, 1 << 40) + 1, torch.zeros_like(term))
    # (b): responses of the peers, as encode_appresp takes them
    peer = 1 + rnd(M, n - 1)
    gm = ar(M) // 4
    col_b = {"type": torch.full((M,), 4, dtype=torch.uint8, device=dev),
             "to": self_id[gm], "from": 16384 + peer * 200000 + gm % 100000,
             "term": term[gm], "index": committed[gm] + rnd(M, 64),
             "reject": (rnd(M, 10) == 0).to(torch.uint8)}
    # (c): four MsgApp per group, one entry each
    recs = np.zeros(M, MSG_DTYPE)
    gi = np.arange(M, dtype=np.uint64) // 4
    recs["group"], recs["to"], recs["type"] = gi, 1 + np.arange(M) % 4, qe.MSG_APP
    recs["index"], recs["log_term"] = (1 << 35) + gi * 64 + 63, 20000
    recs["commit"], recs["aux"] = (1 << 35) + gi * 64, 1
    msgs = torch.from_numpy(recs.view(np.uint8)).to(dev)
    total = torch.full((1,), M, dtype=torch.int64, device=dev)

    fns = {"slots": _lib.fn("qb_dev_encode_slots"), "columns": _lib.fn("qb_dev_encode_messages"),
           "list": _lib.fn("qb_dev_encode_msg_out")}
    work = {"slots": (S, lambda o: qe.encode_slots(groups, cols={"commit": hb_commit, "ctx_g": hb_ctx},
                                                   out=o)),
            "columns": (M, lambda o: qe.encode_columns(col_b, out=o)),
            "list": (M, lambda o: qe.encode_msg_out(groups, msgs, M, total, out=o))}

    def caller(name, out, Mn):
        """The checked wrapper once, then the same call through ctypes alone."""
        work[name][1](out)
        ws = out._ws if name == "columns" else groups._ws
        oc = qe._out_struct(out, Mn)
        eg = groups.struct()
        if name == "slots":
            sc = qe.EncodeSlotColsC(S=S, gflags=None, gmask=0xFF, type_all=qe.MSG_HEARTBEAT,
                                    commit=hb_commit.data_ptr(), ctx_g=hb_ctx.data_ptr())
            args = (C.byref(eg), C.byref(sc), C.byref(oc))
        elif name == "columns":
            cc = qe.EncodeColsC(**{k: v.data_ptr() for k, v in col_b.items()})
            args = (Mn, C.byref(cc), C.byref(oc))
        else:
            args = (C.byref(eg), msgs.data_ptr(), Mn, total.data_ptr(), C.byref(oc))
        keep = (oc, eg, args, ws)
        return lambda: _lib.check(fns[name](*keep[2], ws.data_ptr(), ws.numel(), sp), name), keep

    def timed(call):
        def sample(ev):
            torch.cuda.synchronize()
            ev.record(ev.ev[0], sp)
            call()
            ev.record(ev.ev[1], sp)
            torch.cuda.synchronize()
            return ev.elapsed_ms(0, 1) / 1e3
        ev = HipEvents(2)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.3:  # warm-up: clocks settle (time_region)
            sample(ev)
        ts = [sample(ev) for _ in range(reps)]
        ev.close()
        return float(np.median(ts))

    # Bytes per message, the columns the launches touch (not a traffic counter).
    # Every form: the length written and read by the scan's three launches 20,
    # the offset read twice (p, q share lines: 4), msg_off 8, status 1, ent_at 4
    # and the message's own bytes.  Slots: the slot's group written 4 and read
    # twice 8, ids and commit read twice 32, per group (a fifth each) off,
    # self_id, term, ctx read twice 11.2.  Columns: type 1, five u64 and reject
    # 41, read twice.  List: the 40-byte record twice, the group's off / ids /
    # self_id / term gathered twice 64.
    fixed = 20 + 4 + 8 + 1 + 4
    read_b = {"slots": 4 + 8 + 32 + 11.2, "columns": 2 * 42, "list": 2 * 40 + 64}
    rows, keepers, outs = {}, [], {}
    for name, (Mn, _) in work.items():
        out = qe.new_out(Mn, dev, cap=Mn * 64)
        call, keep = caller(name, out, Mn)
        keepers.append(keep)
        out.stats.zero_()
        tm = timed(call)
        torch.cuda.synchronize()
        nb = int(out.nbytes[0])
        written = int((out.status[:Mn] <= 1).sum())
        b = Mn * (fixed + read_b[name]) + nb
        rows[name] = {"messages": Mn, "written": written, "us": tm * 1e6, "out_bytes": nb,
                      "bytes_per_message": b / Mn, "TBs": b / tm / 1e12,
                      "frac": b / tm / 1e9 / HBM_PEAK_GBS}
        outs[name] = out

    # ---- the decode-side yardstick: the ingest over (b)'s bytes ----
    ob = outs["columns"]
    nbb = int(ob.nbytes[0])
    grp32 = gm.to(torch.int32)
    t_in = timed(lambda: wire.ingest(ob.bytes, nbb, ob.msg_off, grp32, off, ids))
    in_b = nbb + M * (8 + 4 + 40) + M * (4 + 1 + 32 + 1 + 1)
    rows["ingest"] = {"messages": M, "us": t_in * 1e6, "bytes_per_message": in_b / M,
                      "TBs": in_b / t_in / 1e12, "frac": in_b / t_in / 1e9 / HBM_PEAK_GBS}

    # ---- parity at this size: every 1024th message of each workload ----
    h = lambda t: t.cpu().numpy()  # noqa: E731
    u = lambda t: h(t).view(np.uint64)  # noqa: E731
    ok, detail = True, {}
    for name, (Mn, _) in work.items():
        o = outs[name]
        sub = np.arange(0, Mn, 1024)
        offs, st = u(o.msg_off), h(o.status)
        at, by = h(o.ent_at).view(np.uint32), h(o.bytes)
        if name == "slots":
            sg = sub // n
            cg, cx = u(self_id), u(hb_ctx)
            iu, tu, hc = u(ids), u(term), u(hb_commit)
            want = [(E.NONE, None) if iu[s] == cg[g] else
                    E.form(int(cg[g]), int(tu[g]), E.MSG_HEARTBEAT, int(iu[s]), 0, 0, int(hc[s]), 0,
                           int(cx[g])) for s, g in zip(sub, sg)]
        elif name == "columns":
            cb = {k: (h(v) if v.dtype == torch.uint8 else u(v))[sub] for k, v in col_b.items()}
            want = E.columns(cb, len(sub))
        else:
            want = E.msg_out(G, h(off).view(np.uint32), u(ids), u(self_id), u(term), recs[sub],
                             len(sub), None)
        good = 0
        for j, i in enumerate(sub):
            code, m = want[j]
            b = by[int(offs[i]):int(offs[i + 1])].tobytes()
            if code <= E.ENTRIES:
                good += (st[i] == code and b == E.marshal(m) and at[i] == E.ent_at(m))
            else:
                good += (st[i] == code and b == b"")
        stats = o.stats_dict()
        counted = sum(stats.values()) == (reps + 1) * Mn or sum(stats.values()) % Mn == 0
        ok = ok and good == len(sub) and counted and int(offs[Mn]) == int(o.nbytes[0])
        detail[name] = f"{good}/{len(sub)}"
    extra = {"unit": "messages/s", "samples": reps,
             "timing": "one HIP event pair per call, median over the samples after warm-up",
             **{f"{k}_{f}": v for k, r in rows.items() for f, v in r.items()},
             "parity": bool(ok),
             "parity_check": f"tests/encode_ref.py over every 1024th message (bytes, msg_off, "
                             f"status, ent_at): {detail}"}
    r = rows["slots"]
    reporter("encode (heartbeats of every group through the slot form)", r["messages"],
             r["us"] / 1e6, r["messages"] * r["bytes_per_message"], extra)
    assert ok, "encode parity failed"


def follower_wire_config(M, reps, *, reporter=None):
    """The follower's wire ingest (qb_dev_ingest_follower), three workloads:
    (a) M heartbeats with the bytes qb_dev_encode_slots writes (encoded on the
    device through the general columns, one in ten with a read context); (b) M
    MsgApp with no entries; (c) M / 4 MsgApp of 4 entries in 1-2 term runs
    with 64-byte Data (fixed layout, built on the device).  Beside them, in
    the same session, qb_dev_ingest_messages_rows over M MsgAppResp.  One HIP
    event pair per call, median over the samples after warm-up; calls straight
    to the C ABI.  Parity at this size: tests/follower_wire_ref.py over every
    1024th message of each workload — every column, the entry range, the runs —
    and the batch's counters."""
    reporter = reporter or report
    import ctypes as C
    import time
    from etcd_amd import _lib
    from etcd_amd.quorum import encode as qe, wire
    from tests import follower_wire_ref as FW
    G = 1 << 22
    sp = torch.cuda.current_stream(dev).cuda_stream
    ar = lambda k: torch.arange(k, dtype=torch.int64, device=dev)  # noqa: E731
    gen = torch.Generator(device=dev).manual_seed(0xF0110)
    rnd = lambda k, hi: torch.randint(0, hi, (k,), generator=gen, dtype=torch.int64, device=dev)  # noqa: E731
    u8 = lambda k, v: torch.full((k,), v, dtype=torch.uint8, device=dev)  # noqa: E731

    def fields(Mn):
        gm = rnd(Mn, G)
        return gm, {"to": 16384 + (1 + rnd(Mn, 4)) * 200000 + gm % 100000, "from": 16384 + gm % 100000,
                    "term": torch.full((Mn,), 20000, dtype=torch.int64, device=dev),
                    "commit": (1 << 35) + gm * 64 + rnd(Mn, 64)}

    def columns(cols, Mn):
        b, moff, st, _, nb = qe.encode_columns(cols, M=Mn)
        torch.cuda.synchronize()
        assert int(st.max()) == qe.ENC_OK
        return b, int(nb[0]), moff

    work = {}
    gm, f = fields(M)
    f["type"] = u8(M, 8)
    f["context"] = torch.where(rnd(M, 10) == 0, (1 << 56) + rnd(M, 1 << 40) + 1, torch.zeros_like(gm))
    work["heartbeats"] = (M, gm.to(torch.int32), *columns(f, M), 0)
    gm, f = fields(M)
    f["type"], f["log_term"], f["index"] = u8(M, 3), f["term"] - 1, f["commit"] + 64
    work["app_empty"] = (M, gm.to(torch.int32), *columns(f, M), 0)
    # (c): fixed layout — type 3, to / from / term / logTerm of 3 varint bytes,
    # index and commit of 6, 4 entries of 79 bytes (Type 0, Term 3, Index 6,
    # 64-byte Data), the empty Snapshot, Reject 0, RejectHint 0
    Mc = M // 4
    gm, f = fields(Mc)
    index = f["commit"] + 64
    split = 1 + rnd(Mc, 4)  # entries behind `split` carry term + 1: 4 gives one run
    lay = [0x08, 3, 0x10, ("v", f["to"], 3), 0x18, ("v", f["from"], 3), 0x20, ("v", f["term"], 3),
           0x28, ("v", f["term"] - 1, 3), 0x30, ("v", index, 6)]
    for k in range(4):
        lay += [0x3A, 79, 0x08, 0, 0x10, ("v", f["term"] - 1 + (split <= k).to(torch.int64), 3),
                0x18, ("v", index + 1 + k, 6), 0x22, 64] + [0x61 + k] * 64
    lay += [0x40, ("v", f["commit"], 6), 0x4A, len(wire._EMPTY_SNAPSHOT)] + list(wire._EMPTY_SNAPSHOT)
    lay += [0x50, 0, 0x58, 0]
    L = sum(x[2] if isinstance(x, tuple) else 1 for x in lay)
    buf = torch.empty((Mc, L), dtype=torch.uint8, device=dev)
    c = 0
    for x in lay:
        if isinstance(x, tuple):
            for col in wire._dev_varint(x[1], x[2]):
                buf[:, c] = col
                c += 1
        else:
            buf[:, c] = x
            c += 1
    work["app_entries"] = (Mc, gm.to(torch.int32), buf.reshape(-1), Mc * L, ar(Mc + 1) * L, 2 * Mc)
    runs_c = int((split < 4).sum()) + Mc

    def timed(call):
        def sample(ev):
            torch.cuda.synchronize()
            ev.record(ev.ev[0], sp)
            call()
            ev.record(ev.ev[1], sp)
            torch.cuda.synchronize()
            return ev.elapsed_ms(0, 1) / 1e3
        ev = HipEvents(2)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.3:  # warm-up: clocks settle (time_region)
            sample(ev)
        ts = [sample(ev) for _ in range(reps)]
        ev.close()
        return float(np.median(ts))

    # Bytes per message, the columns the launches touch (not a traffic counter):
    # msg_off 8 and msg_group 4 read; pass 1 writes group 4, flags 1, from / term
    # / index / aux / commit 40, status 1, msg_type 1, ent_pos 8, ent_bytes 4,
    # ent_n 4 and the run count 4 = 67; the scan reads and writes ent_off twice
    # 16; pass 2 reads status 1 and two offsets 8; plus the message's own bytes
    # (read once; the entries' keys and varints a second time by pass 2) and 12
    # per run written.
    fixed = 12 + 67 + 16 + 9
    fn = _lib.fn("qb_dev_ingest_follower")
    need = int(_lib.fn("qb_wire_follower_scratch_bytes")(M))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    stats = torch.zeros(len(wire.WIRE_FOLLOWER_STAT_NAMES), dtype=torch.int64, device=dev)
    h = lambda t: t.cpu().numpy()  # noqa: E731
    u = lambda t: h(t).view(np.uint64)  # noqa: E731
    rows, ok, detail = {}, True, {}
    for name, (Mn, grp, b, nb, moff, cap) in work.items():
        o = wire.new_follower_out(Mn, cap, dev)
        ib, app = o.inbox, o.app
        oc = wire.FollowerWireOutC(ib.group.data_ptr(), ib.flags.data_ptr(), ib.frm.data_ptr(),
                                   ib.term.data_ptr(), ib.index.data_ptr(), ib.aux.data_ptr(),
                                   app.commit.data_ptr(), o.status.data_ptr(), o.msg_type.data_ptr(),
                                   o.ent_pos.data_ptr(), o.ent_bytes.data_ptr(), o.ent_n.data_ptr(),
                                   app.ent_off.data_ptr(), app.ent_term.data_ptr(),
                                   app.ent_len.data_ptr(), cap, o.ent_total.data_ptr(), stats.data_ptr())
        call = lambda: _lib.check(fn(Mn, b.data_ptr(), nb, moff.data_ptr(), grp.data_ptr(), G,  # noqa: E731,B023
                                     C.byref(oc), ws.data_ptr(), need, sp), "qb_dev_ingest_follower")  # noqa: B023
        stats.zero_()
        tm = timed(call)
        torch.cuda.synchronize()
        total = int(o.ent_total[0])
        by = Mn * fixed + nb + 12 * total
        rows[name] = {"messages": Mn, "us": tm * 1e6, "in_bytes": nb, "runs": total,
                      "bytes_per_message": by / Mn, "TBs": by / tm / 1e12,
                      "frac": by / tm / 1e9 / HBM_PEAK_GBS}
        # ---- parity: every 1024th message against the restatement ----
        sub = np.arange(0, Mn, 1024)
        offs, gh = u(moff), h(grp).view(np.uint32)
        idx = torch.from_numpy(sub).to(dev)
        start = moff[idx]
        lens = moff[idx + 1] - start
        so = torch.zeros(len(sub) + 1, dtype=torch.int64, device=dev)
        so[1:] = torch.cumsum(lens, 0)
        src = torch.repeat_interleave(start - so[:-1], lens) + ar(int(so[-1]))
        raw, so = h(b[src]).tobytes(), h(so)
        got = {"group": h(ib.group).view(np.uint32), "flags": h(ib.flags), "frm": u(ib.frm),
               "term": u(ib.term), "index": u(ib.index), "aux": u(ib.aux), "commit": u(app.commit),
               "status": h(o.status), "msg_type": h(o.msg_type), "ent_pos": u(o.ent_pos),
               "ent_bytes": h(o.ent_bytes).view(np.uint32), "ent_n": h(o.ent_n).view(np.uint32)}
        eo, et, el = h(app.ent_off).view(np.uint32), u(app.ent_term), h(app.ent_len).view(np.uint32)
        good = 0
        for j, i in enumerate(sub):
            w = FW.decode(raw[so[j]:so[j + 1]], int(gh[i]))
            if w["ent_bytes"]:
                w["ent_pos"] += int(offs[i])
            same = all(int(got[k][i]) == w[k] for k, _ in FW.COLUMNS)
            a, z = int(eo[i]), int(eo[i + 1])
            good += same and list(zip(et[a:z].tolist(), el[a:z].tolist())) == w["runs"]
        st = h(stats).view(np.uint64)
        counted = int(st.sum()) % Mn == 0 and int(st[FW.OK]) == int(st.sum())
        want_total = {"heartbeats": 0, "app_empty": 0, "app_entries": runs_c}[name]
        ok = ok and good == len(sub) and counted and total == want_total == int(eo[Mn])
        detail[name] = f"{good}/{len(sub)}"

    # ---- the leader's ingest over the same count of MsgAppResp, same session ----
    gm = rnd(M, G)
    n = 5
    gg, ss = ar(G).repeat_interleave(n), ar(n).repeat(G)
    ids = 16384 + ss * 200000 + gg % 100000
    off = (ar(G + 1) * n).to(torch.int32)
    bb, nbb, mo = wire.encode_appresp(16384 + gm % 100000, 16384 + (1 + rnd(M, 4)) * 200000 + gm % 100000,
                                      torch.full((M,), 20000, dtype=torch.int64, device=dev),
                                      (1 << 35) + gm * 64 + rnd(M, 64), (rnd(M, 10) == 0).to(torch.uint8))
    grows = wire.group_rows(off, ids)
    g32 = gm.to(torch.int32)
    t_in = timed(lambda: wire.ingest(bb, nbb, mo, g32, off, ids, rows=grows))
    in_b = nbb + M * (8 + 4 + 64) + M * (4 + 1 + 32 + 1 + 1)
    rows["ingest_rows"] = {"messages": M, "us": t_in * 1e6, "bytes_per_message": in_b / M,
                           "TBs": in_b / t_in / 1e12, "frac": in_b / t_in / 1e9 / HBM_PEAK_GBS}
    extra = {"unit": "messages/s", "samples": reps,
             "timing": "one HIP event pair per call, median over the samples after warm-up",
             **{f"{k}_{f}": v for k, r in rows.items() for f, v in r.items()},
             "parity": bool(ok),
             "parity_check": f"tests/follower_wire_ref.py over every 1024th message (every column, "
                             f"the entry range, the runs): {detail}"}
    r = rows["heartbeats"]
    reporter("follower wire ingest (heartbeats as the slot form writes them)", r["messages"],
             r["us"] / 1e6, r["messages"] * r["bytes_per_message"], extra)
    assert ok, "follower wire parity failed"


def request_wire_config(G, reps, *, reporter=None):
    """The requests' wire ingest (qb_dev_ingest_requests) over G groups of
    five voters, max_reads 4, concat on, three samples: (a) one batch of 2^20
    messages — 70 % single-entry MsgProp with a 64-byte payload, 25 %
    MsgReadIndex, 5 % MsgTransferLeader and MsgReadIndexResp — to random
    groups; (b) the same mixture for G / 100 messages; (c) an idle call, M = 0.
    Beside (a) and (b), in the same session, qb_dev_ingest_follower over the
    same bytes (its kernels are the parent's, unchanged: every message decodes
    and comes out QB_WIRE_TYPE), the nearest existing kernel of the same
    shape.  One HIP event pair per call, median over the samples after warm-up;
    calls straight to the C ABI.  Parity: tests/request_wire_ref.py's pass 1
    over every 1024th message, and the counters' sums."""
    reporter = reporter or report
    import ctypes as C
    import time
    from etcd_amd import _lib
    from etcd_amd.quorum import wire
    from tests import request_wire_ref as RW
    sp = torch.cuda.current_stream(dev).cuda_stream
    n, R = 5, 4
    ar = lambda k: torch.arange(k, dtype=torch.int64, device=dev)  # noqa: E731
    gg, ss = ar(G).repeat_interleave(n), ar(n).repeat(G)
    ids = 16384 + ss * 200000 + gg % 100000
    off = (ar(G + 1) * n).to(torch.int32)
    snap = [0x4A, len(wire._EMPTY_SNAPSHOT)] + list(wire._EMPTY_SNAPSHOT) + [0x50, 0, 0x58, 0]

    def batch(M, seed):
        """Host bytes of M messages in four fixed layouts, scattered in order."""
        rng = np.random.default_rng(seed)
        grp = rng.integers(0, G, M).astype(np.uint32)
        g64 = grp.astype(np.uint64)
        frm = np.uint64(16384) + rng.integers(1, n, M).astype(np.uint64) * np.uint64(200000) + \
            g64 % np.uint64(100000)
        to = np.uint64(16384) + g64 % np.uint64(100000)
        ctx = (np.uint64(1) << np.uint64(56)) + rng.integers(1, 1 << 40, M).astype(np.uint64)
        ctxb = ((ctx[:, None] >> (np.arange(7, -1, -1, dtype=np.uint64) * np.uint64(8)))
                & np.uint64(0xFF)).astype(np.uint8)
        u = rng.random(M)
        cls = np.where(u < 0.70, 0, np.where(u < 0.95, 1, np.where(u < 0.975, 2, 3)))
        col = lambda b: np.full((M, 1), b, np.uint8)  # noqa: E731
        cols = lambda bs: [col(b) for b in bs]  # noqa: E731
        head = lambda t, term, index: [col(0x08), col(t), col(0x10), wire._vfix(to, 3), col(0x18),  # noqa: E731
                                       wire._vfix(frm, 3), col(0x20), *term, col(0x28), col(0),
                                       col(0x30), *index]
        ent8 = cols([0x3A, 16, 0x08, 0, 0x10, 0, 0x18, 0, 0x22, 8]) + [ctxb]
        lay = [head(2, [col(0)], [col(0)]) + cols([0x3A, 72, 0x08, 0, 0x10, 0, 0x18, 0, 0x22, 64]) +
               [np.tile(np.arange(64, dtype=np.uint8) + 0x30, (M, 1))] + cols([0x40, 0] + snap),
               head(15, [col(0)], [col(0)]) + ent8 + cols([0x40, 0] + snap),
               head(13, [wire._vfix(np.full(M, 20000, np.uint64), 3)], [col(0)]) + cols([0x40, 0] + snap),
               head(16, [wire._vfix(np.full(M, 20000, np.uint64), 3)],
                    [wire._vfix(np.uint64(1 << 35) + g64, 6)]) + ent8 + cols([0x40, 0] + snap)]
        lay = [np.concatenate(x, axis=1) for x in lay]
        lens = np.array([x.shape[1] for x in lay], np.uint64)[cls]
        moff = np.zeros(M + 1, np.uint64)
        np.cumsum(lens, out=moff[1:])
        buf = np.empty(int(moff[-1]), np.uint8)
        for k, t in enumerate(lay):
            pos = moff[:-1][cls == k].astype(np.int64)
            buf[(pos[:, None] + np.arange(t.shape[1])).reshape(-1)] = t[cls == k].reshape(-1)
        return buf, moff, grp

    def timed(call):
        def sample(ev):
            torch.cuda.synchronize()
            ev.record(ev.ev[0], sp)
            call()
            ev.record(ev.ev[1], sp)
            torch.cuda.synchronize()
            return ev.elapsed_ms(0, 1) / 1e3
        ev = HipEvents(2)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.3:  # warm-up: clocks settle (time_region)
            sample(ev)
        ts = [sample(ev) for _ in range(reps)]
        ev.close()
        return float(np.median(ts))

    # Bytes a call must move (the columns the launches touch, not a traffic
    # counter).  Per group: the zeroed count 4, the scan's two passes over it
    # 16 (none with M = 0), pass 2's count read 4 and the nine dense defaults
    # 36.  Per message: msg_off 8 and msg_group 4 read, its own bytes, the
    # eighteen columns 82 and the count 4 (pass 1); status, kind, group 6 read
    # and the index 4 written (scatter); the index 4 and the kind 1 read
    # (pass 2), and what its kind takes from its columns and puts into the
    # dense ones: a read 9 + 9 + 1, a proposal 24 + 4, a transfer 9.
    PER_GROUP_IDLE, PER_GROUP, PER_MSG = 4 + 4 + 36, 4 + 16 + 4 + 36, 12 + 82 + 4 + 10 + 5
    fn = _lib.fn("qb_dev_ingest_requests")
    ffn = _lib.fn("qb_dev_ingest_follower")
    stats = torch.zeros(len(wire.WIRE_REQUEST_STAT_NAMES), dtype=torch.int64, device=dev)
    h = lambda t: t.cpu().numpy()  # noqa: E731
    rows, ok, detail = {}, True, {}
    for name, M in (("batch_1M", 1 << 20), ("one_percent", G // 100), ("idle", 0)):
        buf, moff, grp = batch(max(M, 1), 0xBEEF + M)
        if M == 0:
            buf, moff, grp = buf[:1], moff[:1], grp[:0]
        nb = int(moff[-1]) if M else 0
        d_buf = torch.from_numpy(buf).to(dev)
        d_moff = torch.from_numpy(moff.view(np.int64).copy()).to(dev)
        d_grp = torch.from_numpy(np.resize(grp, max(M, 1)).view(np.int32).copy()).to(dev)
        o = wire.new_request_out(M, G, R, dev)
        rin, pin = o.request_in, o.propose_in
        dense = {"n_reads": rin.n_reads, "rd_ctx": rin.rd_ctx, "rd_from": rin.rd_from,
                 "xf_from": rin.xf_from, "xf_term": rin.xf_term, "action": pin.action,
                 "n_ents": pin.n_ents, "g_payload": pin.payload, "g_cc_at": pin.cc_at,
                 "g_cc_payload": pin.cc_payload, "gflags": o.gflags}
        oc = wire.RequestWireOutC(*[getattr(o, "frm" if k == "from" else k).data_ptr() for k, _ in wire._RW_MSG],
                                  *[dense[k].data_ptr() for k, _, _ in wire._RW_DENSE], stats.data_ptr())
        need = int(_lib.fn("qb_wire_requests_scratch_bytes")(G, M))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        call = lambda: _lib.check(fn(M, d_buf.data_ptr(), nb, d_moff.data_ptr(), d_grp.data_ptr(), G,  # noqa: E731,B023
                                     off.data_ptr(), ids.data_ptr(), R, 1, C.byref(oc), ws.data_ptr(),  # noqa: B023
                                     need, sp), "qb_dev_ingest_requests")  # noqa: B023
        tm = timed(call)
        stats.zero_()
        call()
        torch.cuda.synchronize()
        st = h(stats).view(np.uint64)
        taken = 19 * int(st[RW.STAT_TAKEN_READS]) + 28 * int(st[RW.STAT_TAKEN_PROPS]) + \
            9 * int(st[RW.STAT_TAKEN_TRANSFERS])
        by = G * (PER_GROUP if M else PER_GROUP_IDLE) + M * PER_MSG + nb + taken
        rows[name] = {"messages": M, "us": tm * 1e6, "in_bytes": nb, "bytes": by, "TBs": by / tm / 1e12,
                      "frac": by / tm / 1e9 / HBM_PEAK_GBS, "taken_props": int(st[RW.STAT_TAKEN_PROPS]),
                      "taken_reads": int(st[RW.STAT_TAKEN_READS]), "deferred": int(st[RW.DEFERRED])}
        ok = ok and int(st[:10].sum()) == M
        # ---- parity: pass 1 of every 1024th message against the restatement ----
        sub = list(range(0, M, 1024))
        hid = h(ids).view(np.uint64)
        got = {k: h(getattr(o, k)).view(dt) for k, dt in RW.COLUMNS} if M else {}
        good = 0
        for i in sub:
            g = int(grp[i])
            w = RW.decode(buf[int(moff[i]):int(moff[i + 1])].tobytes(), g, G, hid[n * g:n * g + n])
            if w["ent_bytes"]:
                w["ent_pos"] += int(moff[i])
            same = all(int(got[k][i]) == w[k] for k, _ in RW.COLUMNS
                       if k not in ("status", "rd_k", "ent_base"))
            good += same and int(got["status"][i]) in (w["status"], RW.DEFERRED)
        ok = ok and good == len(sub)
        detail[name] = f"{good}/{len(sub)}"
        if M:  # the follower's ingest over the same bytes, same session
            fo = wire.new_follower_out(M, 0, dev)
            ib, app = fo.inbox, fo.app
            fc = wire.FollowerWireOutC(ib.group.data_ptr(), ib.flags.data_ptr(), ib.frm.data_ptr(),
                                       ib.term.data_ptr(), ib.index.data_ptr(), ib.aux.data_ptr(),
                                       app.commit.data_ptr(), fo.status.data_ptr(), fo.msg_type.data_ptr(),
                                       fo.ent_pos.data_ptr(), fo.ent_bytes.data_ptr(), fo.ent_n.data_ptr(),
                                       app.ent_off.data_ptr(), app.ent_term.data_ptr(),
                                       app.ent_len.data_ptr(), 0, fo.ent_total.data_ptr(), None)
            fneed = int(_lib.fn("qb_wire_follower_scratch_bytes")(M))
            fws = torch.empty(max(fneed, 256), dtype=torch.uint8, device=dev)
            tf = timed(lambda: _lib.check(ffn(M, d_buf.data_ptr(), nb, d_moff.data_ptr(), d_grp.data_ptr(),  # noqa: B023
                                              G, C.byref(fc), fws.data_ptr(), fneed, sp),  # noqa: B023
                                          "qb_dev_ingest_follower"))
            fby = M * (12 + 67 + 16 + 9) + nb  # follower_wire_config's count, no runs
            rows[name].update(follower_us=tf * 1e6, follower_bytes=fby, follower_TBs=fby / tf / 1e12)
    extra = {"unit": "messages/s", "samples": reps, "groups": G, "max_reads": R, "concat": 1,
             "timing": "one HIP event pair per call, median over the samples after warm-up",
             **{f"{k}_{f}": v for k, r in rows.items() for f, v in r.items()},
             "parity": bool(ok),
             "parity_check": f"tests/request_wire_ref.py pass 1 over every 1024th message, and the "
                             f"status counters' sum: {detail}"}
    r = rows["batch_1M"]
    reporter("request wire ingest (2^20 messages: 70 % MsgProp, 25 % MsgReadIndex)", r["messages"],
             r["us"] / 1e6, r["bytes"], extra)
    assert ok, "request wire parity failed"


def log_compact_config(G, reps, *, reporter=None):
    """The batched CreateSnapshot / Compact (qb_dev_log_compact, explicit mode)
    over G groups.  The call reads no per-slot state, so the voter count of the
    ready row's five-voter table does not enter; the logs are built here: group
    g holds n = 1 + g % 8 runs of four entries from the dummy entry at index 0,
    everything stable and applied, no snapshot yet.  Three samples: no group
    acting (both request columns zero), every 100th group acting, and every
    group acting — a snapshot at last_index and a compaction at the second
    entry of run k, k = (g // 8) % n, so k is spread over 0..7.  One HIP event
    pair per call, median over the samples after warm-up; the columns the call
    writes are put back between samples outside the timed call; calls straight
    to the C ABI.  Bytes: the loads and stores the two kernels issue, summed
    over the groups of the sample (not a traffic counter).  Parity: behind a
    dense sample every written column of all G groups against its closed form,
    and every 1024th group against tests/compact_ref.py."""
    reporter = reporter or report
    import ctypes as C
    import time
    from etcd_amd import _lib
    from etcd_amd.quorum import compact as qcm
    from etcd_amd.quorum._dev import to_np
    from etcd_amd.quorum.follower import MAX_RUNS, FollowerLog
    from etcd_amd.quorum.ready import ReadyState
    from tests import compact_pack as P, compact_ref as R
    g = torch.arange(G, dtype=torch.int64, device=dev)
    n = 1 + g % 8
    q = torch.arange(MAX_RUNS, dtype=torch.int64, device=dev)[:, None]
    live = q < n[None, :]
    run_start = torch.where(live, 4 * q, torch.zeros_like(q)).expand(MAX_RUNS, G).contiguous().view(-1)
    run_term = torch.where(live, q + 1, torch.zeros_like(q)).expand(MAX_RUNS, G).contiguous().view(-1)
    last = 4 * n - 1
    k = (g // 8) % n
    state = {"first_index": torch.ones_like(g), "snap_index": torch.zeros_like(g),
             "snap_term": torch.zeros_like(g), "meta": (n << 16).to(torch.int32) | 0x0300,
             "run_start": run_start, "run_term": run_term}
    saved = {key: v.clone() for key, v in state.items()}
    log = FollowerLog(G, state["meta"], state["first_index"], state["run_start"], state["run_term"])
    rdy = ReadyState(G, {"last_index": last, "applied": last.clone(), "unstable_offset": last + 1,
                         "usnap_index": torch.zeros_like(g)})
    snap_at, compact_at = torch.zeros_like(g), torch.zeros_like(g)
    req = qcm.CompactRequest.explicit(snap_at, compact_at)
    out = qcm.new_compact_result(G, G, dev)
    qcm.log_compact(log, rdy, state["snap_index"], state["snap_term"], req, out=out)  # (checks, workspace)
    out.stats.zero_()
    cg = qcm.CompactGroupsC(G=G, first_index=state["first_index"].data_ptr(),
                            snap_index=state["snap_index"].data_ptr(),
                            snap_term=state["snap_term"].data_ptr(), meta=state["meta"].data_ptr(),
                            run_start=state["run_start"].data_ptr(),
                            run_term=state["run_term"].data_ptr(),
                            **{key: rdy.t[key].data_ptr() for key in rdy.t})
    ci = req.struct()
    co = qcm.CompactOutC(cmflags=out.cmflags.data_ptr(), list_count=out.list_count.data_ptr(),
                         **{key: out.cols[key].data_ptr() for key in qcm._LIST})
    sp = torch.cuda.current_stream(dev).cuda_stream
    f_compact = _lib.fn("qb_dev_log_compact")
    ws = out._ws

    def call():
        _lib.check(f_compact(C.byref(cg), C.byref(ci), G, C.byref(co), out.stats.data_ptr(),
                             ws.data_ptr(), ws.numel(), sp), "qb_dev_log_compact")

    def restore():
        for key, v in saved.items():
            state[key].copy_(v)

    def timed(every):
        on = (g % every == 0) if every else torch.zeros_like(g, dtype=torch.bool)
        snap_at.copy_(torch.where(on, last, torch.zeros_like(g)))
        compact_at.copy_(torch.where(on, 4 * k + 1, torch.zeros_like(g)))
        Rn = int(on.sum().item())

        def sample(ev):
            restore()
            torch.cuda.synchronize()
            ev.record(ev.ev[0], sp)
            call()
            ev.record(ev.ev[1], sp)
            torch.cuda.synchronize()
            return ev.elapsed_ms(0, 1) / 1e3
        ev = HipEvents(2)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.3:  # warm-up: clocks settle (time_region)
            sample(ev)
        out.stats.zero_()
        per = [sample(ev) for _ in range(reps)]
        ev.close()
        st = out.stats_dict()
        assert int(out.list_count.cpu()[0]) == Rn, (every, Rn)
        assert st["snapped"] == st["compacted"] == st["listed"] == reps * Rn, st
        assert st["runs_dropped"] == reps * int(k[on].sum().item()), st
        # C1: the two request columns read, cmflags written; an acting group's
        # six cursor words.  C2: cmflags read; per listed group the request 16,
        # first_index 8 and meta 4 read, n rows of 16 read, the snapshot 16, the
        # kept rows (16 each; with k == 0 row 0's start alone), meta 4 (when the
        # count moves) and first_index 8 written, the record 46.
        nk = (n - k)[on]
        rows_w = torch.where(k[on] == 0, torch.full_like(nk, 8), 16 * nk)
        b = G * (16 + 2 + 2) + Rn * (48 + 28 + 16 + 8 + 46) + int((16 * n[on]).sum().item()) + int(
            rows_w.sum().item()) + 4 * int((k[on] != 0).sum().item())
        return float(np.median(per)), Rn, b

    rows = {}
    for name, every in (("idle", 0), ("one_percent", 100), ("dense", 1)):
        t, Rn, b = timed(every)
        rows[name] = {"acting_groups": Rn, "us": t * 1e6, "bytes": b, "bytes_per_group": b / G,
                      "TBs": b / t / 1e12, "frac": b / t / 1e9 / HBM_PEAK_GBS}

    # ---- parity behind the dense sample ---------------------------------
    c = 4 * k + 1
    assert bool((state["first_index"] == c + 1).all()) and bool((state["snap_index"] == last).all())
    assert bool((state["snap_term"] == n).all())
    assert bool((state["meta"] == (((n - k) << 16).to(torch.int32) | 0x0300)).all())
    rs, rt = state["run_start"].view(MAX_RUNS, G), state["run_term"].view(MAX_RUNS, G)
    kept = q < (n - k)[None, :]
    want_rs = torch.where(q == 0, c[None, :], 4 * (q + k[None, :]))
    assert bool((rs == torch.where(kept, want_rs, saved["run_start"].view(MAX_RUNS, G))).all())
    assert bool((rt == torch.where(kept, q + k[None, :] + 1, saved["run_term"].view(MAX_RUNS, G))).all())
    assert bool((out.cols["gid"] == g.to(torch.int32)).all())
    assert bool((out.cols["compact_index"] == c).all()) and bool((out.cols["first_before"] == 1).all())
    pick = torch.arange(0, G, 1024, device=dev)
    cols = {"first_index": state["first_index"], "snap_index": state["snap_index"],
            "snap_term": state["snap_term"], "meta": state["meta"], **rdy.t}
    got = {key: to_np(cols[key][pick], P.STATE[key]) for key in cols}
    got["run_start"], got["run_term"] = (to_np(x[:, pick].contiguous(), np.uint64) for x in (rs, rt))
    before = {key: to_np(saved[key][pick], P.STATE[key]) for key in ("first_index", "snap_index",
                                                                      "snap_term", "meta")}
    before["run_start"], before["run_term"] = (
        to_np(saved[key].view(MAX_RUNS, G)[:, pick].contiguous(), np.uint64)
        for key in ("run_start", "run_term"))
    before.update({key: got[key] for key in rdy.t})
    nodes = P.unpack_nodes(before)
    ref = R.log_compact(nodes, R.Request(R.CM_EXPLICIT, snap_at=to_np(last[pick], np.uint64),
                                         compact_at=to_np(c[pick], np.uint64)), len(nodes),
                        R.new_stats())
    want = P.pack_nodes(nodes, base=before)
    assert all(f == (R.SNAPPED | R.COMPACTED) for f in ref.flags)
    for key in P.STATE:
        assert np.array_equal(got[key].reshape(-1), want[key].reshape(-1)), key
    d = rows["dense"]
    reporter("log_compact", G, d["us"] / 1e6, d["bytes"],
             {"unit": "groups/s", "samples": reps,
              "timing": "one HIP event pair around qb_dev_log_compact, median over the samples; "
                        "per_launch_us is the dense sample",
              "parity": "all groups against the closed form, every 1024th against compact_ref",
              **{f"{name}_{f}": v for name, r in rows.items() for f, v in r.items()}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="3,4,5")
    ap.add_argument("--gpu-only", action="store_true",
                    help="leader, wire, confchange: skip the CPU baseline (A/B)")
    ap.add_argument("--lab-lib", default=None,
                    help="A/B runs: bind this libquorumbatch.so build (etcd_amd._lib.use_lab_library)")
    a = ap.parse_args()
    if a.lab_lib:
        from etcd_amd import _lib
        _lib.use_lab_library(a.lab_lib)
    global GPU_ONLY
    GPU_ONLY = a.gpu_only
    which = set(a.only.split(","))
    if "1" in which:
        plumbing_config(a.reps)
    if "3" in which:
        csr_config("ragged", 1 << 24, a.reps)
    if "4" in which:
        csr_config("joint", 1 << 23, a.reps)
    if "5" in which:
        tracker_config(1 << 24, a.reps)
    if "leader" in which:
        leader_config(1 << 22, a.reps)
    if "leader-sorted" in which:  # development: records already in group order
        leader_config(1 << 22, a.reps, shuffle=False)
    if "wire" in which:  # with the group-row table (the configuration-time cache)
        wire_config(1 << 24, a.reps, rows=True)
    if "wire-csr" in which:  # gathering off + ids per message
        wire_config(1 << 24, a.reps)
    if "wire-g4k" in which:  # development: 4096 groups (group rows cache-resident)
        wire_config(1 << 24, a.reps, G=4096)
    if "readindex" in which:
        readindex_config(1 << 22, a.reps)
    if "confchange" in which:
        confchange_config(1 << 23, a.reps)
    if "tick" in which:
        tick_config(1 << 22, a.reps)
    if "follower" in which:
        follower_config(1 << 22, a.reps)
    if "follower-log" in which:
        follower_log_config(1 << 22, a.reps)
    if "campaign" in which:
        campaign_config(1 << 22, a.reps)
    if "propose" in which:
        propose_config(1 << 22, a.reps)
    if "switch-config" in which:
        switch_config_row(1 << 22, a.reps)
    if "requests" in which:
        requests_config(1 << 22, a.reps)
    if "ready" in which:
        ready_config(1 << 22, a.reps)
    if "snapshot" in which:
        snapshot_config(1 << 22, a.reps)
    if "log-compact" in which:
        log_compact_config(1 << 22, a.reps)
    if "wire-requests" in which:
        request_wire_config(1 << 22, a.reps)
    if "encode" in which:
        encode_config(1 << 22, a.reps)
    if "follower-wire" in which:
        follower_wire_config(1 << 24, a.reps)
    if "wire-tracker" in which:
        wire_tracker_config(1 << 24, a.reps)
    if "wire-tracker-fused" in which:  # development A/B: the one call alone
        wire_tracker_config(1 << 24, a.reps, fused_only=True)
    if "wire-tracker-csr" in which:  # the composed tick over configs[2]'s ragged CSR groups
        wire_tracker_config(1 << 24, a.reps, csr=True)


if __name__ == "__main__":
    main()
