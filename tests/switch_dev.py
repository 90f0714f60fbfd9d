"""A packed switch-config batch (tests/switch_pack.py) on the device beside
its reference copy: the objects the public wrapper takes, one call, and the
bit-exact comparison of every in/out array, every output (the elements a call
must leave untouched included: they are pre-filled) and every counter.  Test
infrastructure of the GPU tests."""
import copy
import importlib

import numpy as np
import torch

from etcd_amd.quorum import confchange as qcc, leader as ql, switch as qs, tick as qt
from tests import switch_pack as P, switch_ref as R

qc = importlib.import_module("etcd_amd.quorum.campaign")
DEV = "cuda"
FILL_I64 = R.FILL - (1 << 64)
OUT_KEYS = ("swflags", "slot_map", "msg_type", "msg_index", "msg_log_term", "msg_n")


def _dev(x, dt):
    return ql._to_dev(x, dt, torch.device(DEV))


class DeviceRun:
    def __init__(self, a, Q=0, cap=P.INFLIGHT_CAP):
        self.a, self.Q, self.cap = a, Q, cap
        G = self.G = len(a["cfg"])
        S0, S = int(a["old_off"][-1]), int(a["off"][-1])
        self.S0, self.S = S0, S
        # the table as it stood before the change: the old slots (their
        # Progress is not read by the call) and the group words
        arrays = {k: np.zeros(1, dt) for k, dt in ql.GROUP_ARRAYS.items()}
        arrays.update(off=a["old_off"], cfg=np.zeros(G, np.uint32), meta=a["meta"],
                      rq_meta=a["rq_meta"], rq_ctx=np.zeros(max(G * Q, 1), np.uint64),
                      rq_index=np.zeros(max(G * Q, 1), np.uint64))
        for k in ("term", "committed", "first_index", "last_index", "snap_index", "snap_term",
                  "max_ents", "run_start", "run_term"):
            arrays[k] = a[k]
        for k in ("match", "next", "pending_snapshot", "pstate", "infl_pos"):
            arrays[k] = np.zeros(max(S0, 1), ql.GROUP_ARRAYS[k])
        arrays["infl_buf"] = np.zeros(max(S0 * cap, 1), np.uint64)
        self.lg = ql.LeaderGroups(arrays, cap, Q, device=DEV)
        z = np.zeros(G, np.uint32)
        self.state = qt.TickState.from_numpy(a["role"], z, z, z, device=DEV)
        zz = np.zeros(G, np.uint64)
        self.es = qc.ElectionState.for_table(self.lg, self.state, a["self_id"], zz, zz,
                                             a["last_term"], 10, True, True, votes=a["votes"])
        self.old = qcc.ConfigTable(G, S0, cap, {"off": self.lg.t["off"],
                                                "ids": _dev(a["old_ids"], np.uint64)})
        nt = {"off": _dev(a["off"], np.uint32), "cfg": _dev(a["cfg"], np.uint32),
              "ids": _dev(a["ids"], np.uint64), "infl_buf": _dev(a["infl_buf"], np.uint64)}
        for k in ("match", "next", "pending_snapshot", "pstate", "infl_pos"):
            nt[k] = _dev(a[k], qcc.SLOT_ARRAYS[k])
        self.new = qcc.ConfigTable(G, S, cap, nt)
        n, s = max(G, 1), max(S, 1)
        self.out = qs.SwitchResult(
            torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV),
            torch.full((max(S0, 1),), 0xA5, dtype=torch.uint8, device=DEV),
            torch.full((s,), 0xA5, dtype=torch.uint8, device=DEV),
            *[torch.full((s,), FILL_I64, dtype=torch.int64, device=DEV) for _ in range(3)],
            torch.zeros(len(qs.SWSTAT_NAMES), dtype=torch.int64, device=DEV))
        self.ref_out = R.new_out(G, S0, S)
        self.stats = R.new_stats()

    def device_arrays(self):
        G, lg = self.G, self.lg
        got = lg.numpy()
        e = self.es.numpy()
        out = {k: got[k] for k in ("meta", "committed", "match", "next", "pending_snapshot",
                                   "pstate", "infl_pos", "infl_buf", "off", "cfg", "term",
                                   "first_index", "last_index", "snap_index", "snap_term",
                                   "max_ents", "run_start", "run_term")}
        out["rq_meta"] = got["rq_meta"] if self.Q else self.a["rq_meta"]
        out["votes"], out["role"], out["self_id"] = e["votes"], e["role"], e["self_id"]
        out["last_term"] = e["last_term"]
        out["ids"] = ql._to_np(self.new.t["ids"], np.uint64, self.S)
        out["old_ids"] = ql._to_np(self.old.t["ids"], np.uint64, self.S0)
        out["old_off"] = ql._to_np(self.old.t["off"], np.uint32, G + 1)
        return out

    def switch(self, action, where="", expected=None):
        """One call on the device and on the reference copy.  ``expected``:
        (arrays, outputs, stats) behind the call where the caller has them
        already (a batch laid out many times over), instead of the reference
        run."""
        G = self.G
        res = qs.switch_config(self.lg, self.es, self.old, self.new,
                               _dev(action, np.uint8), out=self.out)
        assert res is self.out and self.lg.S == self.S
        if expected is not None:
            self.a, self.ref_out, self.stats = expected
        else:
            self.sent = P.ref_call(self.a, action, self.Q, self.ref_out, self.stats, self.cap)
        got = self.device_arrays()
        for key, g in got.items():
            w = self.a[key][:len(g)]
            assert np.array_equal(g, w), (where, key, np.flatnonzero(g != w)[:8], g[g != w][:8],
                                          w[g != w][:8])
        for key in OUT_KEYS:
            w = self.ref_out[key]
            n = {"swflags": G, "slot_map": self.S0}.get(key, self.S)
            g = ql._to_np(getattr(res, key), w.dtype, n)
            assert np.array_equal(g, w[:n]), (where, key, np.flatnonzero(g != w[:n])[:8],
                                              g[g != w[:n]][:8], w[:n][g != w[:n]][:8])
        assert res.stats_dict() == self.stats, (where, res.stats_dict(), self.stats)
        return self.ref_out["swflags"][:G].copy()


def check_switch(dev=None, G: int = 4096) -> str:
    """The smoke run's family: one seeded batch (pending reads, every role,
    adds, removes, joint configs) through the public wrapper, bit-exact
    against tests/switch_ref.py."""
    a, action = P.random_batch(np.random.default_rng(2024), G, 2)
    run = run_batch(a, action, 2, where="smoke")
    assert run.stats["commits"] and run.stats["probed"] and run.stats["msg_app"], run.stats
    return (f"qb_dev_switch_config {G} groups (meta, votes, pending reads, Progress, rings, "
            f"swflags, slot_map, messages, stats)")


def run_batch(a, action, Q=0, cap=P.INFLIGHT_CAP, where=""):
    run = DeviceRun(copy.deepcopy(a), Q, cap)
    run.switch(action, where)
    return run
