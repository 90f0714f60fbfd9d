"""The smoke run's family of qb_dev_ingest_requests: the 1031-message base of
tests/request_wire_pack.py laid end to end over 4096 groups (copy k's groups
shifted by 257 k, the config tiled), one guarded call through the public
wrapper, every message column, dense column and counter bit-exact against
tests/request_wire_ref.py.  Test infrastructure of the smoke run."""
import numpy as np

from tests import request_wire_pack as P, request_wire_ref as RW


def tiled(G: int):
    """(msgs, groups, (off, ids)) of G // 257 copies of the base over G groups."""
    K = G // P.G
    msgs0, grp0 = P.base_batch()
    goff0, gids0 = P.config()
    sizes = np.tile(np.diff(goff0), K + 1)[:G]
    goff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    gids = np.tile(gids0, K + 1)[:int(goff[-1])]
    grp = [g + P.G * k if g < P.G else G + g - P.G for k in range(K) for g in grp0]
    return list(msgs0) * K, grp, (goff, gids)


def check_request_wire(dev=None, G: int = 4096) -> str:
    assert dev is None or str(dev).startswith(P.DEV)
    msgs, grp, cfg = tiled(G)
    want, _ = P.run(msgs, grp, n_groups=G, max_reads=2, concat=True, cfg=cfg)
    st = want["stats"]
    assert st[RW.STAT_TAKEN_PROPS] and st[RW.STAT_TAKEN_READS] and st[RW.STAT_TAKEN_TRANSFERS], st
    assert st[RW.DEFERRED] and st[RW.CONF_CHANGE] and st[RW.GROUP] and st[RW.STAT_READ_RESPS], st
    return (f"qb_dev_ingest_requests {len(msgs)} messages x {G} groups (message columns, "
            f"qb_request_in, qb_propose_in, gflags, stats)")
