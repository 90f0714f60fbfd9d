// qb_requests.hip — Step(MsgReadIndex) and Step(MsgTransferLeader) for G
// groups at once (qb_dev_leader_requests): stepLeader raft.go:1078-1097 and
// 1339-1370, sendMsgReadIndexResponse raft.go:1827-1843, readOnly.addRequest /
// recvAck read_only.go:56-76, bcastHeartbeatWithCtx raft.go:495-541,
// stepFollower raft.go:1445-1464.  The entry point of the two loops whose
// other halves live in qb_leader.hip, qb_tick.hip, qb_follower.hip and
// qb_campaign.hip.
//
// One kernel in the span-tile shape (qb_span_tile.h):
//   P1  thread per group: the two request bytes first; a group with neither a
//       read nor a transfer writes qflags and xf_type and is done.  An acting
//       group requests all its group words at once (one HBM round trip),
//       applies its reads in k order (the queue's contexts read four at a
//       time; the run table only when committed lies before the last run),
//       then the transfer, whose single sendAppend runs here.  A group that
//       broadcasts claims its slots and leaves committed and its own slot in
//       LDS.
//   P2  (only if a group of the tile broadcasts) match read and hb_commit
//       written.
//
// The per-read outcomes go through a packed per-thread count before the
// BlockTally.
#include "qb_span_tile.h"

namespace qb {
namespace requests {

constexpr u32 kNone = 0xFFFFFFFFu;
constexpr u32 kNoSlot = 0xFFu;
constexpr u32 kReadCodes = QB_RD_BAD;  // rd_status codes 1..11 -> stats 0..10

struct Args {
  qb_request_groups rg;
  qb_request_in in;
  qb_request_out out;
  u64* stats;
};

// The log of one group as term() needs it.
struct Log {
  u64 g, first, last, lastt;
  u32 nruns;
};

struct Tile {
  SpanOwners slots;
  u64 committed[kBlock];
  u8 fl[kBlock];      // non-zero: the group broadcasts
  u8 own[kBlock];      // own slot, 0xFF = the leader has no Progress
  u32 tally[QB_QSTAT_COUNT];
};

// raftLog.term (log.go:268-288) + zeroTermOnErrCompacted.
__device__ __forceinline__ u64 term_at(const Args& A, const Log& l, u64 i) {
  if (i < l.first - 1 || i > l.last) return 0;
  if (i == l.last) return l.lastt;
  return walk_runs(A.rg.run_start, A.rg.run_term, A.rg.G, l.g, i, l.nruns);
}

// term(committed): from the last run's start on it is last_term, and only an
// index before it walks the older runs.
__device__ __forceinline__ u64 term_of_committed(const Args& A, const Log& l, u64 com) {
  if (com < l.first - 1 || com > l.last) return 0;
  if (com == l.last || l.nruns == 1) return l.lastt;
  const u64 lrs = reinterpret_cast<const u64*>(A.rg.run_start)[u64(l.nruns - 1) * A.rg.G + l.g];
  if (com >= lrs) return l.lastt;
  return walk_runs(A.rg.run_start, A.rg.run_term, A.rg.G, l.g, com, l.nruns - 1);
}

// maybeSendAppend on slot i of group l.g, the message to the group's xf_* words.
__device__ __forceinline__ u32 send_slot(const Args& A, const Log& l, u64 ments, u64 i) {
  const u64 nx = reinterpret_cast<const u64*>(A.rg.next)[i];
  return maybe_send_append(A.rg, l.g, i, nx, A.rg.pstate[i], A.rg.infl_pos[i], l.first, l.last,
                           ments, [&] { return term_at(A, l, nx - 1); },
                           reinterpret_cast<u64*>(A.out.xf_index) + l.g,
                           reinterpret_cast<u64*>(A.out.xf_log_term) + l.g,
                           reinterpret_cast<u64*>(A.out.xf_n) + l.g);
}

__global__ __launch_bounds__(kBlock) void k_requests(Args A) {
  __shared__ Tile T;
  const qb_request_groups& rg = A.rg;
  const u64 G = rg.G;
  const u64 ntiles = (G + kBlock - 1) / kBlock;
  const u32 tid = threadIdx.x;
  const u32 cap = rg.readq_cap, maxr = rg.max_reads;
  const bool lease = rg.read_only == QB_READ_ONLY_LEASE_BASED;
  const u64* __restrict__ match = reinterpret_cast<const u64*>(rg.match);
  const u64* __restrict__ rd_ctx = reinterpret_cast<const u64*>(A.in.rd_ctx);
  u64* __restrict__ rd_index = reinterpret_cast<u64*>(A.out.rd_index);
  u64* __restrict__ hb_commit = reinterpret_cast<u64*>(A.out.hb_commit);
  BlockTally<QB_QSTAT_COUNT> tally;
  if (tid < QB_QSTAT_COUNT) T.tally[tid] = 0;
  u32 racc[kReadCodes];  // this thread's reads by outcome, reduced once at the end
#pragma unroll
  for (u32 c = 0; c < kReadCodes; ++c) racc[c] = 0;

  for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    SpanTile S(tile, G);
    const u64 g = S.g0 + tid;
    const bool live = g < G;
    const u32 sb = rg.off[S.g0], se = rg.off[S.gend];  // the tile's span (used in P2 only)

    // ------------------------------------------------------------- P1 ---
    u32 nr = live ? u32(A.in.n_reads[g]) : 0u;
    const u32 xfrom = live ? u32(A.in.xf_from[g]) : kNoSlot;
    const bool badcount = nr > maxr;
    if (badcount) nr = maxr;
    const bool acts = nr != 0 || xfrom != kNoSlot;
    u32 s0 = 0, ns = 0, ls = kNoSlot, xt = 0;
    u64 com = 0;
    u64 packed = 0;  // reads of this tile by outcome, 5 bits each (at most 16 of one)
    u8 qf = badcount ? u8(QB_QFLAG_BAD) : u8(0), fl = 0;
    bool x_started = false, x_aborted = false, x_ignterm = false, x_noprog = false,
         x_learner = false, x_same = false, x_self = false, x_role = false, x_fwd = false,
         x_drop = false, x_host = false;
    if (acts) {
      // every group word of the requests, requested together
      const u8 role = rg.role[g];
      const u32 meta0 = rg.meta[g];
      const u32 cfg = rg.cfg[g];
      s0 = rg.off[g];
      const u32 s1 = rg.off[g + 1];
      const u64 term = reinterpret_cast<const u64*>(rg.term)[g];
      const u64 lead = reinterpret_cast<const u64*>(rg.lead)[g];
      com = reinterpret_cast<const u64*>(rg.committed)[g];
      const u64 mterm = (xfrom != kNoSlot && A.in.xf_term)
                            ? reinterpret_cast<const u64*>(A.in.xf_term)[g] : 0ull;
      const Log lg{g, reinterpret_cast<const u64*>(rg.first_index)[g],
                   reinterpret_cast<const u64*>(rg.last_index)[g],
                   reinterpret_cast<const u64*>(rg.last_term)[g], meta_nruns(meta0)};
      ns = clamp_slots(s0, s1);
      const u32 state = role & 3u;
      const u32 min_ = cfg_incoming(cfg), mout = cfg_outgoing(cfg);
      const u32 oslot = meta_own_slot(meta0);
      ls = oslot < ns ? oslot : kNoSlot;
      u32 meta = meta0;

      // ---------------------------------------------------------- reads ---
      if (nr != 0) {
        if (state == QB_ROLE_LEADER) {
          const bool single = __popc(min_) == 1 && mout == 0;  // IsSingleton, tracker.go:228-230
          const bool cur = single || term_of_committed(A, lg, com) == term;  // raft.go:1731-1733
          const u32 ownbit = oslot < 16u ? 1u << oslot : 0u;
          u32 nq = meta_readq_len(meta0);
          if (nq > cap) nq = cap;
          const u32 nq0 = nq;
          u64* qctx = reinterpret_cast<u64*>(rg.rq_ctx) + g * cap;
          u64* qidx = reinterpret_cast<u64*>(rg.rq_index) + g * cap;
          u32* qmeta = rg.rq_meta + g * cap;
          for (u32 k = 0; k < nr; ++k) {
            const u64 at = u64(k) * G + g;
            const u64 ctx = rd_ctx[at];
            const u32 from = A.in.rd_from[at];
            u32 s;
            if (ctx == 0) {
              s = QB_RD_BAD;
              qf |= QB_QFLAG_BAD;
            } else if (from != kNoSlot && from >= ns) {
              s = QB_RD_HOST;
              qf |= QB_QFLAG_HOST;
            } else if (single || (cur && lease)) {  // raft.go:1080-1085, 1838-1841
              s = (from == kNoSlot || from == oslot) ? QB_RD_READ_STATE : QB_RD_RESP;
              rd_index[at] = com;
            } else if (!cur) {  // raft.go:1089-1092
              s = QB_RD_POSTPONED;
              meta |= QB_META_PENDING_READINDEX;
              qf |= QB_QFLAG_POSTPONED;
            } else {  // ReadOnlySafe, raft.go:1833-1837
              // addRequest, read_only.go:56-63: the queue's contexts four at
              // a time (branch-free, clamped)
              u32 found = kNone;
              for (u32 k0 = 0; k0 < nq && found == kNone; k0 += 4) {
                u64 c[4];
#pragma unroll
                for (u32 i = 0; i < 4; ++i) c[i] = qctx[k0 + i < nq ? k0 + i : nq - 1];
#pragma unroll
                for (u32 i = 0; i < 4; ++i)
                  if (found == kNone && k0 + i < nq && c[i] == ctx) found = k0 + i;
              }
              if (found == kNone && nq == cap) {
                s = QB_RD_QUEUE_FULL;
              } else {
                if (found == kNone) {
                  qctx[nq] = ctx;
                  qidx[nq] = com;
                  qmeta[nq] = ownbit | (from << 16);  // with recvAck(r.id), read_only.go:68-76
                  ++nq;
                  s = QB_RD_BCAST;
                } else {
                  if (ownbit) {
                    const u32 m = qmeta[found];
                    if (!(m & ownbit)) qmeta[found] = m | ownbit;
                  }
                  s = QB_RD_BCAST_DUP;
                }
                fl = 1;  // bcastHeartbeatWithCtx
              }
            }
            A.out.rd_status[at] = u8(s);
            packed += 1ull << (5u * (s - 1u));
          }
          if (nq != nq0) meta = (meta & ~(0x1Fu << 20)) | (nq << 20);
          if (fl) qf |= QB_QFLAG_HEARTBEATS;
        } else {
          u32 s = QB_RD_IGNORED;  // stepCandidate has no case
          if (state == QB_ROLE_FOLLOWER) {  // raft.go:1458-1464
            s = lead != 0 ? u32(QB_RD_FORWARD) : u32(QB_RD_DROPPED);
            if (lead != 0) qf |= QB_QFLAG_FORWARD;
          }
          for (u32 k = 0; k < nr; ++k) A.out.rd_status[u64(k) * G + g] = u8(s);
          packed += u64(nr) << (5u * (s - 1u));
        }
      }

      // ------------------------------------------------------- transfer ---
      if (xfrom != kNoSlot) {
        if (mterm != 0 && mterm < term) {  // raft.go:878-921: ignored
          x_ignterm = true;
        } else if (mterm > term) {  // raft.go:851-877: becomeFollower is the host's
          x_host = true;
          qf |= QB_QFLAG_HOST;
        } else if (state == QB_ROLE_LEADER) {  // raft.go:1099-1104, 1339-1370
          if (xfrom >= ns) {
            x_noprog = true;
          } else if (!(((min_ | mout) >> xfrom) & 1u)) {
            x_learner = true;
          } else {
            const u32 pending = meta_transferee(meta);
            bool go = true;
            if (pending != kNoSlot) {
              if (pending == xfrom) {
                x_same = true;
                go = false;
              } else {  // abortLeaderTransfer
                meta |= 0xFF00u;
                x_aborted = true;
                qf |= QB_QFLAG_TRANSFER_ABORTED;
              }
            }
            if (go && xfrom == oslot) {
              x_self = true;
            } else if (go) {
              rg.election_elapsed[g] = 0;
              meta = (meta & ~0xFF00u) | (xfrom << 8);
              x_started = true;
              qf |= QB_QFLAG_TRANSFER_STARTED;
              const u64 i = u64(s0) + xfrom;
              if (match[i] == lg.last) xt = QB_MSG_TIMEOUT_NOW;
              else xt = send_slot(A, lg, reinterpret_cast<const u64*>(rg.max_ents)[g], i);
            }
          }
        } else if (state == QB_ROLE_FOLLOWER) {  // raft.go:1445-1451
          if (lead != 0) {
            x_fwd = true;
            qf |= QB_QFLAG_FORWARD;
          } else {
            x_drop = true;
          }
        } else {
          x_role = true;
        }
      }
      if (meta != meta0) rg.meta[g] = meta;
    }
    if (live) {
      A.out.qflags[g] = qf;
      A.out.xf_type[g] = u8(xt);
    }
#pragma unroll
    for (u32 c = 0; c < kReadCodes; ++c) racc[c] += u32(packed >> (5u * c)) & 31u;

    // ------------------------------------------------------------- P2 ---
    const bool fires = __syncthreads_or(fl != 0);  // (also: the previous tile's LDS is free)
    if (fires) {
      S.bound(sb, se);
      if (S.staged) {
        if (fl) {
          ns = T.slots.claim(S, s0, ns);
          T.own[tid] = u8(ls);
          T.committed[tid] = com;
        }
        T.fl[tid] = fl;
        __syncthreads();
        for (u32 jb = tid; jb < S.span; jb += kBlock * kSpanUnroll) {
          u64 m[kSpanUnroll], c[kSpanUnroll];
          bool on[kSpanUnroll];
#pragma unroll
          for (u32 u = 0; u < kSpanUnroll; ++u) {
            const u32 j = jb + u * kBlock;
            on[u] = false;
            m[u] = c[u] = 0;
            if (j >= S.span) continue;
            const SpanOwners::Slot o = T.slots.find(j);
            const u32 t = o.t;
            if (!T.fl[t] || !o.in || o.k == T.own[t]) continue;
            on[u] = true;  // sendHeartbeat, raft.go:495-511
            c[u] = T.committed[t];
            m[u] = __builtin_nontemporal_load(match + u64(S.sb) + j);
          }
#pragma unroll
          for (u32 u = 0; u < kSpanUnroll; ++u)
            if (on[u])
              __builtin_nontemporal_store(m[u] < c[u] ? m[u] : c[u],
                                          hb_commit + u64(S.sb) + jb + u * kBlock);
        }
      } else if (fl) {
        for (u32 k = 0; k < ns; ++k) {
          if (k == ls) continue;
          const u64 mk = match[u64(s0) + k];
          hb_commit[u64(s0) + k] = mk < com ? mk : com;
        }
      }
    }
    tally.add(QB_QSTAT_BAD_COUNT, badcount);
    tally.add(QB_QSTAT_BCAST_GROUPS, fl != 0);
    tally.add(QB_QSTAT_XF_STARTED, x_started);
    tally.add(QB_QSTAT_XF_TIMEOUT_NOW, xt == QB_MSG_TIMEOUT_NOW);
    tally.add(QB_QSTAT_XF_MSG_APP, xt == QB_MSG_APP);
    tally.add(QB_QSTAT_XF_MSG_SNAP, xt == QB_MSG_SNAP);
    tally.add(QB_QSTAT_XF_ABORTED, x_aborted);
    tally.add(QB_QSTAT_XF_IGN_TERM, x_ignterm);
    tally.add(QB_QSTAT_XF_IGN_NO_PROGRESS, x_noprog);
    tally.add(QB_QSTAT_XF_IGN_LEARNER, x_learner);
    tally.add(QB_QSTAT_XF_IGN_SAME, x_same);
    tally.add(QB_QSTAT_XF_IGN_SELF, x_self);
    tally.add(QB_QSTAT_XF_IGN_ROLE, x_role);
    tally.add(QB_QSTAT_XF_FORWARD, x_fwd);
    tally.add(QB_QSTAT_XF_DROPPED, x_drop);
    tally.add(QB_QSTAT_XF_HOST, x_host);
  }
#pragma unroll
  for (u32 c = 0; c < kReadCodes; ++c) tally.add_n(int(c), racc[c]);  // QB_QSTAT_* 0..10
  __syncthreads();  // T.tally zeroed; the last tile's LDS reads done
  tally.stage(T.tally);
  __syncthreads();
  BlockTally<QB_QSTAT_COUNT>::publish(T.tally, reinterpret_cast<u64*>(A.stats));
}

static_assert(QB_QSTAT_READ_STATES == QB_RD_READ_STATE - 1 && QB_QSTAT_BAD_CTX == QB_RD_BAD - 1,
              "the read counters follow the rd_status codes");

}  // namespace requests
}  // namespace qb

using namespace qb;

extern "C" int qb_dev_leader_requests(const qb_request_groups* rg, const qb_request_in* in,
                                      const qb_request_out* out, uint64_t* stats, void* stream) {
  QB_REQUIRE(rg, "qb_dev_leader_requests: rg is NULL");
  QB_REQUIRE(in && out, "qb_dev_leader_requests: in / out is NULL");
  QB_REQUIRE(rg->inflight_cap >= 1 && rg->inflight_cap <= 4096,
             "qb_dev_leader_requests: inflight_cap must be 1..4096 (got %u)", rg->inflight_cap);
  QB_REQUIRE(rg->readq_cap <= QB_LEADER_MAX_READQ, "qb_dev_leader_requests: readq_cap %u > %d",
             rg->readq_cap, QB_LEADER_MAX_READQ);
  QB_REQUIRE(rg->read_only <= 1, "qb_dev_leader_requests: read_only must be 0 or 1 (got %u)",
             rg->read_only);
  QB_REQUIRE(rg->max_reads >= 1 && rg->max_reads <= QB_REQ_MAX_READS,
             "qb_dev_leader_requests: max_reads must be 1..%d (got %u)", QB_REQ_MAX_READS,
             rg->max_reads);
  if (rg->G == 0) return QB_OK;
  QB_REQUIRE(rg->off && rg->cfg && rg->meta && rg->role && rg->term && rg->lead && rg->committed &&
                 rg->first_index && rg->last_index && rg->last_term && rg->snap_index &&
                 rg->snap_term && rg->max_ents && rg->run_start && rg->run_term &&
                 rg->election_elapsed && rg->match && rg->next && rg->pending_snapshot &&
                 rg->pstate && rg->infl_pos && rg->infl_buf,
             "qb_dev_leader_requests: required group pointer is NULL");
  QB_REQUIRE(rg->readq_cap == 0 || (rg->rq_ctx && rg->rq_index && rg->rq_meta),
             "qb_dev_leader_requests: read queue arrays are NULL with readq_cap %u", rg->readq_cap);
  QB_REQUIRE(in->n_reads && in->rd_ctx && in->rd_from && in->xf_from,
             "qb_dev_leader_requests: required input pointer is NULL (n_reads / rd_ctx / rd_from / "
             "xf_from)");
  QB_REQUIRE(out->rd_status && out->rd_index && out->hb_commit && out->xf_type && out->xf_index &&
                 out->xf_log_term && out->xf_n && out->qflags && stats,
             "qb_dev_leader_requests: required output pointer is NULL (rd_status / rd_index / "
             "hb_commit / xf_type / xf_index / xf_log_term / xf_n / qflags / stats)");
  requests::Args A{*rg, *in, *out, reinterpret_cast<u64*>(stats)};
  hipLaunchKernelGGL(requests::k_requests, dim3(stream_grid<requests::k_requests>(rg->G)),
                     dim3(kBlock), 0, as_stream(stream), A);
  QB_CHECK_LAUNCH("k_requests");
  return QB_OK;
}
