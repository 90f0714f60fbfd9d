// qb_propose.hip — Step(MsgProp) -> appendEntry -> bcastAppend at the leaders
// of G groups at once, and the log's share of becomeLeader
// (qb_dev_leader_propose): raft.go:1019-1077, 621-642, 1761-1779, 432-522,
// 745-756.  The one call that lets a leader's log grow on the device.
//
// One kernel in the span-tile shape (qb_span_tile.h):
//   P1  thread per group: the action byte first; a group with nothing to do
//       writes its pflags byte and is done.  An acting group requests all its
//       group words at once (one HBM round trip), decides the proposal (role,
//       drops, the conf-change rule, the size limit, the run-table stop),
//       appends, and in a second trip runs MaybeUpdate on its own slot and
//       maybeCommit over its match values.  A group that broadcasts claims its
//       slots and leaves its recipe in LDS: new last index, old last index and
//       term, term, first index, entries per message, own slot.
//   P2  (only if a group of the tile broadcasts) next, pstate and infl_pos are
//       read, maybeSendAppend runs per slot and the message columns are
//       written.
// The term of next - 1 follows from the recipe wherever next - 1 is at or past
// the old last index (old last: last_term; beyond it: the leader's term), so
// the steady proposal reads and writes no run table; an older next - 1 walks
// the group's runs (not its entries).
//
// The entry count goes through a 64-bit cell beside the BlockTally.
#include "qb_span_tile.h"

namespace qb {
namespace propose {

struct Args {
  qb_propose_groups pg;
  qb_propose_in in;
  qb_propose_out out;
  u64* stats;
};

// What maybeSendAppend needs of a slot's group.
struct Recipe {
  u64 g;
  u64 last;   // last index behind the append
  u64 old;    // last index at entry
  u64 term;   // the leader's term: the term of (old, last]
  u64 oldt;   // last_term at entry: the term of old
  u64 ments;  // entries per MsgApp
  u64 first;  // firstIndex
  u32 nruns;  // runs of the table at entry (they cover [first - 1, old])
};

struct Tile {
  SpanOwners slots;
  u64 last[kBlock], old[kBlock], term[kBlock], oldt[kBlock], ments[kBlock], first[kBlock];
  u8 fl[kBlock];      // non-zero: the group broadcasts
  u8 own[kBlock];      // own slot
  u8 nruns[kBlock];
  u32 tally[QB_PSTAT_COUNT];
  u64 ents;            // entries appended by the block
};

// raftLog.term (log.go:268-288) behind the append.  The run table is read only
// for an index below the old last index.
__device__ __forceinline__ u64 term_at(const Args& A, const Recipe& r, u64 i) {
  if (i < r.first - 1 || i > r.last) return 0;
  if (i > r.old) return r.term;
  if (i == r.old) return r.oldt;
  return walk_runs(A.pg.run_start, A.pg.run_term, A.pg.G, r.g, i, r.nruns);
}

// maybeSendAppend on slot i of r's group, the message to the slot's columns.
__device__ __forceinline__ u32 send_slot(const Args& A, const Recipe& r, u64 i, u64 nx, u8 st,
                                         u32 ipos) {
  return maybe_send_append(A.pg, r.g, i, nx, st, ipos, r.first, r.last, r.ments,
                           [&] { return term_at(A, r, nx - 1); },
                           reinterpret_cast<u64*>(A.out.msg_index) + i,
                           reinterpret_cast<u64*>(A.out.msg_log_term) + i,
                           reinterpret_cast<u64*>(A.out.msg_n) + i);
}

__device__ __forceinline__ u64 wave_sum64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u32 lo = u32(__shfl_xor(int(u32(v)), o, 64));
    const u32 hi = u32(__shfl_xor(int(u32(v >> 32)), o, 64));
    v += (u64(hi) << 32) | lo;
  }
  return v;
}

__global__ __launch_bounds__(kBlock) void k_propose(Args A) {
  __shared__ Tile T;
  const qb_propose_groups& pg = A.pg;
  const u64 G = pg.G;
  const u64 ntiles = (G + kBlock - 1) / kBlock;
  const u32 tid = threadIdx.x;
  const u64 limit = pg.max_uncommitted_size ? u64(pg.max_uncommitted_size) : kInf;  // noLimit
  const u64* __restrict__ term_a = reinterpret_cast<const u64*>(pg.term);
  u64* __restrict__ com_a = reinterpret_cast<u64*>(pg.committed);
  u64* __restrict__ last_a = reinterpret_cast<u64*>(pg.last_index);
  u64* __restrict__ lastt_a = reinterpret_cast<u64*>(pg.last_term);
  u64* __restrict__ unc_a = reinterpret_cast<u64*>(pg.uncommitted_size);
  u64* __restrict__ pci_a = reinterpret_cast<u64*>(pg.pending_conf_index);
  u64* __restrict__ match_a = reinterpret_cast<u64*>(pg.match);
  u64* __restrict__ next_a = reinterpret_cast<u64*>(pg.next);
  BlockTally<QB_PSTAT_COUNT> tally;
  if (tid < QB_PSTAT_COUNT) T.tally[tid] = 0;
  if (tid == 0) T.ents = 0;
  u64 ents = 0;  // entries this thread's groups appended

  for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    SpanTile S(tile, G);
    const u64 g = S.g0 + tid;
    const bool live = g < G;
    const u32 sb = pg.off[S.g0], se = pg.off[S.gend];  // the tile's span (used in P2 only)

    // ------------------------------------------------------------- P1 ---
    const u8 action = live ? A.in.action[g] : u8(0);
    const u32 code = action & 0x3Fu;
    const bool bad = code > QB_PROP_LEADER_ENTRY;
    const bool acts = code != QB_PROP_NONE && !bad;
    u32 s0 = 0, ns = 0, own = 0xFFu, napp = 0, nsnap = 0;
    u8 pf = 0, fl = 0;
    Recipe rc{};
    bool d_noprog = false, d_transfer = false, d_size = false, d_nolead = false, d_fwd = false,
         d_cand = false, forwarded = false, cc_acc = false, cc_ref = false, committed = false,
         lentry = false, runs_stop = false, empty = false, ign_role = false, appended = false;
    if (acts) {
      // every group word of the proposal, requested together
      const u8 role = pg.role[g];
      const u32 meta = pg.meta[g];
      const u32 cfg = pg.cfg[g];
      s0 = pg.off[g];
      const u32 s1 = pg.off[g + 1];
      const u64 term = term_a[g], last0 = last_a[g], lt0 = lastt_a[g], com0 = com_a[g];
      const u32 n = A.in.n_ents[g];
      const u64 pay = reinterpret_cast<const u64*>(A.in.payload)[g], unc0 = unc_a[g];
      const u64 ments = reinterpret_cast<const u64*>(pg.max_ents)[g];
      const u64 first = reinterpret_cast<const u64*>(pg.first_index)[g];
      ns = clamp_slots(s0, s1);
      const u32 state = role & 3u;
      const bool entries = code == QB_PROP_ENTRIES;
      if (state != QB_ROLE_LEADER) {
        if (!entries) {
          ign_role = true;
        } else if (state == QB_ROLE_FOLLOWER) {  // raft.go:1423-1430
          if (reinterpret_cast<const u64*>(pg.lead)[g] == 0) {
            d_nolead = true;
            pf = QB_PFLAG_DROPPED;
          } else if (pg.disable_proposal_forwarding) {
            d_fwd = true;
            pf = QB_PFLAG_DROPPED;
          } else {
            forwarded = true;
            pf = QB_PFLAG_FORWARD;
          }
        } else {  // raft.go:1387-1389
          d_cand = true;
          pf = QB_PFLAG_DROPPED;
        }
      } else {
        const u32 nruns = meta_nruns(meta);
        const bool newrun = lt0 != term;
        const u32 oslot = meta_own_slot(meta);
        if (entries && n == 0) {  // raft.go:1020-1022
          empty = true;
          pf = QB_PFLAG_BAD;
        } else if (entries && oslot >= ns) {  // raft.go:1023-1028
          d_noprog = true;
          pf = QB_PFLAG_DROPPED;
        } else if (entries && meta_transferee(meta) != 0xFFu) {  // raft.go:1029-1032
          d_transfer = true;
          pf = QB_PFLAG_DROPPED;
        } else if (newrun && nruns == QB_LEADER_MAX_RUNS) {
          runs_stop = true;
          pf = QB_PFLAG_LOG_RUNS;
        } else {
          bool drop = false;
          u32 cnt = 1;
          if (entries) {
            cnt = n;
            u64 s = pay;
            if (action & QB_PROP_CONF_CHANGE) {  // raft.go:1050-1070
              const u32 at = A.in.cc_at[g];
              if (at < n) {
                const u64 pci = pci_a[g];
                const u64 applied = reinterpret_cast<const u64*>(pg.applied)[g];
                const bool joint = cfg_outgoing(cfg) != 0;
                const bool leave = (action & QB_PROP_CC_LEAVE_JOINT) != 0;
                if (pci > applied || joint != leave) {
                  cc_ref = true;
                  pf |= QB_PFLAG_CC_REFUSED;
                  s = pay - reinterpret_cast<const u64*>(A.in.cc_payload)[g];
                } else {
                  cc_acc = true;
                  pci_a[g] = last0 + at + 1;
                }
              }
            }
            // increaseUncommittedSize, raft.go:1761-1779
            if (unc0 > 0 && s > 0 && unc0 + s > limit) {
              drop = d_size = true;
              pf |= QB_PFLAG_DROPPED;
            } else if (s != 0) {
              unc_a[g] = unc0 + s;
            }
          } else {  // becomeLeader, raft.go:745-756
            lentry = true;
            pci_a[g] = last0;
            if (unc0 != 0) unc_a[g] = 0;
          }
          if (!drop) {
            // raftLog.append through the term index
            if (newrun) {
              reinterpret_cast<u64*>(pg.run_start)[u64(nruns) * G + g] = last0 + 1;
              reinterpret_cast<u64*>(pg.run_term)[u64(nruns) * G + g] = term;
              pg.meta[g] = (meta & ~(0xFu << 16)) | ((nruns + 1) << 16);
              lastt_a[g] = term;
            }
            const u64 last1 = last0 + cnt;
            last_a[g] = last1;
            appended = true;
            pf |= QB_PFLAG_APPENDED;
            ents += cnt;
            if (entries) {
              own = oslot;
              rc = Recipe{g, last1, last0, term, lt0, ments, first, nruns};
              // MaybeUpdate(last1) on the own slot (progress.go:146-157)
              const u64 io = u64(s0) + oslot;
              const u64 m0 = match_a[io], nx0 = next_a[io];
              const u8 st0 = pg.pstate[io];
              u64 ownm = m0;
              if (m0 < last1) {
                ownm = last1;
                match_a[io] = last1;
                if (st0 & QB_PR_PROBE_SENT) pg.pstate[io] = u8(st0 & ~QB_PR_PROBE_SENT);
              }
              if (nx0 < last1 + 1) next_a[io] = last1 + 1;
              // maybeCommit (raft.go:585-588).  First whether every non-empty
              // half has a quorum above committed at all: one pass over match.
              const u32 min_ = cfg_incoming(cfg), mout = cfg_outgoing(cfg);
              int cin = 0, cout = 0;
              for (u32 k = 0; k < ns; ++k) {
                const u64 mk = k == oslot ? ownm : match_a[u64(s0) + k];
                const bool gt = mk > com0;
                cin += gt && ((min_ >> k) & 1u);
                cout += gt && ((mout >> k) & 1u);
              }
              const bool can = (min_ == 0 || cin >= __popc(min_) / 2 + 1) &&
                               (mout == 0 || cout >= __popc(mout) / 2 + 1);
              if (can) {
                // the q-th largest match of each half (majority.go:126-172)
                u64 mci = kInf;
                for (u32 h = 0; h < 2; ++h) {
                  const u32 mask = h ? mout : min_;
                  if (mask == 0) continue;
                  const int q = __popc(mask) / 2 + 1;
                  u64 best = 0;
                  for (u32 a = 0; a < ns; ++a) {
                    if (!((mask >> a) & 1u)) continue;
                    const u64 va = a == oslot ? ownm : match_a[u64(s0) + a];
                    if (va <= best) continue;
                    int c = 0;
                    for (u32 b = 0; b < ns; ++b) {
                      const u64 vb = b == oslot ? ownm : match_a[u64(s0) + b];
                      c += ((mask >> b) & 1u) && vb >= va;
                    }
                    if (c >= q) best = va;
                  }
                  if (best < mci) mci = best;
                }
                if (mci > com0 && term_at(A, rc, mci) == term) {
                  com_a[g] = mci;
                  committed = true;
                  pf |= QB_PFLAG_COMMITTED;
                }
              }
              pf |= QB_PFLAG_BCAST;
              fl = 1;
            }
          }
        }
      }
    }
    if (live) A.out.pflags[g] = pf;

    // ------------------------------------------------------------- P2 ---
    const bool fires = __syncthreads_or(fl != 0);  // (also: the previous tile's LDS is free)
    if (fires) {
      S.bound(sb, se);
      if (S.staged) {
        if (fl) {
          ns = T.slots.claim(S, s0, ns);
          T.own[tid] = u8(own);
          T.nruns[tid] = u8(rc.nruns);
          T.last[tid] = rc.last;
          T.old[tid] = rc.old;
          T.term[tid] = rc.term;
          T.oldt[tid] = rc.oldt;
          T.ments[tid] = rc.ments;
          T.first[tid] = rc.first;
        }
        T.fl[tid] = fl;
        __syncthreads();
        for (u32 jb = tid; jb < S.span; jb += kBlock * kSpanUnroll) {
          // the trip's slot words first, then the sends
          u32 t_[kSpanUnroll], ip[kSpanUnroll];
          u64 nx[kSpanUnroll];
          u8 st[kSpanUnroll], what[kSpanUnroll];  // what: 0 not ours, 1 a peer, 2 the own slot
#pragma unroll
          for (u32 u = 0; u < kSpanUnroll; ++u) {
            const u32 j = jb + u * kBlock;
            what[u] = 0;
            t_[u] = 0;
            ip[u] = 0;
            nx[u] = 0;
            st[u] = 0;
            if (j >= S.span) continue;
            const SpanOwners::Slot o = T.slots.find(j);
            const u32 t = o.t;
            if (!T.fl[t] || !o.in) continue;
            t_[u] = t;
            what[u] = o.k == T.own[t] ? 2 : 1;
            if (what[u] == 1) {
              const u64 i = u64(S.sb) + j;
              nx[u] = next_a[i];
              st[u] = pg.pstate[i];
              ip[u] = pg.infl_pos[i];
            }
          }
#pragma unroll
          for (u32 u = 0; u < kSpanUnroll; ++u) {
            if (!what[u]) continue;
            const u64 i = u64(S.sb) + jb + u * kBlock;
            u32 mt = 0;
            if (what[u] == 1) {
              const u32 t = t_[u];
              const Recipe r{S.g0 + t, T.last[t], T.old[t], T.term[t], T.oldt[t], T.ments[t],
                             T.first[t], T.nruns[t]};
              mt = send_slot(A, r, i, nx[u], st[u], ip[u]);
              napp += mt == QB_MSG_APP;
              nsnap += mt == QB_MSG_SNAP;
            }
            A.out.msg_type[i] = u8(mt);
          }
        }
      } else if (fl) {
        for (u32 k = 0; k < ns; ++k) {
          const u64 i = u64(s0) + k;
          u32 mt = 0;
          if (k != own) {
            mt = send_slot(A, rc, i, next_a[i], pg.pstate[i], pg.infl_pos[i]);
            napp += mt == QB_MSG_APP;
            nsnap += mt == QB_MSG_SNAP;
          }
          A.out.msg_type[i] = u8(mt);
        }
      }
    }
    tally.add(QB_PSTAT_PROPOSALS, appended && !lentry);
    tally.add(QB_PSTAT_DROP_NO_PROGRESS, d_noprog);
    tally.add(QB_PSTAT_DROP_TRANSFER, d_transfer);
    tally.add(QB_PSTAT_DROP_SIZE, d_size);
    tally.add(QB_PSTAT_DROP_NO_LEADER, d_nolead);
    tally.add(QB_PSTAT_DROP_FORWARDING, d_fwd);
    tally.add(QB_PSTAT_DROP_CANDIDATE, d_cand);
    tally.add(QB_PSTAT_FORWARDED, forwarded);
    tally.add(QB_PSTAT_CC_ACCEPTED, cc_acc);
    tally.add(QB_PSTAT_CC_REFUSED, cc_ref);
    tally.add_n(QB_PSTAT_MSG_APP, napp);
    tally.add_n(QB_PSTAT_MSG_SNAP, nsnap);
    tally.add(QB_PSTAT_COMMITS, committed);
    tally.add(QB_PSTAT_LEADER_ENTRIES, appended && lentry);
    tally.add(QB_PSTAT_LOG_RUNS, runs_stop);
    tally.add(QB_PSTAT_EMPTY, empty);
    tally.add(QB_PSTAT_IGNORED_ROLE, ign_role);
    tally.add(QB_PSTAT_BAD_ACTION, live && bad);
  }
  __syncthreads();  // T.tally / T.ents zeroed; the last tile's LDS reads done
  tally.stage(T.tally);
  ents = wave_sum64(ents);  // (u64: a block's entries can pass 2^32)
  if ((tid & 63) == 0 && ents) atomicAdd(&T.ents, ents);
  __syncthreads();
  BlockTally<QB_PSTAT_COUNT>::publish(T.tally, reinterpret_cast<u64*>(A.stats));
  if (tid == 0 && T.ents) atomicAdd(reinterpret_cast<u64*>(A.stats) + QB_PSTAT_ENTRIES, T.ents);
}

}  // namespace propose
}  // namespace qb

using namespace qb;

extern "C" int qb_dev_leader_propose(const qb_propose_groups* pg, const qb_propose_in* in,
                                     const qb_propose_out* out, uint64_t* stats, void* stream) {
  QB_REQUIRE(pg, "qb_dev_leader_propose: pg is NULL");
  QB_REQUIRE(in && out, "qb_dev_leader_propose: in / out is NULL");
  QB_REQUIRE(pg->inflight_cap >= 1 && pg->inflight_cap <= 4096,
             "qb_dev_leader_propose: inflight_cap must be 1..4096 (got %u)", pg->inflight_cap);
  QB_REQUIRE(pg->disable_proposal_forwarding <= 1,
             "qb_dev_leader_propose: disable_proposal_forwarding must be 0 or 1 (got %u)",
             pg->disable_proposal_forwarding);
  if (pg->G == 0) return QB_OK;
  QB_REQUIRE(pg->off && pg->cfg && pg->role && pg->term && pg->lead && pg->first_index &&
                 pg->snap_index && pg->snap_term && pg->max_ents && pg->applied && pg->meta &&
                 pg->committed && pg->last_index && pg->last_term && pg->run_start &&
                 pg->run_term && pg->uncommitted_size && pg->pending_conf_index && pg->match &&
                 pg->next && pg->pending_snapshot && pg->pstate && pg->infl_pos && pg->infl_buf,
             "qb_dev_leader_propose: required group pointer is NULL");
  QB_REQUIRE(in->action && in->n_ents && in->payload && in->cc_at && in->cc_payload,
             "qb_dev_leader_propose: required input pointer is NULL (action / n_ents / payload / "
             "cc_at / cc_payload)");
  QB_REQUIRE(out->pflags && out->msg_type && out->msg_index && out->msg_log_term && out->msg_n &&
                 stats,
             "qb_dev_leader_propose: required output pointer is NULL (pflags / msg_type / "
             "msg_index / msg_log_term / msg_n / stats)");
  propose::Args A{*pg, *in, *out, reinterpret_cast<u64*>(stats)};
  hipLaunchKernelGGL(propose::k_propose, dim3(stream_grid<propose::k_propose>(pg->G)),
                     dim3(kBlock), 0, as_stream(stream), A);
  QB_CHECK_LAUNCH("k_propose");
  return QB_OK;
}
