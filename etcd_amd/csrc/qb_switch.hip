// qb_switch.hip — raft.switchToConfig behind a configuration change or a
// restored snapshot, for G groups at once (qb_dev_switch_config):
// raft.go:1651-1700, 585-588, 432-522, 1606-1609, progress.go:144-153.
//
// One kernel in the span-tile shape (qb_span_tile.h):
//   P1  thread per group: the action byte first; a group with nothing to do
//       writes its swflags byte and is done.  An acting group requests its
//       group words and both ID lists at once (at most 16 u64 each), ranks
//       the old IDs in the new list (the slot map), looks for the two stops,
//       renumbers meta, votes and the pending reads, and at a leader runs
//       maybeCommit over the new match values.  A group that sends claims its
//       new slots and leaves its recipe in LDS: first and last index, the
//       last term, entries per message, runs, own slot and how it sends.
//   P2  (only if a group of the tile sends) next, pstate and infl_pos are
//       read, maybeSendAppend runs per slot — (to, true) for every peer behind
//       a commit, (id, false) for every slot otherwise — and the message
//       columns are written.
// Nothing is appended here, so the run table covers the whole log; the term of
// last_index itself comes from last_term without a walk.
#include "qb_span_tile.h"

namespace qb {
namespace sw {

struct Args {
  qb_switch_groups sg;
  const u8* action;
  qb_switch_out out;
  u64* stats;
};

// how a group sends (Tile::mode)
constexpr u8 kSends = 1;    // step 5 ran
constexpr u8 kBcast = 2;    // behind a commit: bcastAppend
constexpr u8 kRestore = 4;  // MaybeUpdate(next - 1) on the own slot behind its send

// What maybeSendAppend needs of a slot's group.
struct Recipe {
  u64 g;
  u64 first, last, lastt, ments;
  u32 nruns;
};

struct Tile {
  SpanOwners slots;
  u64 first[kBlock], last[kBlock], lastt[kBlock], ments[kBlock];
  u8 mode[kBlock];  // non-zero: the group sends
  u8 own[kBlock];
  u8 nruns[kBlock];
  u32 tally[QB_SWSTAT_COUNT];
};

// The new slot of each old slot, a byte each.
struct SlotMap {
  u64 lo = ~0ull, hi = ~0ull;
  __device__ __forceinline__ void set(u32 k, u32 v) {
    const u64 m = 0xFFull << ((k & 7u) * 8), b = u64(v) << ((k & 7u) * 8);
    if (k < 8) lo = (lo & ~m) | b;
    else hi = (hi & ~m) | b;
  }
  // 0xFF for a removed slot and for k at or above the old slot count
  __device__ __forceinline__ u32 get(u32 k) const {
    if (k >= QB_MAX_SLOTS) return 0xFFu;
    return u32(((k < 8 ? lo : hi) >> ((k & 7u) * 8)) & 0xFFu);
  }
  // a 16-bit slot mask through the map; *dropped: a set bit had no new slot
  __device__ __forceinline__ u32 mask(u32 m, bool* dropped) const {
    u32 r = 0;
    m &= 0xFFFFu;
    while (m) {
      const u32 k = u32(__ffs(int(m))) - 1;
      m &= m - 1;
      const u32 v = get(k);
      if (v == 0xFFu) *dropped = true;
      else r |= 1u << v;
    }
    return r;
  }
};

// raftLog.term (log.go:268-288).
__device__ __forceinline__ u64 term_at(const Args& A, const Recipe& r, u64 i) {
  if (i < r.first - 1 || i > r.last) return 0;
  if (i == r.last) return r.lastt;
  return walk_runs(A.sg.run_start, A.sg.run_term, A.sg.G, r.g, i, r.nruns);
}

// maybeSendAppend(slot i, bcast) of r's group, the message to the slot's columns.
__device__ __forceinline__ u32 send_slot(const Args& A, const Recipe& r, bool bcast, u64 i, u64 nx,
                                         u8 st, u32 ipos) {
  u64* mi = reinterpret_cast<u64*>(A.out.msg_index) + i;
  u64* ml = reinterpret_cast<u64*>(A.out.msg_log_term) + i;
  u64* mn = reinterpret_cast<u64*>(A.out.msg_n) + i;
  const auto tp = [&] { return term_at(A, r, nx - 1); };
  return bcast ? maybe_send_append<true>(A.sg, r.g, i, nx, st, ipos, r.first, r.last, r.ments, tp,
                                         mi, ml, mn)
               : maybe_send_append<false>(A.sg, r.g, i, nx, st, ipos, r.first, r.last, r.ments, tp,
                                          mi, ml, mn);
}

// MaybeUpdate(next - 1) on slot i (progress.go:144-153): next stays.
__device__ __forceinline__ void update_to_next(const qb_switch_groups& sg, u64 i) {
  u64* match = reinterpret_cast<u64*>(sg.match);
  const u64 n = reinterpret_cast<const u64*>(sg.next)[i] - 1;
  if (match[i] < n) {
    match[i] = n;
    const u8 st = sg.pstate[i];
    if (st & QB_PR_PROBE_SENT) sg.pstate[i] = u8(st & ~QB_PR_PROBE_SENT);
  }
}

__global__ __launch_bounds__(kBlock) void k_switch(Args A) {
  __shared__ Tile T;
  const qb_switch_groups& sg = A.sg;
  const u64 G = sg.G;
  const u64 ntiles = (G + kBlock - 1) / kBlock;
  const u32 tid = threadIdx.x;
  const u64* __restrict__ oid_a = reinterpret_cast<const u64*>(sg.old_ids);
  const u64* __restrict__ nid_a = reinterpret_cast<const u64*>(sg.ids);
  u64* __restrict__ com_a = reinterpret_cast<u64*>(sg.committed);
  u64* __restrict__ match_a = reinterpret_cast<u64*>(sg.match);
  u64* __restrict__ next_a = reinterpret_cast<u64*>(sg.next);
  BlockTally<QB_SWSTAT_COUNT> tally;
  if (tid < QB_SWSTAT_COUNT) T.tally[tid] = 0;

  for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    SpanTile S(tile, G);
    const u64 g = S.g0 + tid;
    const bool live = g < G;
    const u32 sb = sg.off[S.g0], se = sg.off[S.gend];  // the tile's span (used in P2 only)

    // ------------------------------------------------------------- P1 ---
    const u8 action = live ? A.action[g] : u8(0);
    const bool bad = action > QB_SW_RESTORE;
    const bool acts = action == QB_SW_SWITCH || action == QB_SW_RESTORE;
    u32 s0 = 0, ns = 0, own = 0xFFu, napp = 0, nsnap = 0;
    u8 sf = 0, mode = 0;
    Recipe rc{};
    if (acts) {
      // every group word and both ID lists, requested together
      const u32 o0 = sg.old_off[g], o1 = sg.old_off[g + 1];
      s0 = sg.off[g];
      const u32 s1 = sg.off[g + 1];
      const u32 cfg = sg.cfg[g];
      const u32 meta = sg.meta[g];
      const u8 role = sg.role[g];
      const u64 self = reinterpret_cast<const u64*>(sg.self_id)[g];
      const u64 term = reinterpret_cast<const u64*>(sg.term)[g], com0 = com_a[g];
      const u64 first = reinterpret_cast<const u64*>(sg.first_index)[g];
      const u64 last = reinterpret_cast<const u64*>(sg.last_index)[g];
      const u64 lastt = reinterpret_cast<const u64*>(sg.last_term)[g];
      const u64 ments = reinterpret_cast<const u64*>(sg.max_ents)[g];
      const u32 votes = sg.votes ? sg.votes[g] : 0u;
      const u32 no = clamp_slots(o0, o1);
      ns = clamp_slots(s0, s1);
      u64 oid[QB_MAX_SLOTS], nid[QB_MAX_SLOTS];
#pragma unroll
      for (u32 k = 0; k < QB_MAX_SLOTS; ++k) {
        oid[k] = k < no ? oid_a[u64(o0) + k] : 0;
        nid[k] = k < ns ? nid_a[u64(s0) + k] : 0;
      }
      // 1. the slot map: the rank of each old ID in the new list
      SlotMap map;
#pragma unroll
      for (u32 j = 0; j < QB_MAX_SLOTS; ++j) {
        if (j < ns && nid[j] == self) own = j;
#pragma unroll
        for (u32 k = 0; k < QB_MAX_SLOTS; ++k)
          if (j < ns && k < no && nid[j] == oid[k]) map.set(k, j);
      }
      const u32 voters = cfg_incoming(cfg) | cfg_outgoing(cfg);
      const bool leader = (role & 3u) == QB_ROLE_LEADER;
      const bool self_out = own == 0xFFu || !((voters >> own) & 1u);
      const u32 xf0 = meta_transferee(meta);
      u32 xf = xf0 == 0xFFu ? 0xFFu : map.get(xf0);
      // 2. the stops
      bool stop = leader && self_out && xf0 != 0xFFu && xf == 0xFFu;
      const u32 cap = sg.readq_cap;
      const u32 nrq = meta_readq_len(meta) < cap ? meta_readq_len(meta) : cap;
      u32* qmeta = sg.rq_meta + g * cap;
      for (u32 k = 0; k < nrq; ++k) {
        const u32 from = (qmeta[k] >> 16) & 0xFFu;
        stop |= from != 0xFFu && map.get(from) == 0xFFu;
      }
      if (stop) {
        sf = QB_SWFLAG_HOST;
      } else {
        sf = QB_SWFLAG_SWITCHED;
        if (A.out.slot_map)
          for (u32 k = 0; k < no; ++k) A.out.slot_map[u64(o0) + k] = u8(map.get(k));
        bool dropped = false, vdropped = false;
        for (u32 k = 0; k < nrq; ++k) {
          const u32 q = qmeta[k];
          const u32 from = (q >> 16) & 0xFFu;
          const u32 q1 = (q & 0xFF000000u) | map.mask(q, &dropped) |
                         ((from == 0xFFu ? 0xFFu : map.get(from)) << 16);
          if (q1 != q) qmeta[k] = q1;
        }
        if (sg.votes) {
          const u32 voted = map.mask(votes, &vdropped), granted = map.mask(votes >> 16, &dropped);
          const u32 v1 = voted | (granted << 16);
          if (v1 != votes) sg.votes[g] = v1;
          if (vdropped) sf |= QB_SWFLAG_VOTE_DROPPED;
        }
        // 3. a leader that is removed or demoted
        if (leader && self_out) {
          sf |= own == 0xFFu ? QB_SWFLAG_SELF_REMOVED : QB_SWFLAG_SELF_LEARNER;
        } else if (leader && cfg_incoming(cfg) != 0) {  // 4.
          // 5. maybeCommit (raft.go:585-588).  First whether every non-empty
          // half has a quorum above committed at all: one pass over match.
          rc = Recipe{g, first, last, lastt, ments, meta_nruns(meta)};
          const u32 min_ = cfg_incoming(cfg), mout = cfg_outgoing(cfg);
          int cin = 0, cout = 0;
          for (u32 k = 0; k < ns; ++k) {
            const bool gt = match_a[u64(s0) + k] > com0;
            cin += gt && ((min_ >> k) & 1u);
            cout += gt && ((mout >> k) & 1u);
          }
          const bool can = cin >= __popc(min_) / 2 + 1 && (mout == 0 || cout >= __popc(mout) / 2 + 1);
          bool committed = false;
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
                const u64 va = match_a[u64(s0) + a];
                if (va <= best) continue;
                int c = 0;
                for (u32 b = 0; b < ns; ++b) c += ((mask >> b) & 1u) && match_a[u64(s0) + b] >= va;
                if (c >= q) best = va;
              }
              if (best < mci) mci = best;
            }
            if (mci > com0 && term_at(A, rc, mci) == term) {
              com_a[g] = mci;
              committed = true;
            }
          }
          sf |= QB_SWFLAG_SENT | (committed ? QB_SWFLAG_COMMITTED : 0u);
          mode = kSends | (committed ? kBcast : 0);
          // 6. the transferee was removed or demoted
          if (xf0 != 0xFFu && (xf == 0xFFu || !((voters >> xf) & 1u))) {
            xf = 0xFFu;
            sf |= QB_SWFLAG_TRANSFER_ABORTED;
          }
        }
        const u32 meta1 = (meta & ~0xFFFFu) | own | (xf << 8);
        if (meta1 != meta) sg.meta[g] = meta1;
        // 7. the end of restore; behind the own slot's send if the group sends
        if (action == QB_SW_RESTORE && own != 0xFFu) {
          if (mode) mode |= kRestore;
          else update_to_next(sg, u64(s0) + own);
        }
      }
    }
    if (live) A.out.swflags[g] = sf;

    // ------------------------------------------------------------- P2 ---
    const bool fires = __syncthreads_or(mode != 0);  // (also: the previous tile's LDS is free)
    if (fires) {
      S.bound(sb, se);
      if (S.staged) {
        if (mode) {
          ns = T.slots.claim(S, s0, ns);
          T.own[tid] = u8(own);
          T.nruns[tid] = u8(rc.nruns);
          T.first[tid] = rc.first;
          T.last[tid] = rc.last;
          T.lastt[tid] = rc.lastt;
          T.ments[tid] = rc.ments;
        }
        T.mode[tid] = mode;
        __syncthreads();
        for (u32 jb = tid; jb < S.span; jb += kBlock * kSpanUnroll) {
          // the trip's slot words first, then the sends
          u32 t_[kSpanUnroll], ip[kSpanUnroll];
          u64 nx[kSpanUnroll];
          u8 st[kSpanUnroll], what[kSpanUnroll];  // what: 0 not ours, 1 sends, 2 the own slot behind a commit
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
            if (!T.mode[t] || !o.in) continue;
            t_[u] = t | (o.k == T.own[t] ? 0x100u : 0u);
            what[u] = (o.k == T.own[t] && (T.mode[t] & kBcast)) ? 2 : 1;
            if (what[u] == 1) {
              const u64 i = u64(S.sb) + j;
              nx[u] = next_a[i];
              st[u] = sg.pstate[i];
              ip[u] = sg.infl_pos[i];
            }
          }
#pragma unroll
          for (u32 u = 0; u < kSpanUnroll; ++u) {
            if (!what[u]) continue;
            const u64 i = u64(S.sb) + jb + u * kBlock;
            const u32 t = t_[u] & 0xFFu;
            const u8 m = T.mode[t];
            u32 mt = 0;
            if (what[u] == 1) {
              const Recipe r{S.g0 + t, T.first[t], T.last[t], T.lastt[t], T.ments[t], T.nruns[t]};
              mt = send_slot(A, r, (m & kBcast) != 0, i, nx[u], st[u], ip[u]);
              napp += mt == QB_MSG_APP;
              nsnap += mt == QB_MSG_SNAP;
            }
            A.out.msg_type[i] = u8(mt);
            if ((t_[u] & 0x100u) && (m & kRestore)) update_to_next(sg, i);
          }
        }
      } else if (mode) {
        for (u32 k = 0; k < ns; ++k) {
          const u64 i = u64(s0) + k;
          u32 mt = 0;
          if (!(k == own && (mode & kBcast))) {
            mt = send_slot(A, rc, (mode & kBcast) != 0, i, next_a[i], sg.pstate[i], sg.infl_pos[i]);
            napp += mt == QB_MSG_APP;
            nsnap += mt == QB_MSG_SNAP;
          }
          A.out.msg_type[i] = u8(mt);
          if (k == own && (mode & kRestore)) update_to_next(sg, i);
        }
      }
    }
    tally.add(QB_SWSTAT_SWITCHED, (sf & QB_SWFLAG_SWITCHED) != 0);
    tally.add(QB_SWSTAT_RESTORES, (sf & QB_SWFLAG_SWITCHED) && action == QB_SW_RESTORE);
    tally.add(QB_SWSTAT_COMMITS, (sf & QB_SWFLAG_COMMITTED) != 0);
    tally.add(QB_SWSTAT_BCAST, (mode & kBcast) != 0);
    tally.add(QB_SWSTAT_PROBED, mode && !(mode & kBcast));
    tally.add_n(QB_SWSTAT_MSG_APP, napp);
    tally.add_n(QB_SWSTAT_MSG_SNAP, nsnap);
    tally.add(QB_SWSTAT_TRANSFER_ABORTED, (sf & QB_SWFLAG_TRANSFER_ABORTED) != 0);
    tally.add(QB_SWSTAT_SELF_REMOVED, (sf & QB_SWFLAG_SELF_REMOVED) != 0);
    tally.add(QB_SWSTAT_SELF_LEARNER, (sf & QB_SWFLAG_SELF_LEARNER) != 0);
    tally.add(QB_SWSTAT_VOTE_DROPPED, (sf & QB_SWFLAG_VOTE_DROPPED) != 0);
    tally.add(QB_SWSTAT_HOST, (sf & QB_SWFLAG_HOST) != 0);
    tally.add(QB_SWSTAT_BAD_ACTION, live && bad);
  }
  __syncthreads();  // T.tally zeroed; the last tile's LDS reads done
  tally.stage(T.tally);
  __syncthreads();
  BlockTally<QB_SWSTAT_COUNT>::publish(T.tally, reinterpret_cast<u64*>(A.stats));
}

}  // namespace sw
}  // namespace qb

using namespace qb;

extern "C" int qb_dev_switch_config(const qb_switch_groups* sg, const uint8_t* action,
                                    const qb_switch_out* out, uint64_t* stats, void* stream) {
  QB_REQUIRE(sg, "qb_dev_switch_config: sg is NULL");
  QB_REQUIRE(out, "qb_dev_switch_config: out is NULL");
  QB_REQUIRE(sg->inflight_cap >= 1 && sg->inflight_cap <= 4096,
             "qb_dev_switch_config: inflight_cap must be 1..4096 (got %u)", sg->inflight_cap);
  QB_REQUIRE(sg->readq_cap <= QB_LEADER_MAX_READQ,
             "qb_dev_switch_config: readq_cap must be 0..%d (got %u)", QB_LEADER_MAX_READQ,
             sg->readq_cap);
  if (sg->G == 0) return QB_OK;
  QB_REQUIRE(sg->old_off && sg->old_ids && sg->off && sg->ids && sg->cfg && sg->self_id &&
                 sg->role && sg->term && sg->first_index && sg->last_index && sg->last_term &&
                 sg->snap_index && sg->snap_term && sg->max_ents && sg->run_start &&
                 sg->run_term && sg->meta && sg->committed && sg->match && sg->next &&
                 sg->pending_snapshot && sg->pstate && sg->infl_pos && sg->infl_buf,
             "qb_dev_switch_config: required group pointer is NULL");
  QB_REQUIRE(sg->readq_cap == 0 || sg->rq_meta,
             "qb_dev_switch_config: rq_meta is NULL with readq_cap %u", sg->readq_cap);
  QB_REQUIRE(action, "qb_dev_switch_config: action is NULL");
  QB_REQUIRE(out->swflags && out->msg_type && out->msg_index && out->msg_log_term && out->msg_n &&
                 stats,
             "qb_dev_switch_config: required output pointer is NULL (swflags / msg_type / "
             "msg_index / msg_log_term / msg_n / stats)");
  sw::Args A{*sg, action, *out, reinterpret_cast<u64*>(stats)};
  hipLaunchKernelGGL(sw::k_switch, dim3(stream_grid<sw::k_switch>(sg->G)), dim3(kBlock), 0,
                     as_stream(stream), A);
  QB_CHECK_LAUNCH("k_switch");
  return QB_OK;
}
