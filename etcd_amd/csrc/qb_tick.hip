// qb_tick.hip — raft.tick() for G groups at once (qb_dev_leader_tick):
// tickElection / tickHeartbeat (raft.go:645-684), the MsgBeat and
// MsgCheckQuorum steps of stepLeader (raft.go:994-1018) and the part of
// becomeFollower -> reset (raft.go:590-619) that touches the tick's fields.
//
// One kernel in the span-tile shape (qb_span_tile.h), with two slot phases:
//   P1  thread per group: role and timers; a non-leader finishes here
//       (tickElection).  A leader decides whether this tick sweeps
//       (electionElapsed >= election_timeout with check_quorum) and whether
//       it may beat, loads only the group words those need, and claims its
//       slots.
//   P2  (only if a group of the tile sweeps) the span's pstate bytes of
//       sweeping groups, kept in LDS and folded into the group's 16-bit
//       RecentActive mask (LDS atomic OR).
//   P3  thread per group: QuorumActive on the mask (tracker.go:215-225),
//       step-down, transfer abort, beat; timers, role, meta, tflags, hb_ctx
//       written; committed / leader slot / slot action left in LDS.
//   P4  the span again: RecentActive bytes that change are stored, and
//       beating groups read match and write hb_commit.
// A tile whose groups fire nothing (no sweep, no beat) skips P2 and P4 and
// their barriers: it reads no slot data.
//
// The owner map is written out here, not taken from SpanOwners: with its LDS
// arrays regrouped into that struct and find() in the two loops this kernel
// measured 2 us (1.5 %) slower per tick in each of four alternating rounds,
// with claim() after the first barrier as well 3 %.  The guard, the claim loop
// and the stale-owner rule below are those of SpanOwners::claim and ::find; a
// change to either is made here too.
#include "qb_span_tile.h"

namespace qb {
namespace tick {

// slot actions of a group (LDS, one byte per group of the tile)
constexpr u8 kActSweep = 1;   // P2: collect RecentActive; P4: clear it
constexpr u8 kActBeat = 2;    // P4: hb_commit
constexpr u8 kActDown = 4;    // P4: the leader's own bit is cleared too

struct Args {
  qb_tick_groups tg;
  u8* tflags;
  u64* hb_commit;
  u64* hb_ctx;
  u64* stats;
};

struct Tile {
  u8 owner[kSpanCap];   // slot of the span -> thread (group) of the tile
  u8 st[kSpanCap];      // pstate bytes of sweeping groups
  u64 committed[kBlock];
  u32 active[kBlock];   // RecentActive bits by slot
  u32 j0[kBlock];       // the group's first slot within the span
  u8 ns[kBlock];        // its slot count (<= QB_MAX_SLOTS)
  u8 act[kBlock];       // kAct*
  u8 lead[kBlock];      // leader slot, 0xFF = the leader has no Progress
  u32 tally[QB_TSTAT_COUNT];
};

__global__ __launch_bounds__(kBlock) void k_tick(Args A) {
  __shared__ Tile T;
  const qb_tick_groups& tg = A.tg;
  const u64 G = tg.G;
  const u64 ntiles = (G + kBlock - 1) / kBlock;
  const u32 tid = threadIdx.x;
  const u32 et = tg.election_timeout, ht = tg.heartbeat_timeout;
  const bool cq = tg.check_quorum != 0;
  const u64* __restrict__ match = reinterpret_cast<const u64*>(tg.match);
  BlockTally<QB_TSTAT_COUNT> tally;
  if (tid < QB_TSTAT_COUNT) T.tally[tid] = 0;

  for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    SpanTile S(tile, G);
    const u64 g = S.g0 + tid;
    const bool live = g < G;

    // ------------------------------------------------------------- P1 ---
    // Every group word the common tick needs is requested at once (one HBM
    // round trip, not a chain role -> counters -> meta -> committed); only
    // cfg (sweep ticks), rand_timeout (promotable non-leaders) and the read
    // queue's newest context (a beat with pending reads) wait for them.
    u32 s0 = 0, ns = 0, ee = 0, he = 0, meta = 0, cfg = 0;
    u64 com = 0;
    u8 role = 0, tf = 0, act = 0;
    bool leader = false, sweep = false;
    if (live) {
      role = tg.role[g];
      ee = tg.election_elapsed[g] + 1;
      he = tg.heartbeat_elapsed[g] + 1;
      s0 = tg.off[g];
      const u32 s1 = tg.off[g + 1];
      meta = tg.meta[g];
      com = reinterpret_cast<const u64*>(tg.committed)[g];
      ns = clamp_slots(s0, s1);
      leader = (role & 3u) == QB_ROLE_LEADER;
    }
    const u32 sb = tg.off[S.g0];
    if (live && !leader) {  // tickElection, raft.go:645-654
      if ((role & QB_ROLE_PROMOTABLE) && ee >= tg.rand_timeout[g]) {  // raft.go:648, 1714-1716
        ee = 0;
        tf = QB_TFLAG_HUP;
      }
      tg.election_elapsed[g] = ee;
      A.tflags[g] = tf;
    }
    if (leader) {  // tickHeartbeat, raft.go:657-684
      sweep = ee >= et;
      if (sweep && cq) {
        cfg = tg.cfg[g];
        act = kActSweep;
      }
      if (he >= ht) act |= kActBeat;  // (withdrawn in P3 if the leader steps down)
    }
    S.bound(sb, tg.off[S.gend]);
    const u32 span = S.span;
    const bool staged = S.staged;
    const u32 j0 = s0 - sb;
    // a staged group's slots lie inside the span for any monotone off; one
    // that does not (a malformed table) acts on no slot
    if (staged && act && !(s0 >= sb && j0 <= span && ns <= span - j0)) ns = 0;
    const bool fires = __syncthreads_or(act != 0);  // (also: the previous tile's LDS is free)
    u32 active = 0;
    if (fires) {
      if (staged && act) {
        T.j0[tid] = j0;
        T.ns[tid] = u8(ns);
        T.active[tid] = 0;
        for (u32 k = 0; k < ns; ++k) T.owner[j0 + k] = u8(tid);
      }
      T.act[tid] = act;
      // ----------------------------------------------------------- P2 ---
      const bool anysweep = __syncthreads_or((act & kActSweep) != 0);
      if (anysweep) {
        if (staged) {
          // four slots per thread and trip: the loads are issued together
          for (u32 jb = tid; jb < span; jb += kBlock * kSpanUnroll) {
            u32 own_t[kSpanUnroll], bit[kSpanUnroll];
            u8 st[kSpanUnroll];
            bool on[kSpanUnroll];
#pragma unroll
            for (u32 u = 0; u < kSpanUnroll; ++u) {
              const u32 j = jb + u * kBlock;
              on[u] = false;
              st[u] = 0;
              if (j < span) {
                // a slot no acting group owns holds a stale owner byte: the
                // named owner's own range decides
                const u32 t = T.owner[j];
                const u32 k = j - T.j0[t];
                on[u] = (T.act[t] & kActSweep) && k < T.ns[t];
                own_t[u] = t;
                bit[u] = 1u << (k & 15u);
                if (on[u]) st[u] = tg.pstate[u64(sb) + j];
              }
            }
#pragma unroll
            for (u32 u = 0; u < kSpanUnroll; ++u) {
              if (!on[u]) continue;
              T.st[jb + u * kBlock] = st[u];
              if (st[u] & QB_PR_RECENT_ACTIVE) atomicOr(&T.active[own_t[u]], bit[u]);
            }
          }
          __syncthreads();
          if (act & kActSweep) active = T.active[tid];
        } else if (act & kActSweep) {
          for (u32 k = 0; k < ns; ++k)
            if (tg.pstate[u64(s0) + k] & QB_PR_RECENT_ACTIVE) active |= 1u << k;
        }
      }
    }

    // ------------------------------------------------------------- P3 ---
    bool beat = false;
    u32 nhb = 0;
    const u32 ls = meta_own_slot(meta) < ns ? meta_own_slot(meta) : 0xFFu;  // raft.go:1004: own Progress
    if (leader) {
      bool down = false;
      if (sweep) {  // raft.go:661
        ee = 0;
        if (cq) {  // raft.go:663-667 -> raft.go:997-1018
          tf |= QB_TFLAG_CHECK_QUORUM;
          if (ls != 0xFFu) active |= 1u << ls;
          down = !quorum_active(cfg, active);  // raft.go:1007-1010
        }
        if (down) {  // becomeFollower(r.Term, None) -> reset, raft.go:590-619
          role = u8(role & ~3u);  // QB_ROLE_FOLLOWER
          he = 0;
          tf |= QB_TFLAG_STEPPED_DOWN;
          if (meta_transferee(meta) != 0xFFu) tg.meta[g] = meta | 0xFF00u;
          tg.role[g] = role;
          act = kActSweep | kActDown;  // no beat: raft.go:674-676
        } else if (meta_transferee(meta) != 0xFFu) {  // raft.go:669-671
          tg.meta[g] = meta | 0xFF00u;
          tf |= QB_TFLAG_TRANSFER_ABORTED;
        }
      }
      beat = !down && he >= ht;  // raft.go:678-683
      if (beat) {
        he = 0;
        tf |= QB_TFLAG_BEAT;
        nhb = ns - (ls != 0xFFu ? 1u : 0u);
        // bcastHeartbeat, raft.go:524-531: lastPendingRequestCtx
        u32 nq = meta_readq_len(meta);
        if (nq > tg.readq_cap) nq = tg.readq_cap;
        A.hb_ctx[g] = nq ? reinterpret_cast<const u64*>(tg.rq_ctx)[g * tg.readq_cap + nq - 1] : 0ull;
      }
      tg.election_elapsed[g] = ee;
      tg.heartbeat_elapsed[g] = he;
      A.tflags[g] = tf;
    }

    // ------------------------------------------------------------- P4 ---
    if (fires) {
      if (staged && act) {
        T.lead[tid] = u8(ls);
        T.committed[tid] = com;
        T.act[tid] = act;
      }
      __syncthreads();
      if (staged) {
        for (u32 jb = tid; jb < span; jb += kBlock * kSpanUnroll) {
          u64 m[kSpanUnroll], c[kSpanUnroll];
          u8 op[kSpanUnroll], nst[kSpanUnroll];  // op: 1 store the state byte, 2 store the heartbeat
#pragma unroll
          for (u32 u = 0; u < kSpanUnroll; ++u) {
            const u32 j = jb + u * kBlock;
            op[u] = 0;
            if (j >= span) continue;
            const u32 t = T.owner[j];
            const u8 a = T.act[t];
            const u32 k = j - T.j0[t];
            if (!a || k >= T.ns[t]) continue;
            const bool own = k == T.lead[t];
            if (a & kActSweep) {  // raft.go:1011-1017; a step-down clears them all
              const u8 st = T.st[j];
              nst[u] = (own && !(a & kActDown)) ? u8(st | QB_PR_RECENT_ACTIVE)
                                                : u8(st & ~QB_PR_RECENT_ACTIVE);
              if (nst[u] != st) op[u] = 1;
            }
            if ((a & kActBeat) && !own) {  // sendHeartbeat, raft.go:495-511
              op[u] |= 2;
              c[u] = T.committed[t];
              m[u] = __builtin_nontemporal_load(match + u64(sb) + j);
            }
          }
#pragma unroll
          for (u32 u = 0; u < kSpanUnroll; ++u) {
            const u64 j = u64(sb) + jb + u * kBlock;
            if (op[u] & 1) tg.pstate[j] = nst[u];
            if (op[u] & 2) __builtin_nontemporal_store(m[u] < c[u] ? m[u] : c[u], A.hb_commit + j);
          }
        }
      } else if (act) {
        for (u32 k = 0; k < ns; ++k) {
          const bool own = k == ls;
          if (act & kActSweep) {
            const u8 st = tg.pstate[u64(s0) + k];
            const u8 nst = (own && !(act & kActDown)) ? u8(st | QB_PR_RECENT_ACTIVE)
                                                      : u8(st & ~QB_PR_RECENT_ACTIVE);
            if (nst != st) tg.pstate[u64(s0) + k] = nst;
          }
          if ((act & kActBeat) && !own) {
            const u64 m = match[u64(s0) + k];
            A.hb_commit[u64(s0) + k] = m < com ? m : com;
          }
        }
      }
    }
    tally.add_n(QB_TSTAT_HEARTBEATS, nhb);
    tally.add(QB_TSTAT_LEADERS, leader);
    tally.add(QB_TSTAT_NON_LEADERS, live && !leader);
    tally.add(QB_TSTAT_BEATS, (tf & QB_TFLAG_BEAT) != 0);
    tally.add(QB_TSTAT_CHECK_QUORUM, (tf & QB_TFLAG_CHECK_QUORUM) != 0);
    tally.add(QB_TSTAT_STEPPED_DOWN, (tf & QB_TFLAG_STEPPED_DOWN) != 0);
    tally.add(QB_TSTAT_TRANSFER_ABORTED, (tf & QB_TFLAG_TRANSFER_ABORTED) != 0);
    tally.add(QB_TSTAT_HUPS, (tf & QB_TFLAG_HUP) != 0);
  }
  __syncthreads();  // T.tally zeroed; the last tile's LDS reads done
  tally.stage(T.tally);
  __syncthreads();
  BlockTally<QB_TSTAT_COUNT>::publish(T.tally, reinterpret_cast<u64*>(A.stats));
}

}  // namespace tick
}  // namespace qb

using namespace qb;

extern "C" int qb_dev_leader_tick(const qb_tick_groups* tg, uint8_t* tflags, uint64_t* hb_commit,
                                  uint64_t* hb_ctx, uint64_t* stats, void* stream) {
  QB_REQUIRE(tg, "qb_dev_leader_tick: tg is NULL");
  QB_REQUIRE(tg->readq_cap <= QB_LEADER_MAX_READQ, "qb_dev_leader_tick: readq_cap %u > %d",
             tg->readq_cap, QB_LEADER_MAX_READQ);
  QB_REQUIRE(tg->election_timeout >= 1 && tg->heartbeat_timeout >= 1,
             "qb_dev_leader_tick: election_timeout and heartbeat_timeout must be >= 1 (got %u, %u)",
             tg->election_timeout, tg->heartbeat_timeout);
  QB_REQUIRE(tg->check_quorum <= 1, "qb_dev_leader_tick: check_quorum must be 0 or 1 (got %u)",
             tg->check_quorum);
  if (tg->G == 0) return QB_OK;
  QB_REQUIRE(tg->off && tg->cfg && tg->meta && tg->committed && tg->match && tg->pstate &&
                 tg->role && tg->election_elapsed && tg->heartbeat_elapsed && tg->rand_timeout,
             "qb_dev_leader_tick: required group pointer is NULL");
  QB_REQUIRE(tflags && hb_commit && hb_ctx && stats,
             "qb_dev_leader_tick: required output pointer is NULL (tflags / hb_commit / hb_ctx / stats)");
  QB_REQUIRE(tg->rq_ctx || tg->readq_cap == 0, "qb_dev_leader_tick: rq_ctx is NULL with readq_cap %u",
             tg->readq_cap);
  tick::Args A{*tg, tflags, reinterpret_cast<u64*>(hb_commit), reinterpret_cast<u64*>(hb_ctx),
               reinterpret_cast<u64*>(stats)};
  hipLaunchKernelGGL(tick::k_tick, dim3(stream_grid<tick::k_tick>(tg->G)), dim3(kBlock), 0,
                     as_stream(stream), A);
  QB_CHECK_LAUNCH("k_tick");
  return QB_OK;
}
