// qb_campaign.hip — the state changes of an election for G groups at once
// (qb_dev_campaign): Step(MsgHup) -> hup -> campaign -> becomePreCandidate /
// becomeCandidate -> poll self -> vote requests (raft.go:760-845), and
// becomeLeader (+ bcastAppend) / becomeFollower once the tally is in
// (raft.go:1399-1414, 724-758, 686-693), with reset (raft.go:590-619) over
// every field the engine's arrays hold.
//
// One kernel in the span-tile shape (qb_span_tile.h):
//   P1  thread per group: the action byte first; a group with nothing to do
//       writes its cflags / req_type bytes and is done.  An acting group
//       requests all its group words at once (one HBM round trip), runs the
//       transition in registers and writes the group words that changed.  A
//       group whose transition runs reset claims its slots and leaves its
//       recipe in LDS: own slot, last_index, leader / bcastAppend bits.
//   P2  (only if a group of the tile resets) match, next, pending_snapshot,
//       pstate and infl_pos of the claimed slots are written.  Reset reads no
//       slot: the phase is write-only.
#include "qb_span_tile.h"

namespace qb {
namespace campaign {

// a resetting group's recipe (LDS, one byte per group of the tile)
constexpr u8 kReset = 1;   // reset ran: the group's slots are rewritten
constexpr u8 kLeader = 2;  // becomeLeader: the own slot replicates at last_index + 1
constexpr u8 kBcast = 4;   // bcastAppend: every other slot has its probe in flight

struct Args {
  qb_campaign_groups cg;
  const u8* action;
  u8* cflags;
  u8* req_type;
  u64* req_term;
  u16* req_mask;
  u64* stats;
};

struct Tile {
  SpanOwners slots;
  u64 last[kBlock];    // last_index at entry
  u8 fl[kBlock];       // kReset | kLeader | kBcast; 0: the group's slots stay
  u8 own[kBlock];      // own slot, 0xFF = the node has no Progress
  u32 tally[QB_CSTAT_COUNT];
};

// What reset / becomeLeader / bcastAppend leave in slot k of a group.
struct SlotImage {
  u64 match, next;
  u8 st;
};
__device__ __forceinline__ SlotImage slot_image(u8 fl, bool own, u64 last) {
  SlotImage s;
  s.match = own ? last : 0ull;  // raft.go:605-613
  s.next = last + 1;
  s.st = QB_PR_PROBE;
  if (own && (fl & kLeader)) {
    // BecomeReplicate (progress.go:133-137), then MaybeUpdate(last + 1)
    // (raft.go:638, progress.go:146-157)
    const u64 n = last + 1;
    if (s.match < n) s.match = n;
    if (s.next < n + 1) s.next = n + 1;
    s.st = QB_PR_REPLICATE;
  } else if (!own && (fl & kBcast)) {
    s.st = u8(QB_PR_PROBE | QB_PR_PROBE_SENT);  // raft.go:476-490
  }
  return s;
}

__global__ __launch_bounds__(kBlock) void k_campaign(Args A) {
  __shared__ Tile T;
  const qb_campaign_groups& cg = A.cg;
  const u64 G = cg.G;
  const u64 ntiles = (G + kBlock - 1) / kBlock;
  const u32 tid = threadIdx.x;
  const bool pre_vote = cg.pre_vote != 0;
  u64* __restrict__ term_a = reinterpret_cast<u64*>(cg.term);
  u64* __restrict__ vote_a = reinterpret_cast<u64*>(cg.vote);
  u64* __restrict__ lead_a = reinterpret_cast<u64*>(cg.lead);
  u64* __restrict__ com_a = reinterpret_cast<u64*>(cg.committed);
  u64* __restrict__ match_a = reinterpret_cast<u64*>(cg.match);
  u64* __restrict__ next_a = reinterpret_cast<u64*>(cg.next);
  u64* __restrict__ psnap_a = reinterpret_cast<u64*>(cg.pending_snapshot);
  BlockTally<QB_CSTAT_COUNT> tally;
  if (tid < QB_CSTAT_COUNT) T.tally[tid] = 0;

  for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    SpanTile S(tile, G);
    const u64 g = S.g0 + tid;
    const bool live = g < G;
    const u32 sb = cg.off[S.g0], se = cg.off[S.gend];  // the tile's span (used in P2 only)

    // ------------------------------------------------------------- P1 ---
    const u8 action = live ? A.action[g] : u8(0);
    const u32 code = action & 0x7Fu;
    const bool bad = code > QB_CAMP_LOST;
    const bool acts = code != QB_CAMP_NONE && !bad;
    u32 s0 = 0, ns = 0, own = 0xFFu, npre = 0, ncamp = 0, nreq = 0;
    u64 last = 0;
    u8 fl = 0, cf = 0, rt = 0;
    bool ign_leader = false, ign_unprom = false, ign_conf = false, ign_role = false;
    bool now_leader = false, now_follower = false;
    if (acts) {
      // every group word of the transition, requested together
      u8 role = cg.role[g];
      const u32 meta = cg.meta[g];
      const u32 cfg = cg.cfg[g];
      s0 = cg.off[g];
      const u32 s1 = cg.off[g + 1];
      const u64 term0 = term_a[g], vote0 = vote_a[g], com0 = com_a[g];
      const u64 self = reinterpret_cast<const u64*>(cg.self_id)[g];
      last = reinterpret_cast<const u64*>(cg.last_index)[g];
      ns = clamp_slots(s0, s1);
      const u32 min_ = cfg_incoming(cfg), mout = cfg_outgoing(cfg), voters = min_ | mout;
      const u32 oslot = meta_own_slot(meta);
      own = oslot < ns ? oslot : 0xFFu;
      const u32 ownbit = oslot < 16u ? 1u << oslot : 0u;
      const u32 state = role & 3u;
      const bool candidate = state == QB_ROLE_CANDIDATE || state == QB_ROLE_PRE_CANDIDATE;
      u64 term = term0, vote = vote0, com = com0, rterm = 0;

      // which transition: 1 pre-campaign, 2 campaign, 3 transfer campaign,
      // 4 becomeLeader + bcastAppend, 5 becomeFollower, 6 becomeLeader
      u32 what = 0;
      if (code == QB_CAMP_HUP || code == QB_CAMP_TRANSFER) {  // hup, raft.go:760-781
        const bool promotable = (role & QB_ROLE_PROMOTABLE) && own != 0xFFu && ((voters >> own) & 1u);
        if (state == QB_ROLE_LEADER) ign_leader = true;
        else if (!promotable) ign_unprom = true;
        else if (action & QB_CAMP_PENDING_CONF) ign_conf = true;
        else what = code == QB_CAMP_TRANSFER ? 3u : (pre_vote ? 1u : 2u);
      } else if (!candidate) {
        ign_role = true;
      } else if (code == QB_CAMP_WON) {  // raft.go:1402-1409
        what = state == QB_ROLE_PRE_CANDIDATE ? 2u : 4u;
      } else {  // raft.go:1410-1413
        what = 5u;
      }

      const u32 selfvote = ownbit | ownbit << 16;  // poll(r.id, ..., true), raft.go:803
      const bool self_wins = masks_vote(min_, mout, ownbit, ownbit) == QB_VOTE_WON;
      if (what == 1u) {  // becomePreCandidate, raft.go:708-722
        role = u8((role & ~3u) | QB_ROLE_PRE_CANDIDATE);
        npre = 1;
        if (self_wins) {
          what = 2u;  // raft.go:806-807
        } else {
          rt = QB_MSG_PREVOTE;
          rterm = term + 1;  // raft.go:797
        }
      }
      if (what == 2u || what == 3u) {  // becomeCandidate, raft.go:695-706
        term = term + 1;  // reset(r.Term + 1): the term differs
        vote = self;
        fl = kReset;
        role = u8((role & ~3u) | QB_ROLE_CANDIDATE);
        ncamp = 1;
        if (self_wins) {
          what = 6u;  // raft.go:808-809
        } else {
          rt = u8(QB_MSG_VOTE | (what == 3u ? QB_CREQ_TRANSFER : 0u));
          rterm = term;
        }
      }
      u64 lead = 0;  // every become sets it; reset: None
      if (what == 4u || what == 6u) {  // becomeLeader, raft.go:724-758
        fl = u8(kReset | kLeader | (what == 4u ? kBcast : 0));
        lead = self;
        role = u8((role & ~3u) | QB_ROLE_LEADER);
        now_leader = true;
        cf |= QB_CFLAG_BECAME_LEADER;
        if (what == 4u) cf |= QB_CFLAG_BCAST_APPEND;
        // maybeCommit (raft.go:585-588) with only the own Progress at the new
        // entry: every non-empty half must be {own}
        const bool alone = own != 0xFFu && voters != 0 && (min_ == 0 || min_ == ownbit) &&
                           (mout == 0 || mout == ownbit);
        if (alone && last + 1 > com) com = last + 1;
      }
      if (what == 5u) {  // becomeFollower(r.Term, None), raft.go:686-693
        fl = kReset;
        role = u8(role & ~3u);
        now_follower = true;
      }

      if (what) {
        if (rt) {
          const u32 mask = voters & ~ownbit;
          nreq = u32(__builtin_popcount(mask));
          A.req_term[g] = rterm;
          A.req_mask[g] = u16(mask);
          cf |= QB_CFLAG_REQUESTS;
        }
        if (fl) {  // reset, raft.go:590-619
          cf |= QB_CFLAG_RESET;
          cg.election_elapsed[g] = 0;
          cg.heartbeat_elapsed[g] = 0;
          const u32 nmeta = (meta | 0xFF00u) & ~(0x1Fu << 20);
          if (nmeta != meta) cg.meta[g] = nmeta;
        }
        cg.votes[g] = (now_leader || now_follower) ? 0u : selfvote;
        cg.role[g] = role;
        lead_a[g] = lead;
        if (term != term0) term_a[g] = term;
        if (vote != vote0) vote_a[g] = vote;
        if (com != com0) com_a[g] = com;
        if (term != term0 || vote != vote0 || com != com0) cf |= QB_CFLAG_HARDSTATE;
      } else {
        cf = QB_CFLAG_IGNORED;
      }
    }
    if (live) {
      A.cflags[g] = cf;
      A.req_type[g] = rt;
    }

    // ------------------------------------------------------------- P2 ---
    const bool fires = __syncthreads_or(fl != 0);  // (also: the previous tile's LDS is free)
    if (fires) {
      S.bound(sb, se);
      if (S.staged) {
        if (fl) {
          ns = T.slots.claim(S, s0, ns);
          T.own[tid] = u8(own);
          T.last[tid] = last;
        }
        T.fl[tid] = fl;
        __syncthreads();
        for (u32 jb = tid; jb < S.span; jb += kBlock * kSpanUnroll) {
#pragma unroll
          for (u32 u = 0; u < kSpanUnroll; ++u) {
            const u32 j = jb + u * kBlock;
            if (j >= S.span) continue;
            const SpanOwners::Slot o = T.slots.find(j);
            const u32 t = o.t;
            const u8 f = T.fl[t];
            if (!f || !o.in) continue;
            const SlotImage s = slot_image(f, o.k == T.own[t], T.last[t]);
            const u64 i = u64(S.sb) + j;
            __builtin_nontemporal_store(s.match, match_a + i);
            __builtin_nontemporal_store(s.next, next_a + i);
            __builtin_nontemporal_store(0ull, psnap_a + i);
            cg.pstate[i] = s.st;
            __builtin_nontemporal_store(0u, cg.infl_pos + i);
          }
        }
      } else if (fl) {
        for (u32 k = 0; k < ns; ++k) {
          const SlotImage s = slot_image(fl, k == own, last);
          const u64 i = u64(s0) + k;
          match_a[i] = s.match;
          next_a[i] = s.next;
          psnap_a[i] = 0;
          cg.pstate[i] = s.st;
          cg.infl_pos[i] = 0;
        }
      }
    }
    tally.add_n(QB_CSTAT_VOTE_REQUESTS, nreq);
    tally.add(QB_CSTAT_PRE_CAMPAIGNS, npre != 0);
    tally.add(QB_CSTAT_CAMPAIGNS, ncamp != 0);
    tally.add(QB_CSTAT_BECAME_LEADER, now_leader);
    tally.add(QB_CSTAT_BECAME_FOLLOWER, now_follower);
    tally.add(QB_CSTAT_IGNORED_LEADER, ign_leader);
    tally.add(QB_CSTAT_IGNORED_UNPROMOTABLE, ign_unprom);
    tally.add(QB_CSTAT_IGNORED_PENDING_CONF, ign_conf);
    tally.add(QB_CSTAT_IGNORED_ROLE, ign_role);
    tally.add(QB_CSTAT_BAD_ACTION, live && bad);
  }
  __syncthreads();  // T.tally zeroed; the last tile's LDS reads done
  tally.stage(T.tally);
  __syncthreads();
  BlockTally<QB_CSTAT_COUNT>::publish(T.tally, reinterpret_cast<u64*>(A.stats));
}

}  // namespace campaign
}  // namespace qb

using namespace qb;

extern "C" int qb_dev_campaign(const qb_campaign_groups* cg, const uint8_t* action, uint8_t* cflags,
                               uint8_t* req_type, uint64_t* req_term, uint16_t* req_mask,
                               uint64_t* stats, void* stream) {
  QB_REQUIRE(cg, "qb_dev_campaign: cg is NULL");
  QB_REQUIRE(cg->pre_vote <= 1, "qb_dev_campaign: pre_vote must be 0 or 1 (got %u)", cg->pre_vote);
  if (cg->G == 0) return QB_OK;
  QB_REQUIRE(cg->off && cg->cfg && cg->meta && cg->self_id && cg->term && cg->vote && cg->lead &&
                 cg->committed && cg->last_index && cg->last_term && cg->role &&
                 cg->election_elapsed && cg->heartbeat_elapsed && cg->votes && cg->match &&
                 cg->next && cg->pending_snapshot && cg->pstate && cg->infl_pos,
             "qb_dev_campaign: required group pointer is NULL");
  QB_REQUIRE(action && cflags && req_type && req_term && req_mask && stats,
             "qb_dev_campaign: required output pointer is NULL (action / cflags / req_type / "
             "req_term / req_mask / stats)");
  campaign::Args A{*cg, action, cflags, req_type, reinterpret_cast<u64*>(req_term), req_mask,
                   reinterpret_cast<u64*>(stats)};
  hipLaunchKernelGGL(campaign::k_campaign, dim3(stream_grid<campaign::k_campaign>(cg->G)),
                     dim3(kBlock), 0, as_stream(stream), A);
  QB_CHECK_LAUNCH("k_campaign");
  return QB_OK;
}
