// qb_follower.hip — raft.Step for the non-leader inbox of G groups at once
// (qb_dev_follower_step): MsgHeartbeat, MsgVote / MsgPreVote and
// MsgTimeoutNow through the term filter (raft.go:847-920), the vote rules
// (raft.go:930-978), stepFollower / stepCandidate (raft.go:1393-1457),
// handleHeartbeat (raft.go:1513-1516) and the part of becomeFollower -> reset
// (raft.go:590-619, 686-693) that touches this call's fields.
//
// A group's records must be applied in batch order, so the batch is grouped
// first (a counting sort by group over the workspace), then stepped:
//   F1 k_count    thread per record: cnt[group]++ (bad group / bad kind are
//                 answered "no message" and dropped here).
//   F2 scan       exclusive prefix of cnt (qb_scan.h): group g's run starts
//                 at cnt[g].
//   F3 k_scatter  thread per record: perm[cnt[group]++] = batch index.  After
//                 it cnt[g] is the END of group g's run (its start is
//                 cnt[g - 1]); the order inside a run is the order the
//                 atomics happened to take.
//   F4 k_step     thread per group: the group's words requested in one round
//                 trip, a run of up to kInline records sorted by batch index
//                 in place, then the records stepped sequentially over
//                 register-held state with the next record's loads in
//                 flight; only what changed is written back.  A group
//                 without records writes gflags 0 / stop_at UINT32_MAX and
//                 touches nothing else.  A longer run is listed for F5.
//   F5 k_long     workgroup per listed group: the run sorted by the whole
//                 workgroup (bitonic; in LDS up to kLdsRun records, beyond
//                 that in the workspace), then stepped by one thread.  This
//                 is also the fallback for any skew: one group may hold the
//                 whole batch.
// Statistics: per-thread counts, summed per wave and per workgroup, one
// global atomic per counter per workgroup; F4's grid is capped (kStepBlocks)
// and strides the tiles so that stays a few thousand atomics.
#include "qb_common.h"
#include "qb_scan.h"

namespace qb {
namespace fol {

constexpr u32 kInline = 16;      // F4 sorts and steps runs up to this itself
constexpr u32 kLdsRun = 4096;    // F5 sorts runs up to this in LDS
constexpr unsigned kStepBlocks = 2048;
constexpr unsigned kLongBlocks = 256;
constexpr u32 kNoStop = 0xFFFFFFFFu;
constexpr int kStepStats = QB_FSTAT_AFTER_STOP + 1;  // the counters F4 / F5 keep
constexpr u64 kMaxM = 0xFFFFFFFEull;

struct Args {
  qb_follower_groups fg;
  qb_follower_inbox in;
  u8* resp_type;
  u64* resp_term;
  u32* stop_at;
  u8* gflags;
  u64* stats;
  u32* cnt;    // [G + 1] counts -> run starts -> run ends
  u32* perm;   // [M] batch indices, grouped
  u32* longs;  // [M / (kInline + 1) + 1] groups with a run past kInline
  u32* nlong;
};

// a record F4 / F5 step: in range and of a known kind
__device__ __forceinline__ bool rec_ok(const Args& A, u64 i, u32& g, bool& badg, bool& badk) {
  g = A.in.group[i];
  const u32 kind = A.in.flags[i] & QB_FREC_KIND_MASK;
  badg = u64(g) >= A.fg.G;
  badk = !badg && kind > QB_FIN_HOST;
  return !badg && !badk;
}

__global__ __launch_bounds__(kBlock) void k_count(Args A) {
  __shared__ u32 sh[2];
  const u64 i = u64(blockIdx.x) * kBlock + threadIdx.x;
  bool badg = false, badk = false;
  if (i < A.in.M) {
    u32 g;
    if (rec_ok(A, i, g, badg, badk)) {
      atomicAdd(A.cnt + g, 1u);
    } else {
      A.resp_type[i] = 0;
      A.resp_term[i] = 0;
    }
  }
  BlockTally<2> t;
  t.add(0, badg);
  t.add(1, badk);
  const int slot[2] = {QB_FSTAT_BAD_GROUP, QB_FSTAT_BAD_KIND};
  t.flush(sh, A.stats, slot);
}

__global__ __launch_bounds__(kBlock) void k_scatter(Args A) {
  const u64 i = u64(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= A.in.M) return;
  u32 g;
  bool badg, badk;
  if (!rec_ok(A, i, g, badg, badk)) return;
  const u32 pos = atomicAdd(A.cnt + g, 1u);
  if (u64(pos) < A.in.M) A.perm[pos] = u32(i);  // (always, for a batch that does not change under the call)
}

struct Rec {
  u64 from, term, index, aux;
  u8 fl;
};
__device__ __forceinline__ Rec load_rec(const qb_follower_inbox& in, u32 i) {
  Rec r;
  r.fl = in.flags[i];
  r.from = reinterpret_cast<const u64*>(in.from)[i];
  r.term = reinterpret_cast<const u64*>(in.term)[i];
  r.index = reinterpret_cast<const u64*>(in.index)[i];
  r.aux = reinterpret_cast<const u64*>(in.aux)[i];
  return r;
}

// Group g's run (n >= 1 batch indices, ascending) stepped in order.
__device__ __forceinline__ void step_group(const Args& A, u64 g, const u32* run, u32 n,
                                           u32 (&c)[kStepStats]) {
  const qb_follower_groups& fg = A.fg;
  u64* gterm = reinterpret_cast<u64*>(fg.term);
  u64* gvote = reinterpret_cast<u64*>(fg.vote);
  u64* glead = reinterpret_cast<u64*>(fg.lead);
  u64* gcom = reinterpret_cast<u64*>(fg.committed);
  // every word of the group and the first record in one round trip
  Rec nx = load_rec(A.in, run[0]);
  const u64 term0 = gterm[g], vote0 = gvote[g], lead0 = glead[g], com0 = gcom[g];
  const u64 li = reinterpret_cast<const u64*>(fg.last_index)[g];
  const u64 lt = reinterpret_cast<const u64*>(fg.last_term)[g];
  const u8 role0 = fg.role[g];
  const u32 ee0 = fg.election_elapsed[g];
  const u32 et = fg.election_timeout;
  const bool cq = fg.check_quorum != 0, pv = fg.pre_vote != 0;
  u64 term = term0, vote = vote0, lead = lead0, com = com0;
  u8 role = role0, gf = 0;
  u32 ee = ee0, stop = kNoStop;

  // becomeFollower(t, l) -> reset(t), raft.go:686-693, 590-619
  auto become_follower = [&](u64 t, u64 l) {
    if (term != t) {  // raft.go:591-594
      term = t;
      vote = 0;
    }
    lead = l;          // raft.go:595, 690
    ee = 0;            // raft.go:597 (heartbeatElapsed: written below)
    role = u8(role & ~3u);  // raft.go:691, QB_ROLE_FOLLOWER
    gf |= QB_FFLAG_RESET;
    ++c[QB_FSTAT_BECAME_FOLLOWER];
  };

  u32 k = 0;
  for (; k < n && stop == kNoStop; ++k) {
    const u32 i = run[k];
    const Rec r = nx;
    if (k + 1 < n) nx = load_rec(A.in, run[k + 1]);
    const u32 kind = r.fl & QB_FREC_KIND_MASK;
    const bool is_vote = kind == QB_FIN_VOTE || kind == QB_FIN_PREVOTE;
    u8 rt = 0;
    u64 rterm = 0;
    const bool higher = r.term != 0 && r.term > term;  // raft.go:850-852
    if (kind == QB_FIN_HOST) {
      stop = i;
      gf |= QB_FFLAG_HOST_MSG;
    } else if (r.term != 0 && r.term < term) {  // raft.go:883-919
      if ((cq || pv) && kind == QB_FIN_HEARTBEAT) {
        rt = QB_FRESP_APP_RESP;  // raft.go:906
        rterm = term;
        ++c[QB_FSTAT_STALE_ANSWERED];
      } else if (kind == QB_FIN_PREVOTE) {
        rt = QB_FRESP_PREVOTE_RESP | QB_FRESP_REJECT;  // raft.go:913
        rterm = term;
        ++c[QB_FSTAT_STALE_ANSWERED];
      } else {
        ++c[QB_FSTAT_STALE_IGNORED];
      }
    } else if (higher && is_vote && !(r.fl & QB_FREC_FORCE) && cq && lead != 0 && ee < et) {
      ++c[QB_FSTAT_LEASE_DROPPED];  // raft.go:853-862
    } else if (kind == QB_FIN_HEARTBEAT && (higher || (role & 3u) != QB_ROLE_LEADER) &&
               com < r.index && li < r.index) {
      stop = i;  // commitTo would panic, log.go:236-244: nothing of the record is applied
      gf |= QB_FFLAG_COMMIT_RANGE;
    } else {
      if (higher && kind != QB_FIN_PREVOTE)  // raft.go:864-881
        become_follower(r.term, kind == QB_FIN_HEARTBEAT ? r.from : 0ull);
      if (is_vote) {  // raft.go:930-978
        const bool can_vote = vote == r.from || (vote == 0 && lead == 0) ||
                              (kind == QB_FIN_PREVOTE && r.term > term);
        const bool up_to_date = r.aux > lt || (r.aux == lt && r.index >= li);  // log.go:316-318
        rt = kind == QB_FIN_VOTE ? QB_FRESP_VOTE_RESP : QB_FRESP_PREVOTE_RESP;
        if (can_vote && up_to_date) {
          rterm = r.term;  // raft.go:968
          if (kind == QB_FIN_VOTE) {  // raft.go:969-973
            ee = 0;
            vote = r.from;
          }
          ++c[QB_FSTAT_GRANTED];
        } else {
          rt |= QB_FRESP_REJECT;  // raft.go:977
          rterm = term;
          ++c[QB_FSTAT_REJECTED];
        }
      } else if (kind == QB_FIN_HEARTBEAT) {
        if ((role & 3u) == QB_ROLE_LEADER) {  // stepLeader has no case for it
          ++c[QB_FSTAT_ROLE_IGNORED];
        } else {
          if ((role & 3u) != QB_ROLE_FOLLOWER) {  // stepCandidate, raft.go:1393-1395
            become_follower(r.term, r.from);
          } else {  // stepFollower, raft.go:1437-1440
            ee = 0;
            lead = r.from;
          }
          if (com < r.index) com = r.index;  // handleHeartbeat -> commitTo, raft.go:1513-1516
          rt = QB_FRESP_HEARTBEAT_RESP;
          rterm = term;
          ++c[QB_FSTAT_HEARTBEATS];
        }
      } else {  // QB_FIN_TIMEOUT_NOW, raft.go:1415-1416, 1452-1457 -> hup, 760-768
        if ((role & 3u) == QB_ROLE_FOLLOWER && (role & QB_ROLE_PROMOTABLE)) {
          stop = i;
          gf |= QB_FFLAG_CAMPAIGN;
        } else {
          ++c[QB_FSTAT_ROLE_IGNORED];
        }
      }
    }
    A.resp_type[i] = rt;
    A.resp_term[i] = rterm;
  }
  for (; k < n; ++k) {  // behind the stop: the host re-submits them
    const u32 i = run[k];
    A.resp_type[i] = 0;
    A.resp_term[i] = 0;
    ++c[QB_FSTAT_AFTER_STOP];
  }
  if (term != term0) gterm[g] = term;
  if (vote != vote0) gvote[g] = vote;
  if (lead != lead0) glead[g] = lead;
  if (com != com0) gcom[g] = com;
  if (role != role0) fg.role[g] = role;
  if (ee != ee0) fg.election_elapsed[g] = ee;
  if (gf & QB_FFLAG_RESET) fg.heartbeat_elapsed[g] = 0;  // raft.go:598
  if (term != term0 || vote != vote0 || com != com0) gf |= QB_FFLAG_HARDSTATE;
  A.gflags[g] = gf;
  A.stop_at[g] = stop;
}

// group g's run [b, e) of perm after F3; an inconsistent table yields an empty run
__device__ __forceinline__ void run_of(const Args& A, u64 g, u32& b, u32& e) {
  b = g ? A.cnt[g - 1] : 0u;
  e = A.cnt[g];
  if (e < b || u64(e) > A.in.M) e = b = 0;
}

template <int K>
__device__ __forceinline__ void flush_counts(const u32 (&c)[K], u32* lds, u64* stats) {
  BlockTally<K> t;
#pragma unroll
  for (int j = 0; j < K; ++j) t.add_n(j, c[j]);
  int slot[K];
#pragma unroll
  for (int j = 0; j < K; ++j) slot[j] = j;
  t.flush(lds, stats, slot);
}

__global__ __launch_bounds__(kBlock) void k_step(Args A) {
  __shared__ u32 sh[kStepStats];
  const u64 G = A.fg.G;
  const u64 ntiles = (G + kBlock - 1) / kBlock;
  u32 c[kStepStats];
#pragma unroll
  for (int j = 0; j < kStepStats; ++j) c[j] = 0;
  for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const u64 g = tile * kBlock + threadIdx.x;
    if (g >= G) continue;
    u32 b, e;
    run_of(A, g, b, e);
    const u32 n = e - b;
    if (n == 0) {
      A.gflags[g] = 0;
      A.stop_at[g] = kNoStop;
    } else if (n <= kInline) {
      u32* run = A.perm + b;
      for (u32 j = 1; j < n; ++j) {  // insertion sort by batch index
        const u32 v = run[j];
        u32 p = j;
        while (p > 0 && run[p - 1] > v) {
          run[p] = run[p - 1];
          --p;
        }
        if (p != j) run[p] = v;
      }
      step_group(A, g, run, n, c);
    } else {
      const u32 s = atomicAdd(A.nlong, 1u);
      A.longs[s] = u32(g);  // (at most M / (kInline + 1) such groups)
    }
  }
  flush_counts(c, sh, A.stats);
}

// Bitonic sort of v[0, n), ascending, by the whole workgroup.  Every
// comparator is ascending (the first step of each merge mirrors: partner =
// i ^ (2k - 1)), so an element "past n" would never move and its pairs are
// simply skipped: any n, no padding.
template <class Load, class Store>
__device__ __forceinline__ void block_bitonic(u32 n, Load ld, Store st) {
  for (u64 k = 1; k < n; k <<= 1) {  // (u64: n may pass 2^31)
    for (u64 j = k; j >= 1; j >>= 1) {
      const u32 mask = u32(j == k ? 2 * k - 1 : j);
      for (u32 i = threadIdx.x; i < n; i += kBlock) {
        const u32 p = i ^ mask;
        if (p > i && p < n) {
          const u32 a = ld(i), b = ld(p);
          if (a > b) {
            st(i, b);
            st(p, a);
          }
        }
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_long(Args A) {
  __shared__ u32 run[kLdsRun];
  __shared__ u32 sh[kStepStats];
  const u32 nl = *A.nlong;
  u32 c[kStepStats];
#pragma unroll
  for (int j = 0; j < kStepStats; ++j) c[j] = 0;
  for (u32 q = blockIdx.x; q < nl; q += gridDim.x) {
    const u64 g = A.longs[q];
    u32 b, e;
    run_of(A, g, b, e);
    const u32 n = e - b;  // > kInline
    u32* pg = A.perm + b;
    if (n <= kLdsRun) {
      for (u32 i = threadIdx.x; i < n; i += kBlock) run[i] = pg[i];
      __syncthreads();
      block_bitonic(n, [&](u32 i) { return run[i]; }, [&](u32 i, u32 v) { run[i] = v; });
      if (threadIdx.x == 0 && n) step_group(A, g, run, n, c);
    } else {
      // in the workspace: device-scope accesses, so no lane reads a line its
      // CU cached before another wave's store
      __syncthreads();
      block_bitonic(
          n, [&](u32 i) { return __hip_atomic_load(pg + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
          [&](u32 i, u32 v) { __hip_atomic_store(pg + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); });
      __threadfence();
      __syncthreads();
      if (threadIdx.x == 0) step_group(A, g, pg, n, c);
    }
    __syncthreads();  // the LDS run is free for the next group
  }
  flush_counts(c, sh, A.stats);
}

// Workspace: [cnt (G + 1) | nlong] zeroed per call, then the scan's block
// sums, the long-run list and perm.
struct Carve {
  size_t cnt, nlong, zero_end, bsum, longs, perm, total;
};
inline Carve carve(u64 G, u64 M) {
  Carve c{};
  Carver k;
  c.cnt = k.take(sizeof(u32) * (G + 1));
  c.nlong = k.take(256);
  c.zero_end = k.o;
  c.bsum = k.take(sizeof(u32) * (u64(scan::blocks(G)) + 1));
  c.longs = k.take(sizeof(u32) * (M / (kInline + 1) + 1));
  c.perm = k.take(sizeof(u32) * (M ? M : 1));
  c.total = k.o;
  return c;
}

}  // namespace fol
}  // namespace qb

using namespace qb;

extern "C" size_t qb_follower_workspace_bytes(uint64_t G, uint64_t M) {
  if (M > fol::kMaxM || G > 0xFFFFFFFFull) return 0;
  return fol::carve(G, M).total;
}

extern "C" int qb_dev_follower_step(const qb_follower_groups* fg, const qb_follower_inbox* in,
                                    uint8_t* resp_type, uint64_t* resp_term, uint32_t* stop_at,
                                    uint8_t* gflags, uint64_t* stats, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  QB_REQUIRE(fg, "qb_dev_follower_step: fg is NULL");
  QB_REQUIRE(in, "qb_dev_follower_step: in is NULL");
  QB_REQUIRE(fg->election_timeout >= 1, "qb_dev_follower_step: election_timeout must be >= 1 (got %u)",
             fg->election_timeout);
  QB_REQUIRE(fg->check_quorum <= 1, "qb_dev_follower_step: check_quorum must be 0 or 1 (got %u)",
             fg->check_quorum);
  QB_REQUIRE(fg->pre_vote <= 1, "qb_dev_follower_step: pre_vote must be 0 or 1 (got %u)", fg->pre_vote);
  QB_REQUIRE(in->M <= fol::kMaxM, "qb_dev_follower_step: M %llu > 2^32 - 2",
             static_cast<unsigned long long>(in->M));
  QB_REQUIRE(fg->G <= 0xFFFFFFFFull, "qb_dev_follower_step: G %llu > 2^32 - 1 (groups are uint32)",
             static_cast<unsigned long long>(fg->G));
  if (fg->G == 0) return QB_OK;  // every record is a bad group; nothing to initialise
  const u64 G = fg->G, M = in->M;
  QB_REQUIRE(fg->term && fg->vote && fg->lead && fg->committed && fg->last_index && fg->last_term &&
                 fg->role && fg->election_elapsed && fg->heartbeat_elapsed,
             "qb_dev_follower_step: required group pointer is NULL");
  QB_REQUIRE(M == 0 || (in->group && in->flags && in->from && in->term && in->index && in->aux),
             "qb_dev_follower_step: required inbox pointer is NULL");
  QB_REQUIRE(stop_at && gflags && stats && (M == 0 || (resp_type && resp_term)),
             "qb_dev_follower_step: required output pointer is NULL (resp_type / resp_term / "
             "stop_at / gflags / stats)");
  const fol::Carve cv = fol::carve(G, M);
  QB_REQUIRE(workspace, "qb_dev_follower_step: workspace is NULL");
  QB_REQUIRE(workspace_bytes >= cv.total,
             "qb_dev_follower_step: workspace too small: %zu < %zu (qb_follower_workspace_bytes)",
             workspace_bytes, cv.total);
  QB_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0,
             "qb_dev_follower_step: workspace must be 8-byte aligned");
  char* ws = static_cast<char*>(workspace);
  hipStream_t st = as_stream(stream);
  fol::Args A{*fg, *in, resp_type, reinterpret_cast<u64*>(resp_term), stop_at, gflags,
              reinterpret_cast<u64*>(stats), reinterpret_cast<u32*>(ws + cv.cnt),
              reinterpret_cast<u32*>(ws + cv.perm), reinterpret_cast<u32*>(ws + cv.longs),
              reinterpret_cast<u32*>(ws + cv.nlong)};
  hipError_t e = hipMemsetAsync(ws + cv.cnt, 0, cv.zero_end - cv.cnt, st);
  if (e != hipSuccess) return hip_fail(e, "qb_dev_follower_step: memset");
  if (M) {
    hipLaunchKernelGGL(fol::k_count, dim3(grid_for(M)), dim3(kBlock), 0, st, A);
    QB_CHECK_LAUNCH("k_count");
    scan::launch(A.cnt, G, reinterpret_cast<u32*>(ws + cv.bsum), st);
    QB_CHECK_LAUNCH("follower scan");
    hipLaunchKernelGGL(fol::k_scatter, dim3(grid_for(M)), dim3(kBlock), 0, st, A);
    QB_CHECK_LAUNCH("k_scatter");
  }
  const unsigned tiles = grid_for(G);
  hipLaunchKernelGGL(fol::k_step, dim3(tiles < fol::kStepBlocks ? tiles : fol::kStepBlocks),
                     dim3(kBlock), 0, st, A);
  QB_CHECK_LAUNCH("k_step");
  if (M > fol::kInline) {
    const u64 most = M / (fol::kInline + 1);  // groups that can hold a long run
    hipLaunchKernelGGL(fol::k_long, dim3(unsigned(most < fol::kLongBlocks ? most : fol::kLongBlocks)),
                       dim3(kBlock), 0, st, A);
    QB_CHECK_LAUNCH("k_long");
  }
  return QB_OK;
}
