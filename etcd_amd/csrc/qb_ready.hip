// qb_ready.hip — RawNode.HasReady / readyWithoutAccept / acceptReady / Advance
// for G groups (qb_dev_ready, qb_dev_advance) and the unstable offset's share
// of a follower append (qb_dev_unstable_truncate): rawnode.go:125-179,
// newReady / MustSync node.go:564-595, raft.advance raft.go:543-580,
// reduceUncommittedSize raft.go:1783-1801, raftLog log.go:173-205, 246-258,
// unstable log_unstable.go:55-145.
//
// Ready is qb_delta.hip's count / scan / write over a bounded grid:
//   R1 k_ready_flags  thread per group streams the compared columns, writes
//                     rflags[g] and the tile's ready count (wave ballots, the
//                     waves summed through LDS) to cnt[tile]
//   scan              exclusive scan of the tile counts (qb_scan.h)
//   R2 k_ready_write  thread per group reads rflags[g] alone; a ready group's
//                     position is its tile's offset plus the ready groups
//                     before it in the tile (ballots, waves in order); past
//                     ready_cap it is flagged deferred, else it re-reads the
//                     columns its flags name, writes its record and accepts
// R2 re-reads instead of R1 staging records: an idle group then costs 2 bytes
// in R2, and a ready one reads what its flags name (DESIGN.md §3.7k has the
// bytes at both ends).  No workgroup waits on another: the order comes from
// the scan between the launches.
#include "qb_scan.h"
#include "qb_span_tile.h"

namespace qb {
namespace ready {

constexpr u32 kWaves = kBlock / 64;
constexpr u32 kReadyMask = 0xFFFFu & ~(QB_RDF_MUST_SYNC | QB_RDF_DEFERRED);
constexpr u32 kFlagStats = 9;  // QB_RSTAT_SOFT .. QB_RSTAT_BAD_LOG follow the flag bits

static_assert(QB_RDF_SOFT == 1u << QB_RSTAT_SOFT && QB_RDF_BAD_LOG == 1u << QB_RSTAT_BAD_LOG,
              "the flag counters follow the flag bits");

__device__ __forceinline__ const u64* c64(const void* p) { return static_cast<const u64*>(p); }
__device__ __forceinline__ u64* m64(void* p) { return static_cast<u64*>(p); }

// nextEnts' lower bound (log.go:183-184).
__device__ __forceinline__ u64 apply_from(u64 applied, u64 first) {
  const u64 a = applied + 1;
  return a > first ? a : first;
}

// The flags of group g (everything but QB_RDF_DEFERRED).
__device__ __forceinline__ u32 flags_of(const qb_ready_groups& rg, u64 g) {
  // every column requested together: one HBM round trip
  const u64 term = c64(rg.term)[g], vote = c64(rg.vote)[g], com = c64(rg.committed)[g];
  const u64 lead = c64(rg.lead)[g];
  const u64 first = c64(rg.first_index)[g], last = c64(rg.last_index)[g];
  const u64 applied = c64(rg.applied)[g], uoff = c64(rg.unstable_offset)[g];
  const u64 usnap = c64(rg.usnap_index)[g];
  const u64 pterm = c64(rg.prev_term)[g], pvote = c64(rg.prev_vote)[g];
  const u64 pcom = c64(rg.prev_commit)[g], plead = c64(rg.prev_lead)[g];
  const u32 role = rg.role[g], prole = rg.prev_role[g], pend = rg.pending[g];

  const bool has_next = com + 1 > apply_from(applied, first);  // log.go:197-201
  // slice's bound (log.go:384-397) and an offset past the log's end + 1
  if ((has_next && com + 1 > last + 1) || uoff > last + 1) return QB_RDF_BAD_LOG;
  u32 f = 0;
  if (lead != plead || ((role ^ prole) & ~QB_ROLE_PROMOTABLE & 0xFFu)) f |= QB_RDF_SOFT;
  if ((term | vote | com) != 0 && (term != pterm || vote != pvote || com != pcom))
    f |= QB_RDF_HARD;  // rawnode.go:150-152
  if (uoff <= last) f |= QB_RDF_ENTRIES;
  if (usnap != 0) f |= QB_RDF_SNAPSHOT;
  if (has_next) f |= QB_RDF_COMMITTED;
  if (pend & QB_RDP_MSGS) f |= QB_RDF_MSGS;
  if (pend & QB_RDP_READSTATES) f |= QB_RDF_READSTATES;
  if ((f & QB_RDF_ENTRIES) || vote != pvote || term != pterm) f |= QB_RDF_MUST_SYNC;  // node.go:589-595
  return f;
}

__global__ __launch_bounds__(kBlock) void k_ready_flags(qb_ready_groups rg, u16* __restrict__ rflags,
                                                        u32* __restrict__ cnt, u64* stats) {
  __shared__ u32 ws[2][kWaves];
  __shared__ u32 tl[kFlagStats];
  const u64 G = rg.G;
  const u64 ntiles = (G + kBlock - 1) / kBlock;
  const u32 tid = threadIdx.x;
  BlockTally<kFlagStats> tally;
  if (tid < kFlagStats) tl[tid] = 0;
  u32 par = 0;
  for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x, par ^= 1u) {
    const u64 g = tile * kBlock + tid;
    u32 f = 0;
    if (g < G) {
      f = flags_of(rg, g);
      rflags[g] = u16(f);
    }
    const u32 c = wave_popc((f & kReadyMask) != 0);
    if ((tid & 63u) == 0) ws[par][tid >> 6] = c;
#pragma unroll
    for (u32 k = 0; k < kFlagStats; ++k) tally.add(int(k), (f >> k) & 1u);
    __syncthreads();  // one barrier a tile: ws alternates between two rows
    if (tid == 0) {
      u32 t = 0;
#pragma unroll
      for (u32 w = 0; w < kWaves; ++w) t += ws[par][w];
      cnt[tile] = t;
    }
  }
  __syncthreads();  // tl zeroed (a block with no tile passed no barrier)
  tally.stage(tl);
  __syncthreads();
  BlockTally<kFlagStats>::publish(tl, stats);
}

struct WriteArgs {
  qb_ready_groups rg;
  qb_ready_out out;
  u64 cap;
  u64* stats;
  const u32* cnt;
  u32 ntiles;
  int accept;
};

__global__ __launch_bounds__(kBlock) void k_ready_write(WriteArgs A) {
  __shared__ u32 ws[2][kWaves];
  __shared__ u32 tl[2];
  const qb_ready_groups& rg = A.rg;
  const qb_ready_out& o = A.out;
  const u64 G = rg.G;
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  BlockTally<2> tally;  // 0: deferred, 1: listed
  if (tid < 2) tl[tid] = 0;
  if (blockIdx.x == 0 && tid == 0) *o.ready_count = A.cnt[A.ntiles];
  u32 par = 0;
  for (u64 tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x, par ^= 1u) {
    const u64 g = tile * kBlock + tid;
    const bool live = g < G;
    const u32 f = live ? u32(o.rflags[g]) : 0u;
    const bool rdy = (f & kReadyMask) != 0;
    const u64 b = __ballot(rdy);
    if (lane == 0) ws[par][wave] = u32(__popcll(b));
    __syncthreads();
    u32 before = 0;
    for (u32 q = 0; q < wave; ++q) before += ws[par][q];
    const u64 pos = u64(A.cnt[tile]) + before + u32(__popcll(b & ((1ull << lane) - 1ull)));
    const bool listed = rdy && pos < A.cap, deferred = rdy && !listed;
    tally.add(0, deferred);
    tally.add(1, listed);
    if (deferred) o.rflags[g] = u16(f | QB_RDF_DEFERRED);
    if (!listed) continue;
    // the record: only the columns the flags name are read again
    const u64 lead = c64(rg.lead)[g];
    const u8 role = u8(rg.role[g] & ~QB_ROLE_PROMOTABLE);
    u64 ht = 0, hv = 0, hc = 0, el = 0, eh = 0, et = 0, al = 0, ah = 0, sn = 0;
    if (f & (QB_RDF_HARD | QB_RDF_COMMITTED)) hc = c64(rg.committed)[g];
    if (f & QB_RDF_COMMITTED) {
      al = apply_from(c64(rg.applied)[g], c64(rg.first_index)[g]);
      ah = hc;
    }
    if (f & QB_RDF_HARD) {
      ht = c64(rg.term)[g];
      hv = c64(rg.vote)[g];
    } else {
      hc = 0;
    }
    if (f & QB_RDF_ENTRIES) {
      el = c64(rg.unstable_offset)[g];
      eh = c64(rg.last_index)[g];
      et = c64(rg.last_term)[g];
    }
    if (f & QB_RDF_SNAPSHOT) sn = c64(rg.usnap_index)[g];
    o.ready_gid[pos] = u32(g);
    o.rd_flags[pos] = u16(f);
    m64(o.hs_term)[pos] = ht;
    m64(o.hs_vote)[pos] = hv;
    m64(o.hs_commit)[pos] = hc;
    m64(o.ent_lo)[pos] = el;
    m64(o.ent_hi)[pos] = eh;
    m64(o.ent_last_term)[pos] = et;
    m64(o.apply_lo)[pos] = al;
    m64(o.apply_hi)[pos] = ah;
    m64(o.snap_index)[pos] = sn;
    m64(o.lead)[pos] = lead;
    o.role[pos] = role;
    if (A.accept && !(f & QB_RDF_BAD_LOG)) {  // acceptReady, rawnode.go:139-147
      if (f & QB_RDF_SOFT) {
        m64(rg.prev_lead)[g] = lead;
        rg.prev_role[g] = role;
      }
      rg.pending[g] = 0;
    }
  }
  __syncthreads();
  tally.stage(tl);
  __syncthreads();
  if (tid < 2 && tl[tid]) atomicAdd(A.stats + QB_RSTAT_DEFERRED + tid, u64(tl[tid]));
}

static_assert(QB_RSTAT_LISTED == QB_RSTAT_DEFERRED + 1, "k_ready_write's two counters");

// ------------------------------------------------------------- advance ---
struct AdvArgs {
  qb_ready_groups rg;
  qb_advance_in in;
  u64 A;
  u8* aflags;
  u64* stats;
};

__global__ __launch_bounds__(kBlock) void k_advance(AdvArgs P) {
  __shared__ u32 tl[QB_ASTAT_COUNT];
  const qb_ready_groups& rg = P.rg;
  const qb_advance_in& in = P.in;
  const u64 G = rg.G;
  const u32 tid = threadIdx.x;
  BlockTally<QB_ASTAT_COUNT> tally;
  if (tid < QB_ASTAT_COUNT) tl[tid] = 0;
  const u64 ntiles = (P.A + kBlock - 1) / kBlock;
  for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const u64 i = tile * kBlock + tid;
    const bool live = i < P.A;
    const u64 g = live ? u64(in.adv_gid[i]) : 0ull;
    const bool bad = live && g >= G;
    bool range = false, hard = false, appl = false, autol = false, stab = false, stale = false,
         snap = false;
    if (live && !bad) {
      // the record and the group words it meets, requested together
      const u64 ht = c64(in.hs_term)[i], hv = c64(in.hs_vote)[i], hc = c64(in.hs_commit)[i];
      const u64 ato = c64(in.applied_to)[i], pay = c64(in.applied_payload)[i];
      const u64 si = c64(in.stable_index)[i], stt = c64(in.stable_term)[i];
      const u64 ss = c64(in.stable_snap)[i];
      const u64 applied = c64(rg.applied)[g], com = c64(rg.committed)[g];
      range = ato != 0 && (com < ato || ato < applied);  // log.go:250-252
      if (!range) {
        if ((ht | hv | hc) != 0) {  // rawnode.go:174-177
          m64(rg.prev_term)[g] = ht;
          m64(rg.prev_vote)[g] = hv;
          m64(rg.prev_commit)[g] = hc;
          hard = true;
        }
        if (pay != 0) {  // reduceUncommittedSize, raft.go:1783-1801
          const u64 us = c64(rg.uncommitted_size)[g];
          if (us != 0) m64(rg.uncommitted_size)[g] = pay > us ? 0ull : us - pay;
        }
        if (ato != 0) {  // raft.go:550-571
          m64(rg.applied)[g] = ato;
          appl = true;
          if (rg.ext && ((rg.ext[g] >> 16) & 1u)) {
            const u64 pci = c64(rg.pending_conf_index)[g];
            autol = applied <= pci && ato >= pci && (rg.role[g] & 3u) == QB_ROLE_LEADER;
          }
        }
        if (si != 0) {  // stableTo, log_unstable.go:77-89
          const u64 uoff = c64(rg.unstable_offset)[g], last = c64(rg.last_index)[g];
          bool ok = uoff <= si && si <= last;
          if (ok) {
            u64 t;
            if (si == last) {
              t = c64(rg.last_term)[g];
            } else if (si < c64(rg.first_index)[g] - 1) {
              t = 0;
            } else {
              t = walk_runs(rg.run_start, rg.run_term, G, g, si, meta_nruns(rg.meta[g]));
            }
            ok = t == stt;
          }
          if (ok) m64(rg.unstable_offset)[g] = si + 1;
          stab = ok;
          stale = !ok;
        }
        if (ss != 0 && c64(rg.usnap_index)[g] == ss) {  // stableSnapTo, log_unstable.go:109-113
          m64(rg.usnap_index)[g] = 0;
          m64(rg.usnap_term)[g] = 0;
          snap = true;
        }
      }
    }
    if (live)
      P.aflags[i] = u8((range ? QB_AFLAG_APPLIED_RANGE : 0u) | (autol ? QB_AFLAG_AUTO_LEAVE : 0u) |
                       (stale ? QB_AFLAG_STABLE_STALE : 0u) | (bad ? QB_AFLAG_BAD_GROUP : 0u));
    tally.add(QB_ASTAT_HARDSTATE, hard);
    tally.add(QB_ASTAT_APPLIED, appl);
    tally.add(QB_ASTAT_AUTO_LEAVE, autol);
    tally.add(QB_ASTAT_STABLE, stab);
    tally.add(QB_ASTAT_STABLE_STALE, stale);
    tally.add(QB_ASTAT_SNAP_STABLE, snap);
    tally.add(QB_ASTAT_APPLIED_RANGE, range);
    tally.add(QB_ASTAT_BAD_GROUP, bad);
  }
  __syncthreads();
  tally.stage(tl);
  __syncthreads();
  BlockTally<QB_ASTAT_COUNT>::publish(tl, P.stats);
}

// offset := min(offset, after) in each case of truncateAndAppend
// (log_unstable.go:121-145).
__global__ __launch_bounds__(kBlock) void k_unstable_truncate(u64 M, const u32* __restrict__ group,
                                                              const u64* __restrict__ app_from, u64 G,
                                                              u64* unstable_offset) {
  for (u64 i = u64(blockIdx.x) * kBlock + threadIdx.x; i < M; i += u64(gridDim.x) * kBlock) {
    const u64 from = app_from[i];
    const u64 g = group[i];
    if (from != 0 && g < G) atomicMin(unstable_offset + g, from);
  }
}

}  // namespace ready
}  // namespace qb

using namespace qb;

namespace {
// Workspace: the tile counts (+ the total) and their scan's block sums.
struct Carve {
  u64 nt;
  size_t cnt, bsum, total;
};
Carve carve(u64 G) {
  Carve c{};
  Carver k;
  c.nt = (G + kBlock - 1) / kBlock;
  c.cnt = k.take(sizeof(u32) * (c.nt + 1));
  c.bsum = k.take(sizeof(u32) * (scan::blocks(c.nt) + 1));
  c.total = k.o;
  return c;
}

bool groups_complete(const qb_ready_groups* rg) {
  return rg->term && rg->vote && rg->committed && rg->lead && rg->role && rg->first_index &&
         rg->last_index && rg->last_term && rg->meta && rg->run_start && rg->run_term &&
         rg->pending_conf_index && rg->applied && rg->unstable_offset && rg->usnap_index &&
         rg->usnap_term && rg->prev_term && rg->prev_vote && rg->prev_commit && rg->prev_lead &&
         rg->prev_role && rg->pending && rg->uncommitted_size;
}
}  // namespace

extern "C" size_t qb_ready_scratch_bytes(uint64_t G) {
  return G > QB_READY_MAX_GROUPS ? 0 : carve(G).total;
}

extern "C" int qb_dev_ready(const qb_ready_groups* rg, int accept, uint64_t ready_cap,
                            const qb_ready_out* out, uint64_t* stats, void* workspace,
                            size_t workspace_bytes, void* stream) {
  QB_REQUIRE(rg, "qb_dev_ready: rg is NULL");
  QB_REQUIRE(out, "qb_dev_ready: out is NULL");
  QB_REQUIRE(rg->G <= QB_READY_MAX_GROUPS, "qb_dev_ready: G %llu > %llu (ready_gid is a uint32)",
             (unsigned long long)rg->G, (unsigned long long)QB_READY_MAX_GROUPS);
  QB_REQUIRE(out->ready_count, "qb_dev_ready: ready_count is NULL");
  hipStream_t st = as_stream(stream);
  if (rg->G == 0) {
    const hipError_t e = hipMemsetAsync(out->ready_count, 0, sizeof(u64), st);
    return e == hipSuccess ? QB_OK : hip_fail(e, "hipMemsetAsync(ready_count)");
  }
  QB_REQUIRE(groups_complete(rg), "qb_dev_ready: required group pointer is NULL");
  QB_REQUIRE(out->rflags && out->ready_gid && out->rd_flags && out->hs_term && out->hs_vote &&
                 out->hs_commit && out->ent_lo && out->ent_hi && out->ent_last_term &&
                 out->apply_lo && out->apply_hi && out->snap_index && out->lead && out->role && stats,
             "qb_dev_ready: required output pointer is NULL");
  const Carve cv = carve(rg->G);
  QB_REQUIRE(workspace && workspace_bytes >= cv.total,
             "qb_dev_ready: workspace too small (qb_ready_scratch_bytes)");
  char* ws = static_cast<char*>(workspace);
  u32* cnt = reinterpret_cast<u32*>(ws + cv.cnt);
  u32* bsum = reinterpret_cast<u32*>(ws + cv.bsum);
  hipLaunchKernelGGL(ready::k_ready_flags, dim3(stream_grid<ready::k_ready_flags>(rg->G)),
                     dim3(kBlock), 0, st, *rg, out->rflags, cnt, reinterpret_cast<u64*>(stats));
  QB_CHECK_LAUNCH("k_ready_flags");
  scan::launch(cnt, cv.nt, bsum, st);
  QB_CHECK_LAUNCH("scan(ready)");
  ready::WriteArgs A{*rg, *out, ready_cap, reinterpret_cast<u64*>(stats), cnt, u32(cv.nt), accept};
  hipLaunchKernelGGL(ready::k_ready_write, dim3(stream_grid<ready::k_ready_write>(rg->G)),
                     dim3(kBlock), 0, st, A);
  QB_CHECK_LAUNCH("k_ready_write");
  return QB_OK;
}

extern "C" int qb_dev_advance(const qb_ready_groups* rg, uint64_t A, const qb_advance_in* in,
                              uint8_t* aflags, uint64_t* stats, void* stream) {
  QB_REQUIRE(rg, "qb_dev_advance: rg is NULL");
  QB_REQUIRE(rg->G <= QB_READY_MAX_GROUPS, "qb_dev_advance: G %llu > %llu",
             (unsigned long long)rg->G, (unsigned long long)QB_READY_MAX_GROUPS);
  if (A == 0) return QB_OK;
  QB_REQUIRE(in, "qb_dev_advance: in is NULL");
  QB_REQUIRE(rg->G == 0 || groups_complete(rg), "qb_dev_advance: required group pointer is NULL");
  QB_REQUIRE(in->adv_gid && in->hs_term && in->hs_vote && in->hs_commit && in->applied_to &&
                 in->applied_payload && in->stable_index && in->stable_term && in->stable_snap,
             "qb_dev_advance: required input pointer is NULL");
  QB_REQUIRE(aflags && stats, "qb_dev_advance: aflags / stats is NULL");
  ready::AdvArgs P{*rg, *in, A, aflags, reinterpret_cast<u64*>(stats)};
  hipLaunchKernelGGL(ready::k_advance, dim3(stream_grid<ready::k_advance>(A)), dim3(kBlock), 0,
                     as_stream(stream), P);
  QB_CHECK_LAUNCH("k_advance");
  return QB_OK;
}

extern "C" int qb_dev_unstable_truncate(uint64_t M, const uint32_t* group, const uint64_t* app_from,
                                        uint64_t G, uint64_t* unstable_offset, void* stream) {
  if (M == 0) return QB_OK;
  QB_REQUIRE(group && app_from, "qb_dev_unstable_truncate: group / app_from is NULL");
  QB_REQUIRE(G == 0 || unstable_offset, "qb_dev_unstable_truncate: unstable_offset is NULL");
  const unsigned tiles = grid_for(M);
  hipLaunchKernelGGL(ready::k_unstable_truncate, dim3(tiles < kStreamBlocks ? tiles : kStreamBlocks),
                     dim3(kBlock), 0, as_stream(stream), M, group, reinterpret_cast<const u64*>(app_from),
                     G, reinterpret_cast<u64*>(unstable_offset));
  QB_CHECK_LAUNCH("k_unstable_truncate");
  return QB_OK;
}
