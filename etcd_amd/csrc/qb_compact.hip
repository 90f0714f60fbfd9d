// qb_compact.hip — MemoryStorage.CreateSnapshot / Compact and etcdserver's
// trigger for G groups (qb_dev_log_compact): storage.go:190-236,
// server/etcdserver/server.go:1096-1117 (triggerSnapshot, shouldSnapshot),
// 1993-2067 (snapshot(): CreateSnapshot, the inflightSnapshots pause,
// SnapshotCatchUpEntries, Compact).
//
// The shape is qb_ready.hip's count / scan / write over a bounded grid:
//   C1 k_compact_flags  thread per group streams the request columns; a
//                       requesting group loads its six cursor words and
//                       decides both halves; writes cmflags[g] and the tile's
//                       count of acting groups (ballots, the waves summed
//                       through LDS) to cnt[tile].  Changes nothing.
//   scan                exclusive scan of the tile counts (qb_scan.h)
//   C2 k_compact_write  thread per group reads cmflags[g] alone; an acting
//                       group's position is its tile's offset plus the acting
//                       groups before it in the tile; past list_cap it is
//                       flagged deferred, else it loads its request, meta and
//                       table rows, applies, and writes its record
// No flag depends on the term runs (the checks are on cursors), so C1 loads
// no table row: the rows are read once, in C2, by the groups that change.
// A group's state is written by its own thread of C2 alone, so what C1
// decided still holds there.  No workgroup waits on another.
#include "qb_scan.h"
#include "qb_span_tile.h"

namespace qb {
namespace compact {

constexpr u32 kWaves = kBlock / 64;
constexpr u32 kRuns = QB_LEADER_MAX_RUNS;
constexpr u32 kFlagStats = 9;  // QB_CMSTAT_SNAPPED .. QB_CMSTAT_BAD_LOG follow the flag bits
constexpr u32 kActed = QB_CMF_SNAPPED | QB_CMF_COMPACTED;
constexpr u32 kStop = QB_CMF_OUT_OF_BOUND | QB_CMF_PAST_APPLIED;

static_assert(QB_CMF_SNAPPED == 1u << QB_CMSTAT_SNAPPED && QB_CMF_BAD_LOG == 1u << QB_CMSTAT_BAD_LOG &&
                  QB_CMF_DEFERRED == 1u << QB_CMSTAT_DEFERRED,
              "the flag counters follow the flag bits");
static_assert(kRuns == 8, "shift_rows moves by 4, 2, 1");

__device__ __forceinline__ const u64* c64(const void* p) { return static_cast<const u64*>(p); }
__device__ __forceinline__ u64* m64(void* p) { return static_cast<u64*>(p); }

// What group g is asked to do.  Explicit mode: the two columns, 0 = none.
// Trigger mode: shouldSnapshot (server.go:1115-1117), then snapshot()'s two
// indexes (server.go:1111, 2047-2051).
struct Request {
  bool snap, comp;
  u64 s, c;
};

__device__ __forceinline__ Request request_of(const qb_compact_groups& cg, const qb_compact_in& in,
                                              u64 g) {
  Request r{false, false, 0ull, 0ull};
  if (in.mode == QB_CM_EXPLICIT) {
    r.s = in.snap_at ? c64(in.snap_at)[g] : 0ull;
    r.c = in.compact_at ? c64(in.compact_at)[g] : 0ull;
    r.snap = r.s != 0;
    r.comp = r.c != 0;
    return r;
  }
  const u64 appl = c64(cg.applied)[g], snapi = c64(cg.snap_index)[g];
  const bool force = in.force && in.force[g] != 0;
  if ((force && appl != snapi) || appl - snapi > in.snapshot_count) {
    r.snap = r.comp = true;
    r.s = appl;
    r.c = appl > in.catch_up_entries ? appl - in.catch_up_entries : 1ull;
  }
  return r;
}

// The flags of a requesting group (everything but QB_CMF_DEFERRED): rules 2-6
// of the header.  The six cursor words are requested together.
__device__ __forceinline__ u32 decide(const qb_compact_groups& cg, const qb_compact_in& in, u64 g,
                                      const Request& r) {
  const u64 first = c64(cg.first_index)[g], snapi = c64(cg.snap_index)[g];
  const u64 last = c64(cg.last_index)[g], applied = c64(cg.applied)[g];
  const u64 uoff = c64(cg.unstable_offset)[g], usnap = c64(cg.usnap_index)[g];
  const u64 off = first - 1, sl = uoff - 1;
  if (first == 0 || sl < off || sl > last) return QB_CMF_BAD_LOG;
  if (usnap != 0) return QB_CMF_PENDING_SNAPSHOT;
  u32 f = 0;
  bool comp = r.comp;
  if (r.snap) {  // storage.go:194-213
    if (r.s <= snapi) f |= QB_CMF_SNAP_OUT_OF_DATE;
    else if (r.s > sl || r.s < off) f |= QB_CMF_OUT_OF_BOUND;
    else if (r.s > applied) f |= QB_CMF_PAST_APPLIED;
    else f |= QB_CMF_SNAPPED;
    if (in.mode == QB_CM_TRIGGER) {
      if (!(f & QB_CMF_SNAPPED)) {
        comp = false;  // server.go:2016-2023
      } else if (in.hold && in.hold[g] != 0) {
        f |= QB_CMF_HELD;  // server.go:2042-2045
        comp = false;
      }
    }
  }
  if (comp) {  // storage.go:218-236
    if (r.c <= off) f |= QB_CMF_ALREADY_COMPACTED;
    else if (r.c > sl) f |= QB_CMF_OUT_OF_BOUND;
    else if (r.c > applied) f |= QB_CMF_PAST_APPLIED;
    else f |= QB_CMF_COMPACTED;
  }
  if (f & kStop) f &= ~kActed;  // Go would not have returned: nothing applied
  return f;
}

struct FlagArgs {
  qb_compact_groups cg;
  qb_compact_in in;
  u16* cmflags;
  u32* cnt;
  u64* stats;
};

__global__ __launch_bounds__(kBlock) void k_compact_flags(FlagArgs A) {
  __shared__ u32 ws[2][kWaves];
  __shared__ u32 tl[kFlagStats];
  const u64 G = A.cg.G;
  const u64 ntiles = (G + kBlock - 1) / kBlock;
  const u32 tid = threadIdx.x;
  BlockTally<kFlagStats> tally;
  if (tid < kFlagStats) tl[tid] = 0;
  u32 par = 0;
  for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x, par ^= 1u) {
    const u64 g = tile * kBlock + tid;
    u32 f = 0;
    if (g < G) {
      const Request r = request_of(A.cg, A.in, g);
      if (r.snap || r.comp) f = decide(A.cg, A.in, g, r);
      A.cmflags[g] = u16(f);
    }
    const u32 c = wave_popc((f & kActed) != 0);
    if ((tid & 63u) == 0) ws[par][tid >> 6] = c;
#pragma unroll
    for (u32 k = 0; k < kFlagStats; ++k) tally.add(int(k), (f >> k) & 1u);
    __syncthreads();  // one barrier a tile: ws alternates between two rows
    if (tid == 0) {
      u32 t = 0;
#pragma unroll
      for (u32 w = 0; w < kWaves; ++w) t += ws[par][w];
      A.cnt[tile] = t;
    }
  }
  __syncthreads();  // tl zeroed (a block with no tile passed no barrier)
  tally.stage(tl);
  __syncthreads();
  BlockTally<kFlagStats>::publish(tl, A.stats);
}

// v[j] := v[j + k] for j + k < 8, in registers: three conditional moves by 4,
// 2 and 1, every index a constant.
__device__ __forceinline__ void shift_rows(u64 (&v)[kRuns], u32 k) {
#pragma unroll
  for (u32 s = 4; s >= 1; s >>= 1) {
    const bool on = (k & s) != 0;
#pragma unroll
    for (u32 j = 0; j + s < kRuns; ++j) v[j] = on ? v[j + s] : v[j];
  }
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

struct WriteArgs {
  qb_compact_groups cg;
  qb_compact_in in;
  qb_compact_out out;
  u64 cap;
  u64* stats;
  const u32* cnt;
  u32 ntiles;
};

__global__ __launch_bounds__(kBlock) void k_compact_write(WriteArgs A) {
  __shared__ u32 ws[2][kWaves];
  __shared__ u32 tl[3];  // deferred, listed, runs dropped
  __shared__ u64 te;     // entries dropped
  const qb_compact_groups& cg = A.cg;
  const qb_compact_out& o = A.out;
  const u64 G = cg.G;
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  BlockTally<2> tally;  // 0: deferred, 1: listed
  u32 kacc = 0;
  u64 eacc = 0;
  if (tid < 3) tl[tid] = 0;
  if (tid == 0) te = 0;
  if (blockIdx.x == 0 && tid == 0) *o.list_count = A.cnt[A.ntiles];
  u32 par = 0;
  for (u64 tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x, par ^= 1u) {
    const u64 g = tile * kBlock + tid;
    const bool live = g < G;
    const u32 f = live ? u32(o.cmflags[g]) : 0u;
    const bool act = (f & kActed) != 0;
    const u64 b = __ballot(act);
    if (lane == 0) ws[par][wave] = u32(__popcll(b));
    __syncthreads();
    u32 before = 0;
    for (u32 q = 0; q < wave; ++q) before += ws[par][q];
    const u64 pos = u64(A.cnt[tile]) + before + u32(__popcll(b & ((1ull << lane) - 1ull)));
    const bool listed = act && pos < A.cap, deferred = act && !listed;
    tally.add(0, deferred);
    tally.add(1, listed);
    if (deferred) o.cmflags[g] = u16(f | QB_CMF_DEFERRED);
    if (!listed) continue;
    const bool snapped = (f & QB_CMF_SNAPPED) != 0, compacted = (f & QB_CMF_COMPACTED) != 0;
    // the request again, and the words the table walk waits for
    const Request r = request_of(cg, A.in, g);
    const u64 first = c64(cg.first_index)[g];
    const u32 meta = cg.meta[g];
    u64 si = 0, st = 0;
    if (!snapped) {  // the record carries the snapshot as it stays
      si = c64(cg.snap_index)[g];
      st = c64(cg.snap_term)[g];
    }
    const u32 n = meta_nruns(meta);
    // every row of the group before any is written; run-major rows are
    // coalesced across the wave
    u64 rs[kRuns], rt[kRuns];
#pragma unroll
    for (u32 q = 0; q < kRuns; ++q) {
      rs[q] = q < n ? c64(cg.run_start)[q * G + g] : 0ull;
      rt[q] = q < n ? c64(cg.run_term)[q * G + g] : 0ull;
    }
    if (snapped) {  // term(s): storage.go:207
      si = r.s;
      st = rt[0];
#pragma unroll
      for (u32 q = 1; q < kRuns; ++q)
        if (q < n && rs[q] <= r.s) st = rt[q];
      m64(cg.snap_index)[g] = si;
      m64(cg.snap_term)[g] = st;
    }
    if (compacted) {  // storage.go:229-234 on the runs
      u32 k = 0;
#pragma unroll
      for (u32 q = 1; q < kRuns; ++q)
        if (q < n && rs[q] <= r.c) k = q;
      shift_rows(rs, k);
      shift_rows(rt, k);
      rs[0] = r.c;
      const u32 keep = n - k;
#pragma unroll
      for (u32 j = 0; j < kRuns; ++j) {
        if (j < keep && (j == 0 || k != 0)) m64(cg.run_start)[j * G + g] = rs[j];
        if (j < keep && k != 0) m64(cg.run_term)[j * G + g] = rt[j];
      }
      const u32 m1 = (meta & ~0xF0000u) | (keep << 16);
      if (m1 != meta) cg.meta[g] = m1;
      m64(cg.first_index)[g] = r.c + 1;
      kacc += k;
      eacc += r.c - (first - 1);
    }
    o.gid[pos] = u32(g);
    o.flags[pos] = u16(f);
    m64(o.snap_index)[pos] = si;
    m64(o.snap_term)[pos] = st;
    m64(o.compact_index)[pos] = compacted ? r.c : 0ull;
    m64(o.first_before)[pos] = first;
  }
  __syncthreads();
  tally.stage(tl);
  const u32 kw = wave_sum(kacc);
  const u64 ew = wave_sum64(eacc);
  if (lane == 0) {
    if (kw) atomicAdd(&tl[2], kw);
    if (ew) atomicAdd(&te, ew);
  }
  __syncthreads();
  if (tid < 2 && tl[tid]) atomicAdd(A.stats + QB_CMSTAT_DEFERRED + tid, u64(tl[tid]));
  if (tid == 2 && tl[2]) atomicAdd(A.stats + QB_CMSTAT_RUNS_DROPPED, u64(tl[2]));
  if (tid == 3 && te) atomicAdd(A.stats + QB_CMSTAT_ENTRIES_DROPPED, te);
}

static_assert(QB_CMSTAT_LISTED == QB_CMSTAT_DEFERRED + 1, "k_compact_write's first two counters");

}  // namespace compact
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
}  // namespace

extern "C" size_t qb_log_compact_scratch_bytes(uint64_t G) {
  return G > QB_READY_MAX_GROUPS ? 0 : carve(G).total;
}

extern "C" int qb_dev_log_compact(const qb_compact_groups* cg, const qb_compact_in* in,
                                  uint64_t list_cap, const qb_compact_out* out, uint64_t* stats,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  QB_REQUIRE(cg, "qb_dev_log_compact: cg is NULL");
  QB_REQUIRE(in, "qb_dev_log_compact: in is NULL");
  QB_REQUIRE(out, "qb_dev_log_compact: out is NULL");
  QB_REQUIRE(in->mode == QB_CM_EXPLICIT || in->mode == QB_CM_TRIGGER,
             "qb_dev_log_compact: mode %u is neither QB_CM_EXPLICIT nor QB_CM_TRIGGER", in->mode);
  QB_REQUIRE(cg->G <= QB_READY_MAX_GROUPS, "qb_dev_log_compact: G %llu > %llu (gid is a uint32)",
             (unsigned long long)cg->G, (unsigned long long)QB_READY_MAX_GROUPS);
  QB_REQUIRE(out->list_count, "qb_dev_log_compact: list_count is NULL");
  hipStream_t st = as_stream(stream);
  if (cg->G == 0) {
    const hipError_t e = hipMemsetAsync(out->list_count, 0, sizeof(u64), st);
    return e == hipSuccess ? QB_OK : hip_fail(e, "hipMemsetAsync(list_count)");
  }
  QB_REQUIRE(cg->first_index && cg->snap_index && cg->snap_term && cg->meta && cg->run_start &&
                 cg->run_term && cg->last_index && cg->applied && cg->unstable_offset &&
                 cg->usnap_index,
             "qb_dev_log_compact: required group pointer is NULL");
  QB_REQUIRE(out->cmflags && out->gid && out->flags && out->snap_index && out->snap_term &&
                 out->compact_index && out->first_before && stats,
             "qb_dev_log_compact: required output pointer is NULL");
  const Carve cv = carve(cg->G);
  QB_REQUIRE(workspace && workspace_bytes >= cv.total,
             "qb_dev_log_compact: workspace too small (qb_log_compact_scratch_bytes)");
  char* ws = static_cast<char*>(workspace);
  u32* cnt = reinterpret_cast<u32*>(ws + cv.cnt);
  u32* bsum = reinterpret_cast<u32*>(ws + cv.bsum);
  compact::FlagArgs F{*cg, *in, out->cmflags, cnt, reinterpret_cast<u64*>(stats)};
  hipLaunchKernelGGL(compact::k_compact_flags, dim3(stream_grid<compact::k_compact_flags>(cg->G)),
                     dim3(kBlock), 0, st, F);
  QB_CHECK_LAUNCH("k_compact_flags");
  scan::launch(cnt, cv.nt, bsum, st);
  QB_CHECK_LAUNCH("scan(compact)");
  compact::WriteArgs W{*cg, *in, *out, list_cap, reinterpret_cast<u64*>(stats), cnt, u32(cv.nt)};
  hipLaunchKernelGGL(compact::k_compact_write, dim3(stream_grid<compact::k_compact_write>(cg->G)),
                     dim3(kBlock), 0, st, W);
  QB_CHECK_LAUNCH("k_compact_write");
  return QB_OK;
}
