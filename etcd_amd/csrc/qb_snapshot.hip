// qb_snapshot.hip — MsgSnap at a non-leader for R records of distinct groups
// (qb_dev_follower_snapshot): Step's term filter raft.go:849-920, stepCandidate
// raft.go:1396-1398, stepFollower raft.go:1441-1444, handleSnapshot / restore
// raft.go:1518-1614, promotable raft.go:1618-1621, raftLog.restore
// log.go:336-340, unstable.restore log_unstable.go:115-119, raftLog.term /
// matchTerm log.go:268-288, 320-326, commitTo log.go:236-244.
//
// The shape is k_advance's (qb_ready.hip): one launch, a thread per record, a
// workgroup strides tiles of 256 records over a grid bounded by stream_grid.
// A record gathers its group's words and scatters what its outcome changes;
// the groups of a call are distinct, so no thread meets another's group.  A
// record's outcome is decided in registers and written at the end: the stop
// (commitTo's panic) is found before anything of the record is applied.
#include "qb_span_tile.h"

namespace qb {
namespace snapshot {

constexpr u32 kFlagStats = QB_SSTAT_COUNT;  // the counters follow the first flag bits

static_assert(QB_SNF_RESTORED == 1u << QB_SSTAT_RESTORED &&
                  QB_SNF_FAST_FORWARD == 1u << QB_SSTAT_FAST_FORWARD &&
                  QB_SNF_OLD == 1u << QB_SSTAT_OLD && QB_SNF_NOT_MEMBER == 1u << QB_SSTAT_NOT_MEMBER &&
                  QB_SNF_STALE == 1u << QB_SSTAT_STALE &&
                  QB_SNF_ROLE_IGNORED == 1u << QB_SSTAT_ROLE_IGNORED &&
                  QB_SNF_RESET == 1u << QB_SSTAT_BECAME_FOLLOWER &&
                  QB_SNF_COMMIT_RANGE == 1u << QB_SSTAT_COMMIT_RANGE &&
                  QB_SNF_BAD_GROUP == 1u << QB_SSTAT_BAD_GROUP,
              "the flag counters follow the flag bits");

__device__ __forceinline__ const u64* c64(const void* p) { return static_cast<const u64*>(p); }
__device__ __forceinline__ u64* m64(void* p) { return static_cast<u64*>(p); }

struct Args {
  qb_snapshot_groups sg;
  qb_snapshot_inbox in;
  qb_snapshot_out out;
  u64* stats;
};

struct Resp {
  u32 type;
  u64 term, index;
};

// The node's own ID in Voters / Learners / VotersOutgoing of the record's
// ConfState (raft.go:1554-1573): a loop over the record's span.  Consecutive
// records own consecutive spans, so a wave reads one contiguous run.
__device__ __forceinline__ bool is_member(const qb_snapshot_inbox& in, u64 i, u64 self) {
  const u64 C = in.C;
  u64 s0 = in.cs_off[i], s1 = in.cs_off[i + 1];
  s0 = s0 < C ? s0 : C;
  s1 = s1 < C ? s1 : C;
  bool found = false;
  for (u64 k = s0; k < s1; ++k)
    found |= c64(in.cs_id)[k] == self && in.cs_set[k] <= QB_CS_VOTERS_OUTGOING;
  return found;
}

// raft.Step(MsgSnap) of record i on group g < G.  Returns the record's sflags.
__device__ __forceinline__ u32 step(const Args& P, u64 i, u64 g, Resp* resp) {
  const qb_snapshot_groups& sg = P.sg;
  const qb_snapshot_inbox& in = P.in;
  const u64 G = sg.G;
  // the record and the group words every outcome meets, requested together
  const u64 from = c64(in.from)[i], mt = c64(in.term)[i];
  const u64 si = c64(in.snap_index)[i], st = c64(in.snap_term)[i];
  const u64 term0 = m64(sg.term)[g], com0 = m64(sg.committed)[g];
  const u64 self = c64(sg.self_id)[g], last = m64(sg.last_index)[g];
  const u32 role0 = sg.role[g];

  if (mt != 0 && mt < term0) return QB_SNF_STALE;  // raft.go:883-919: no branch names MsgSnap
  const bool higher = mt != 0 && mt > term0;       // raft.go:876-877
  const u32 state = higher ? u32(QB_ROLE_FOLLOWER) : (role0 & 3u);
  if (state == QB_ROLE_LEADER) return QB_SNF_ROLE_IGNORED;  // stepLeader: no case
  // becomeFollower(m.Term, m.From): the filter's, or a (pre-)candidate's (raft.go:1396-1398)
  const bool reset = higher || state != QB_ROLE_FOLLOWER;
  const u64 term1 = reset ? mt : term0;

  u32 f = reset ? u32(QB_SNF_RESET) : 0u;
  u64 com1 = com0;
  bool restored = false;
  u32 meta = 0;
  bool have_meta = false;
  if (si <= com0) {  // raft.go:1535-1537
    f |= QB_SNF_OLD;
  } else if (!is_member(in, i, self)) {  // raft.go:1554-1580
    f |= QB_SNF_NOT_MEMBER;
  } else {
    // term(snap_index), log.go:268-288: last_term at the end, the run table
    // inside the log, 0 outside [first_index - 1, last_index]
    u64 t;
    if (si == last) {
      t = m64(sg.last_term)[g];
    } else if (si > last || si < m64(sg.first_index)[g] - 1) {
      t = 0;
    } else {
      meta = sg.meta[g];
      have_meta = true;
      t = walk_runs(sg.run_start, sg.run_term, G, g, si, meta_nruns(meta));
    }
    if (t == st) {  // matchTerm: raft.go:1584-1589
      if (last < si) return QB_SNF_COMMIT_RANGE;  // commitTo panics (log.go:239-241): nothing applied
      f |= QB_SNF_FAST_FORWARD;
    } else {
      f |= QB_SNF_RESTORED;
      restored = true;
      if (!have_meta) meta = sg.meta[g];
    }
    com1 = si;
  }

  // ---- the record's writes ----
  if (term1 != term0) {  // reset, raft.go:591-594
    m64(sg.term)[g] = term1;
    m64(sg.vote)[g] = 0;
  }
  m64(sg.lead)[g] = from;  // raft.go:690 / 1443
  sg.election_elapsed[g] = 0;
  if (reset) sg.heartbeat_elapsed[g] = 0;
  u32 role1 = reset ? ((role0 & ~3u) | QB_ROLE_FOLLOWER) : role0;
  if (restored) role1 &= ~u32(QB_ROLE_PROMOTABLE);  // hasPendingSnapshot, raft.go:1618-1621
  if (role1 != role0) sg.role[g] = u8(role1);
  if (com1 != com0) m64(sg.committed)[g] = com1;
  if (restored) {  // raftLog.restore + unstable.restore
    m64(sg.unstable_offset)[g] = si + 1;
    m64(sg.usnap_index)[g] = si;
    m64(sg.usnap_term)[g] = st;
    m64(sg.last_index)[g] = si;
    m64(sg.last_term)[g] = st;
    m64(sg.first_index)[g] = si + 1;
    m64(sg.run_start)[g] = si;  // run 0; the rows behind it keep what they hold
    m64(sg.run_term)[g] = st;
    const u32 m1 = (meta & ~0xF0000u) | 0x10000u;
    if (m1 != meta) sg.meta[g] = m1;
  }
  if (sg.pending) {  // the response is a message: len(r.msgs) > 0
    const u8 p = sg.pending[g];
    if (!(p & QB_RDP_MSGS)) sg.pending[g] = u8(p | QB_RDP_MSGS);
  }
  if (term1 != term0 || com1 != com0) f |= QB_SNF_HARDSTATE;
  resp->type = QB_FRESP_APP_RESP;
  resp->term = term1;                  // send stamps r.Term
  resp->index = restored ? si : com1;  // lastIndex() / committed, raft.go:1523, 1527
  return f;
}

__global__ __launch_bounds__(kBlock) void k_snapshot(Args P) {
  __shared__ u32 tl[kFlagStats];
  const u64 G = P.sg.G, R = P.in.R;
  const u32 tid = threadIdx.x;
  BlockTally<kFlagStats> tally;
  if (tid < kFlagStats) tl[tid] = 0;
  const u64 ntiles = (R + kBlock - 1) / kBlock;
  for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const u64 i = tile * kBlock + tid;
    u32 f = 0;
    if (i < R) {
      const u64 g = P.in.group[i];
      Resp resp{0u, 0ull, 0ull};
      f = g < G ? step(P, i, g, &resp) : u32(QB_SNF_BAD_GROUP);
      P.out.sflags[i] = u16(f);
      P.out.resp_type[i] = u8(resp.type);
      m64(P.out.resp_term)[i] = resp.term;
      m64(P.out.resp_index)[i] = resp.index;
    }
#pragma unroll
    for (u32 k = 0; k < kFlagStats; ++k) tally.add(int(k), (f >> k) & 1u);
  }
  __syncthreads();
  tally.stage(tl);
  __syncthreads();
  BlockTally<kFlagStats>::publish(tl, P.stats);
}

}  // namespace snapshot
}  // namespace qb

using namespace qb;

extern "C" int qb_dev_follower_snapshot(const qb_snapshot_groups* sg, const qb_snapshot_inbox* in,
                                        const qb_snapshot_out* out, uint64_t* stats, void* stream) {
  QB_REQUIRE(sg, "qb_dev_follower_snapshot: sg is NULL");
  QB_REQUIRE(in, "qb_dev_follower_snapshot: in is NULL");
  QB_REQUIRE(out, "qb_dev_follower_snapshot: out is NULL");
  QB_REQUIRE(sg->G <= QB_READY_MAX_GROUPS, "qb_dev_follower_snapshot: G %llu > %llu",
             (unsigned long long)sg->G, (unsigned long long)QB_READY_MAX_GROUPS);
  QB_REQUIRE(in->R <= 0xFFFFFFFEull, "qb_dev_follower_snapshot: R %llu > 2^32 - 2",
             (unsigned long long)in->R);
  if (sg->G == 0 || in->R == 0) return QB_OK;
  QB_REQUIRE(sg->self_id && sg->term && sg->vote && sg->lead && sg->committed && sg->role &&
                 sg->election_elapsed && sg->heartbeat_elapsed && sg->first_index && sg->last_index &&
                 sg->last_term && sg->meta && sg->run_start && sg->run_term && sg->unstable_offset &&
                 sg->usnap_index && sg->usnap_term,
             "qb_dev_follower_snapshot: required group pointer is NULL");
  QB_REQUIRE(in->group && in->from && in->term && in->snap_index && in->snap_term && in->cs_off &&
                 (in->C == 0 || (in->cs_id && in->cs_set)),
             "qb_dev_follower_snapshot: required input pointer is NULL");
  QB_REQUIRE(out->sflags && out->resp_type && out->resp_term && out->resp_index && stats,
             "qb_dev_follower_snapshot: required output pointer is NULL");
  snapshot::Args P{*sg, *in, *out, reinterpret_cast<u64*>(stats)};
  hipLaunchKernelGGL(snapshot::k_snapshot, dim3(stream_grid<snapshot::k_snapshot>(in->R)),
                     dim3(kBlock), 0, as_stream(stream), P);
  QB_CHECK_LAUNCH("k_snapshot");
  return QB_OK;
}
