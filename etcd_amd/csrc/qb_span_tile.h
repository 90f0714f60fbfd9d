// qb_span_tile.h — the shape the streaming step kernels share (k_tick,
// k_campaign, k_propose, k_requests, k_switch): one pass with no cross-group
// dependence.
//
// A workgroup takes tiles of 256 consecutive groups, which own one contiguous
// slot span [off[g0], off[gend]).  A group phase runs a thread per group and
// decides which groups act on their slots.  If any does, each acting group
// names itself owner of its slots in LDS (SpanOwners: one byte per slot of the
// span) and leaves its recipe beside the map in the kernel's own arrays; the
// workgroup then strides the span, kSpanUnroll slots per thread and trip with
// their loads in flight together, so slot arrays move as coalesced runs and
// slots of groups that do not act touch nothing.  A tile in which nothing acts
// skips the slot phase and its barriers.  256 well-formed groups own at most
// kSpanCap slots; a wider span — only a table with gaps, or groups above
// QB_MAX_SLOTS slots, which are read as QB_MAX_SLOTS — is not staged: each
// thread loops over its own group's slots in the global arrays.
//
// Each kernel keeps its phases, barriers and stride loop written out; this
// header owns the geometry, the owner map and its two rules (claim, find), the
// grid cap, and maybeSendAppend over Progress held in global memory.  k_tick
// alone spells the owner map out itself (it measured slower on SpanOwners;
// qb_tick.hip says by how much).
// qb_leader.hip's maybe_send_append<S> works on Progress staged in LDS by its
// own step and is a separate copy.
#pragma once

#include "qb_common.h"

namespace qb {

constexpr u32 kSpanCap = kBlock * QB_MAX_SLOTS;  // 4096: every well-formed tile
constexpr u32 kSpanUnroll = 4;  // slots per thread whose loads are in flight together
static_assert(kBlock <= 256 && QB_MAX_SLOTS <= 255, "SpanOwners keeps threads and slot counts in bytes");

// The grid's cap where the runtime will not say how many workgroups the device
// holds.  tests/test_gpu_stride.py sizes its batches by it (more tiles than
// this, so that workgroups take a second tile).
constexpr unsigned kStreamBlocks = 2048;

__device__ __forceinline__ u32 clamp_slots(u32 s0, u32 s1) {
  return s1 > s0 ? (s1 - s0 < QB_MAX_SLOTS ? s1 - s0 : u32(QB_MAX_SLOTS)) : 0u;
}

// What a workgroup knows of its tile.
struct SpanTile {
  u64 g0, gend;  // its groups
  u32 sb, span;  // its slots: [sb, sb + span)
  bool staged;   // the span fits the owner map (workgroup-uniform)
  __device__ __forceinline__ SpanTile(u64 tile, u64 G)
      : g0(tile * kBlock), gend(g0 + kBlock < G ? g0 + kBlock : G) {}
  // sb = off[g0], se = off[gend]
  __device__ __forceinline__ void bound(u32 sb_, u32 se) {
    sb = sb_;
    span = se - sb_;
    staged = se >= sb_ && span <= kSpanCap;
  }
};

// Slot of a staged span -> the thread (group) of the tile that acts on it.
struct SpanOwners {
  u8 owner[kSpanCap];
  u32 j0[kBlock];  // the group's first slot within the span
  u8 ns[kBlock];   // its slot count (<= QB_MAX_SLOTS)

  struct Slot {
    u32 t, k;  // the named owner and the slot's index within it
    bool in;   // k lies in t's range
  };

  // An acting group of a staged tile names itself owner of its ns slots from
  // s0 and gets back the count it may act on.  For any monotone off those
  // slots lie inside the span; a group whose slots do not (a malformed table)
  // claims and acts on none.  That test is all that stands between a bad off
  // table and a write outside owner[].
  __device__ __forceinline__ u32 claim(const SpanTile& S, u32 s0, u32 n) {
    const u32 j = s0 - S.sb;
    if (!(s0 >= S.sb && j <= S.span && n <= S.span - j)) n = 0;
    j0[threadIdx.x] = j;
    ns[threadIdx.x] = u8(n);
    for (u32 k = 0; k < n; ++k) owner[j + k] = u8(threadIdx.x);
    return n;
  }

  // Slot j < span of the tile.  Only acting groups claim, so a slot no acting
  // group owns holds a stale owner byte (an earlier tile's, or none at all):
  // the named owner's own range decides, and so does its action — the caller
  // acts on the slot only if its own flag byte of group t is set (a group that
  // does not act leaves j0 / ns stale too) and `in` holds.
  __device__ __forceinline__ Slot find(u32 j) const {
    const u32 t = owner[j];
    const u32 k = j - j0[t];
    return {t, k, k < ns[t]};
  }
};

// The workgroups the device holds at once (occupancy x CUs), at most
// kStreamBlocks, and kStreamBlocks if the runtime will not say: with that grid
// every workgroup strides the same number of tiles, none waits for a slot, and
// the statistics flush stays a few thousand atomics however large G is.  Asked
// once per process and kernel.
template <auto Kernel>
inline unsigned resident_blocks() {
  static const unsigned n = [] {
    int dev = 0, per_cu = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, Kernel, kBlock, 0) != hipSuccess ||
        per_cu <= 0 || cus <= 0) {
      (void)hipGetLastError();
      return kStreamBlocks;
    }
    const unsigned r = unsigned(per_cu) * unsigned(cus);
    return r < kStreamBlocks ? r : kStreamBlocks;
  }();
  return n;
}

// The grid of a streaming step kernel over G groups.
template <auto Kernel>
inline unsigned stream_grid(u64 G) {
  const unsigned tiles = grid_for(G), cap = resident_blocks<Kernel>();
  return tiles < cap ? tiles : cap;
}

// The term of index i from group g's run table (run q at run_start[q * G + g]),
// walking its first `upto` runs; 0 if none starts at or below i.
__device__ __forceinline__ u64 walk_runs(const void* run_start, const void* run_term, u64 G, u64 g,
                                         u64 i, u32 upto) {
  const u64* rs = static_cast<const u64*>(run_start) + g;
  const u64* rt = static_cast<const u64*>(run_term) + g;
  u64 t = 0;
  for (u32 q = 0; q < upto; ++q)
    if (rs[q * G] <= i) t = rt[q * G];
  return t;
}

// maybeSendAppend(to, true) (raft.go:432-492) on slot i of group g, whose next
// / pstate / infl_pos words (nx, st, ipos) the caller has read.  pg is the
// call's groups struct (Progress, Inflights, the snapshot words); first / last
// / ments are the log's bounds and the entries per message; term_prev() gives
// term(nx - 1) and is called only for a slot that is not paused.  The message
// goes to *mi (index), *ml (log term), *mn (entries).  Returns its type (0:
// none).  SendIfEmpty = false is maybeSendAppend(to, false): an empty entry
// list, a compacted next included, returns before the snapshot fallback
// (raft.go:442-444).
template <bool SendIfEmpty = true, class Groups, class TermPrev>
__device__ __forceinline__ u32 maybe_send_append(const Groups& pg, u64 g, u64 i, u64 nx, u8 st,
                                                 u32 ipos, u64 first, u64 last, u64 ments,
                                                 TermPrev term_prev, u64* mi, u64* ml, u64* mn) {
  const u32 K = pg.inflight_cap;
  const u32 state = st & 3u;
  // IsPaused (progress.go:193-212)
  if (state == QB_PR_PROBE ? (st & QB_PR_PROBE_SENT) != 0
                           : (state == QB_PR_REPLICATE ? (ipos >> 16) == K : true))
    return 0;
  const u64 lt = term_prev();
  u64 n = 0;
  bool compacted = false;
  if (nx <= last) {
    if (nx < first) compacted = true;  // ErrCompacted
    else {
      const u64 avail = last - nx + 1;
      n = avail < ments ? avail : ments;
    }
  }
  if (!SendIfEmpty && n == 0) return 0;
  if (compacted) {
    if (!(st & QB_PR_RECENT_ACTIVE)) return 0;
    const u64 snapi = reinterpret_cast<const u64*>(pg.snap_index)[g];
    if (snapi == 0) return 0;  // ErrSnapshotTemporarilyUnavailable
    *mi = snapi;
    *ml = reinterpret_cast<const u64*>(pg.snap_term)[g];
    *mn = 0;
    // BecomeSnapshot (progress.go:139-144)
    pg.pstate[i] = u8((st & QB_PR_RECENT_ACTIVE) | QB_PR_SNAPSHOT);
    reinterpret_cast<u64*>(pg.pending_snapshot)[i] = snapi;
    pg.infl_pos[i] = 0;
    return QB_MSG_SNAP;
  }
  *mi = nx - 1;
  *ml = lt;
  *mn = n;
  if (n != 0) {
    if (state == QB_PR_REPLICATE) {
      // OptimisticUpdate (progress.go:159-161), Inflights.Add (inflights.go:55-70)
      const u64 sent = nx + n - 1;
      reinterpret_cast<u64*>(pg.next)[i] = sent + 1;
      const u32 start = ipos & 0xFFFFu, count = ipos >> 16;
      u32 nxt = start + count;
      if (nxt >= K) nxt -= K;
      if (nxt < K) reinterpret_cast<u64*>(pg.infl_buf)[i * K + nxt] = sent;  // (the ring's invariant)
      pg.infl_pos[i] = start | ((count + 1) << 16);
    } else {
      pg.pstate[i] = u8(st | QB_PR_PROBE_SENT);
    }
  }
  return QB_MSG_APP;
}

}  // namespace qb
