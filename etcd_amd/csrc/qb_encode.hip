// qb_encode.hip — gogoproto Message.Marshal of M outgoing messages
// (qb_dev_encode_messages, qb_dev_encode_msg_out, qb_dev_encode_slots): the
// mirror of qb_wire.hip.  raftpb/raft.pb.go: Message.Size 1235-1263,
// MarshalToSizedBuffer 903-972, the nested Snapshot 863-886, SnapshotMetadata
// 824-846, ConfState 1021-1063 and Entry 785-807; raft.send raft.go:386-419,
// sendHeartbeat 495-511, maybeSendAppend 432-492, responseToReadIndexReq
// 1737-1751.
//
// One encoder over a source functor that yields the fields and the status of
// message i (as qb_wire_src.h parameterises the decoder); three launches and
// the scan between them:
//   E1 k_enc_size   thread per message: its length (Message.Size) as a u32
//   scan            exclusive scan of the lengths (qb_scan.h): the offsets
//   E2 k_enc_write  a workgroup per tile of 256 consecutive messages, tiles
//                   strided over a bounded grid.  A tile's bytes are one
//                   contiguous span of at most 256 * QB_ENC_MAX_BYTES; each
//                   lane re-reads its fields, encodes its message into an
//                   LDS stage at its offset within the span, and the
//                   workgroup copies the stage out with 16-byte stores.  The
//                   stage starts at (address of the span's first byte) & 15,
//                   so aligned 16-byte LDS reads feed aligned 16-byte global
//                   stores; the bytes before the first and behind the last
//                   16-byte boundary of the span share their block with the
//                   neighbouring tiles and go out as byte stores of the
//                   tile's own bytes only (never a read-modify-write: two
//                   workgroups may hold the same block at once).
// E2 re-reads instead of E1 keeping the fields: the lengths are the only
// words between the passes (DESIGN.md §3.8d has the bytes of both).  No
// workgroup waits on another: the order comes from the scan.
#include "qb_scan.h"
#include "qb_span_tile.h"

namespace qb {
namespace enc {

constexpr u32 kStage = kBlock * QB_ENC_MAX_BYTES;  // 28,416: a full tile's span
constexpr u32 kSnapBytes = 12;                     // field 9 holding the empty Snapshot
constexpr u32 kReadEntryBytes = 18;                // field 7 holding Entry{Data: 8 bytes}
constexpr u32 kContextBytes = 10;                  // field 12 holding 8 bytes

__device__ __forceinline__ const u64* c64(const void* p) { return static_cast<const u64*>(p); }

// What a source yields for message i.
struct Msg {
  u64 to, from, term, log_term, index, commit, hint, ctx;
  u32 type, reject;
  u32 st;  // QB_ENC_OK / ENTRIES / HOST / NONE
};

__device__ __forceinline__ Msg no_msg(u32 st) {
  Msg m{};
  m.st = st;
  return m;
}

__device__ __forceinline__ bool is_read(u32 type) { return type == 15u || type == 16u; }

// sovRaft (raft.pb.go:1354-1356).
__device__ __forceinline__ u32 sov(u64 v) { return u32(64 - __clzll((long long)(v | 1ull)) + 6) / 7u; }

// Bytes up to and including the Index field: ent_at.
__device__ __forceinline__ u32 head_size(const Msg& m) {
  return 6u + sov(m.type) + sov(m.to) + sov(m.from) + sov(m.term) + sov(m.log_term) + sov(m.index);
}

// Message.Size (raft.pb.go:1235-1263) of what the device writes.
__device__ __forceinline__ u32 size_of(const Msg& m) {
  u32 n = head_size(m) + 1u + sov(m.commit) + kSnapBytes + 2u + 1u + sov(m.hint);
  if (m.ctx != 0) n += is_read(m.type) ? kReadEntryBytes : kContextBytes;
  return n;
}

__device__ __forceinline__ u8* put_field(u8* p, u32 key, u64 v) {
  *p++ = u8(key);
  while (v >= 0x80) {  // encodeVarintRaft (raft.pb.go:1180-1190)
    *p++ = u8(v) | 0x80u;
    v >>= 7;
  }
  *p++ = u8(v);
  return p;
}

__device__ __forceinline__ u8* put_be64(u8* p, u64 v) {
#pragma unroll
  for (int k = 7; k >= 0; --k) *p++ = u8(v >> (8 * k));
  return p;
}

// MarshalToSizedBuffer (raft.pb.go:903-972), front to back.
__device__ __forceinline__ void encode(u8* p, const Msg& m) {
  p = put_field(p, 0x08, m.type);
  p = put_field(p, 0x10, m.to);
  p = put_field(p, 0x18, m.from);
  p = put_field(p, 0x20, m.term);
  p = put_field(p, 0x28, m.log_term);
  p = put_field(p, 0x30, m.index);
  if (m.ctx != 0 && is_read(m.type)) {  // Entries: one Entry{Type 0, Term 0, Index 0, Data}
    const u8 e[10] = {0x3a, 0x10, 0x08, 0x00, 0x10, 0x00, 0x18, 0x00, 0x22, 0x08};
#pragma unroll
    for (int k = 0; k < 10; ++k) *p++ = e[k];
    p = put_be64(p, m.ctx);
  }
  p = put_field(p, 0x40, m.commit);
  // Snapshot{Metadata{ConfState{AutoLeave: false}, Index: 0, Term: 0}}
  const u8 s[kSnapBytes] = {0x4a, 0x0a, 0x12, 0x08, 0x0a, 0x02, 0x28, 0x00, 0x10, 0x00, 0x18, 0x00};
#pragma unroll
  for (u32 k = 0; k < kSnapBytes; ++k) *p++ = s[k];
  *p++ = 0x50;
  *p++ = m.reject ? 1 : 0;
  p = put_field(p, 0x58, m.hint);
  if (m.ctx != 0 && !is_read(m.type)) {
    *p++ = 0x62;
    *p++ = 0x08;
    p = put_be64(p, m.ctx);
  }
}

// ---------------------------------------------------------------- sources ---
// The general form: every field a column, NULL reads as 0.
struct ColSrc {
  qb_encode_cols c;
  __device__ __forceinline__ static u64 at(const void* p, u64 i) { return p ? c64(p)[i] : 0ull; }
  __device__ __forceinline__ Msg get(u64 i) const {
    const u32 type = c.type[i];
    if (type == 0) return no_msg(QB_ENC_NONE);
    if (type == QB_MSG_SNAP) return no_msg(QB_ENC_HOST);
    Msg m;
    m.type = type;
    m.to = at(c.to, i);
    m.from = at(c.from, i);
    m.term = at(c.term, i);
    m.log_term = at(c.log_term, i);
    m.index = at(c.index, i);
    m.commit = at(c.commit, i);
    m.hint = at(c.reject_hint, i);
    m.ctx = at(c.context, i);
    m.reject = c.reject ? c.reject[i] : 0u;
    m.st = !is_read(type) && at(c.n_entries, i) != 0 ? QB_ENC_ENTRIES : QB_ENC_OK;
    return m;
  }
};

// What the group front ends form of a type and its raw operands (n: entries,
// ctx: request id), with raft.send's From and Term (raft.go:386-419).
__device__ __forceinline__ Msg form(const qb_encode_groups& eg, u64 g, u32 type, u64 to, u64 index,
                                    u64 log_term, u64 commit, u64 n, u64 ctx) {
  Msg m{};
  m.type = type;
  m.to = to;
  m.from = c64(eg.self_id)[g];
  m.term = c64(eg.term)[g];
  m.st = QB_ENC_OK;
  switch (type) {
    case QB_MSG_APP:  // maybeSendAppend, raft.go:471-475
      m.index = index;
      m.log_term = log_term;
      m.commit = commit;
      if (n != 0) m.st = QB_ENC_ENTRIES;
      break;
    case QB_MSG_HEARTBEAT:  // sendHeartbeat, raft.go:503-508
      m.commit = commit;
      m.ctx = ctx;
      break;
    case QB_MSG_TIMEOUT_NOW:  // sendTimeoutNow, raft.go:1722-1724
      break;
    case QB_MSG_READ_INDEX_RESP:  // responseToReadIndexReq, raft.go:1745-1750
      m.index = index;
      m.ctx = ctx;
      break;
    default:
      return no_msg(QB_ENC_HOST);
  }
  return m;
}

__device__ __forceinline__ bool no_type(u32 type) { return type == 0 || type == QB_READ_STATE; }

// qb_dev_leader_step's list (or an outbox's record arrays, flat).
struct ListSrc {
  qb_encode_groups eg;
  const qb_msg_out* msgs;
  const u64* total;  // device, nullable
  __device__ __forceinline__ Msg get(u64 i) const {
    if (total && i >= *total) return no_msg(QB_ENC_NONE);
    const qb_msg_out r = msgs[i];
    if (no_type(r.type) || r.to == 0xFFu || r.group >= eg.G) return no_msg(QB_ENC_NONE);
    const u32 s0 = eg.off[r.group];
    if (r.to >= clamp_slots(s0, eg.off[r.group + 1])) return no_msg(QB_ENC_NONE);
    return form(eg, r.group, r.type, c64(eg.ids)[s0 + r.to], r.index, r.log_term, r.commit, r.aux,
                r.aux);
  }
};

// Slot-aligned columns: message s belongs to slot s; sgrp[s] names its group
// (k_slot_groups).  A word of sgrp no group wrote is whatever the workspace
// held: the group it names owns s only if its own off range says so.
struct SlotSrc {
  qb_encode_groups eg;
  qb_encode_slot_cols c;
  const u32* sgrp;
  __device__ __forceinline__ Msg get(u64 s) const {
    const u64 g = sgrp[s];
    if (g >= eg.G) return no_msg(QB_ENC_NONE);
    const u32 s0 = eg.off[g];
    if (!(s >= s0 && s - s0 < clamp_slots(s0, eg.off[g + 1]))) return no_msg(QB_ENC_NONE);
    if (c.gflags && !(c.gflags[g] & c.gmask)) return no_msg(QB_ENC_NONE);
    const u32 type = c.type ? u32(c.type[s]) : (c.type_all & 0xFFu);
    if (no_type(type)) return no_msg(QB_ENC_NONE);
    const u64 to = c64(eg.ids)[s];
    if (to == c64(eg.self_id)[g]) return no_msg(QB_ENC_NONE);
    const u64 commit = c.commit ? c64(c.commit)[s] : (c.commit_g ? c64(c.commit_g)[g] : 0ull);
    return form(eg, g, type, to, ColSrc::at(c.index, s), ColSrc::at(c.log_term, s), commit,
                ColSrc::at(c.n_entries, s), c.ctx_g ? c64(c.ctx_g)[g] : 0ull);
  }
};

// sgrp[s] = g for the slots of group g (its first QB_MAX_SLOTS, below S).
__global__ __launch_bounds__(kBlock) void k_slot_groups(u64 G, const u32* __restrict__ off, u64 S,
                                                        u32* __restrict__ sgrp) {
  for (u64 g = u64(blockIdx.x) * kBlock + threadIdx.x; g < G; g += u64(gridDim.x) * kBlock) {
    const u32 s0 = off[g], n = clamp_slots(s0, off[g + 1]);
    for (u32 k = 0; k < n; ++k)
      if (u64(s0) + k < S) sgrp[s0 + k] = u32(g);
  }
}

// ------------------------------------------------------------------ passes ---
template <class Src>
__global__ __launch_bounds__(kBlock) void k_enc_size(Src src, u64 M, u32* __restrict__ len) {
  for (u64 i = u64(blockIdx.x) * kBlock + threadIdx.x; i < M; i += u64(gridDim.x) * kBlock) {
    const Msg m = src.get(i);
    len[i] = m.st <= QB_ENC_ENTRIES ? size_of(m) : 0u;
  }
}

template <class Src>
__global__ __launch_bounds__(kBlock) void k_enc_write(Src src, u64 M, const u32* __restrict__ pre,
                                                      qb_encode_out o) {
  __shared__ __attribute__((aligned(16))) u8 stage[kStage + 16];
  __shared__ u32 s_wend[2];  // the end of the tile's written bytes, by trip parity
  __shared__ u32 tl[QB_ENC_STATUS_COUNT];
  const u32 tid = threadIdx.x;
  const u64 ntiles = (M + kBlock - 1) / kBlock;
  BlockTally<QB_ENC_STATUS_COUNT> tally;
  if (tid < QB_ENC_STATUS_COUNT) tl[tid] = 0;
  if (blockIdx.x == 0 && tid == 0) {
    *o.nbytes = pre[M];
    o.msg_off[M] = pre[M];
  }
  u32 par = 0;
  for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x, par ^= 1u) {
    const u64 i0 = tile * kBlock, i1 = i0 + kBlock < M ? i0 + kBlock : M;
    const u32 begin = pre[i0], end = pre[i1];
    const u32 shift = u32(reinterpret_cast<uintptr_t>(o.bytes) + begin) & 15u;
    // Messages fit up to the first whose end lies past cap; that one (it has
    // bytes, so it is the only one with p <= cap < q) names the end instead.
    if (tid == 0) s_wend[par] = end <= o.cap ? end : begin;
    __syncthreads();  // and the stage's last copy-out is over
    const u64 i = i0 + tid;
    u32 st = QB_ENC_STATUS_COUNT;  // no message: counted nowhere
    if (i < M) {
      const u32 p = pre[i], q = pre[i + 1];
      const Msg m = src.get(i);
      st = m.st;
      if (st <= QB_ENC_ENTRIES) {
        // q - p is this message's length unless the caller changed the
        // columns between the passes: then nothing of it is written
        if (q > o.cap || q - p != size_of(m)) {
          st = QB_ENC_NO_SPACE;
          if (p <= o.cap && q > o.cap) s_wend[par] = p;
        } else {
          encode(stage + shift + (p - begin), m);
        }
        if (o.ent_at && st <= QB_ENC_ENTRIES) o.ent_at[i] = head_size(m);
      }
      o.msg_off[i] = p;
      o.status[i] = u8(st);
    }
#pragma unroll
    for (u32 k = 0; k < QB_ENC_STATUS_COUNT; ++k) tally.add(int(k), st == k);
    __syncthreads();
    const u32 wend = s_wend[par];
    const u32 n = wend > begin ? wend - begin : 0u;
    u8* dst = o.bytes + begin;
    const u8* src_b = stage + shift;
    const u32 lead = (16u - shift) & 15u;
    const u32 head = lead < n ? lead : n;
    const u32 nblk = (n - head) / 16u, tail0 = head + 16u * nblk;
    if (tid < head) dst[tid] = src_b[tid];
    for (u32 b = tid; b < nblk; b += kBlock)
      *reinterpret_cast<uint4*>(dst + head + 16u * b) =
          *reinterpret_cast<const uint4*>(src_b + head + 16u * b);
    if (tid >= 64u && tail0 + (tid - 64u) < n) dst[tail0 + tid - 64u] = src_b[tail0 + tid - 64u];
  }
  __syncthreads();  // tl zeroed (a block with no tile passed no barrier)
  tally.stage(tl);
  __syncthreads();
  if (o.stats) BlockTally<QB_ENC_STATUS_COUNT>::publish(tl, reinterpret_cast<u64*>(o.stats));
}

static_assert(QB_ENC_OK == 0 && QB_ENC_ENTRIES == 1 && QB_ENC_NO_SPACE == QB_ENC_STATUS_COUNT - 1,
              "written statuses first; the counters follow the statuses");
static_assert(sizeof(qb_msg_out) == 40, "qb_msg_out");

}  // namespace enc
}  // namespace qb

using namespace qb;

namespace {
// Workspace: the lengths / offsets (+ the total), their scan's block sums and
// the slot front end's group of each slot.
struct Carve {
  size_t len, bsum, sgrp, total;
};
Carve carve(u64 M) {
  Carve c{};
  Carver k;
  c.len = k.take(sizeof(u32) * (M + 1));
  c.bsum = k.take(sizeof(u32) * (scan::blocks(M) + 1));
  c.sgrp = k.take(sizeof(u32) * M);
  c.total = k.o;
  return c;
}

bool fits(u64 M) { return M < (1ull << 32) && M * QB_ENC_MAX_BYTES < (1ull << 32); }

int check_out(const char* who, u64 M, const qb_encode_out* out, const void* workspace,
              size_t workspace_bytes) {
  QB_REQUIRE(out, "%s: out is NULL", who);
  QB_REQUIRE(out->msg_off && out->nbytes, "%s: msg_off / nbytes is NULL", who);
  if (M == 0) return QB_OK;
  QB_REQUIRE(out->status, "%s: status is NULL", who);
  QB_REQUIRE(out->bytes || out->cap == 0, "%s: bytes is NULL with cap %llu", who,
             (unsigned long long)out->cap);
  QB_REQUIRE(fits(M), "%s: %llu messages of up to %d bytes pass 2^32 (the offsets' scan is 32-bit)",
             who, (unsigned long long)M, QB_ENC_MAX_BYTES);
  QB_REQUIRE(workspace && workspace_bytes >= carve(M).total,
             "%s: workspace too small (qb_encode_scratch_bytes)", who);
  return QB_OK;
}

int check_groups(const char* who, const qb_encode_groups* eg) {
  QB_REQUIRE(eg, "%s: eg is NULL", who);
  QB_REQUIRE(eg->G == 0 || (eg->off && eg->ids && eg->self_id && eg->term),
             "%s: required group pointer is NULL", who);
  QB_REQUIRE(eg->G <= QB_READY_MAX_GROUPS, "%s: G %llu > %llu", who, (unsigned long long)eg->G,
             (unsigned long long)QB_READY_MAX_GROUPS);
  return QB_OK;
}

// No message: *nbytes = 0 and msg_off[0] = 0.
int run_empty(const qb_encode_out* out, hipStream_t st) {
  hipError_t e = hipMemsetAsync(out->nbytes, 0, sizeof(u64), st);
  if (e == hipSuccess) e = hipMemsetAsync(out->msg_off, 0, sizeof(u64), st);
  return e == hipSuccess ? QB_OK : hip_fail(e, "hipMemsetAsync(nbytes)");
}

template <class Src>
int run(const Src& src, u64 M, const qb_encode_out* out, void* workspace, hipStream_t st) {
  const Carve cv = carve(M);
  char* ws = static_cast<char*>(workspace);
  u32* len = reinterpret_cast<u32*>(ws + cv.len);
  hipLaunchKernelGGL(enc::k_enc_size<Src>, dim3(stream_grid<enc::k_enc_size<Src>>(M)), dim3(kBlock),
                     0, st, src, M, len);
  QB_CHECK_LAUNCH("k_enc_size");
  scan::launch(len, M, reinterpret_cast<u32*>(ws + cv.bsum), st);
  QB_CHECK_LAUNCH("scan(encode)");
  hipLaunchKernelGGL(enc::k_enc_write<Src>, dim3(stream_grid<enc::k_enc_write<Src>>(M)),
                     dim3(kBlock), 0, st, src, M, len, *out);
  QB_CHECK_LAUNCH("k_enc_write");
  return QB_OK;
}
}  // namespace

extern "C" size_t qb_encode_scratch_bytes(uint64_t M) { return fits(M) ? carve(M).total : 0; }

extern "C" int qb_dev_encode_messages(uint64_t M, const qb_encode_cols* c, const qb_encode_out* out,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  static const char* who = "qb_dev_encode_messages";
  if (const int rc = check_out(who, M, out, workspace, workspace_bytes)) return rc;
  if (M == 0) return run_empty(out, as_stream(stream));
  QB_REQUIRE(c && c->type, "%s: c / c->type is NULL", who);
  return run(enc::ColSrc{*c}, M, out, workspace, as_stream(stream));
}

extern "C" int qb_dev_encode_msg_out(const qb_encode_groups* eg, const qb_msg_out* msgs,
                                     uint64_t msg_cap, const uint64_t* msg_total,
                                     const qb_encode_out* out, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  static const char* who = "qb_dev_encode_msg_out";
  if (const int rc = check_groups(who, eg)) return rc;
  const u64 M = eg->G == 0 ? 0 : msg_cap;
  if (const int rc = check_out(who, M, out, workspace, workspace_bytes)) return rc;
  if (M == 0) return run_empty(out, as_stream(stream));
  QB_REQUIRE(msgs, "%s: msgs is NULL", who);
  return run(enc::ListSrc{*eg, msgs, reinterpret_cast<const u64*>(msg_total)}, M, out, workspace,
             as_stream(stream));
}

extern "C" int qb_dev_encode_slots(const qb_encode_groups* eg, const qb_encode_slot_cols* s,
                                   const qb_encode_out* out, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  static const char* who = "qb_dev_encode_slots";
  if (const int rc = check_groups(who, eg)) return rc;
  QB_REQUIRE(s, "%s: s is NULL", who);
  const u64 M = eg->G == 0 ? 0 : s->S;
  if (const int rc = check_out(who, M, out, workspace, workspace_bytes)) return rc;
  hipStream_t st = as_stream(stream);
  if (M == 0) return run_empty(out, st);
  u32* sgrp = reinterpret_cast<u32*>(static_cast<char*>(workspace) + carve(M).sgrp);
  const unsigned tiles = grid_for(eg->G);
  hipLaunchKernelGGL(enc::k_slot_groups, dim3(tiles < kStreamBlocks ? tiles : kStreamBlocks),
                     dim3(kBlock), 0, st, u64(eg->G), eg->off, M, sgrp);
  QB_CHECK_LAUNCH("k_slot_groups");
  return run(enc::SlotSrc{*eg, *s, sgrp}, M, out, workspace, st);
}
