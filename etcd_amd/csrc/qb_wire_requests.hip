// qb_wire_requests.hip — request wire ingest: raw raftpb.Message bytes -> the
// dense inputs of qb_dev_leader_requests (qb_request_in) and
// qb_dev_leader_propose (qb_propose_in), gfx950.  DESIGN.md §3.8f.
//
// What a leader receives from its followers' clients: MsgProp, MsgReadIndex
// and MsgTransferLeader (forwarded, raft.go:1423-1470), and what a follower
// gets back, MsgReadIndexResp.  Validation is Message.Unmarshal as the other
// two ingests have it (qb_wire_decode.h); the Message decoder's entry sink
// sees every Entry's Type and the byte range of its Data, which is read only
// where it is a conf change (ConfChange / ConfChangeV2.Unmarshal,
// raft.pb.go:2543-2908) or a read's request id.
//
//   pass 1 (k_request_decode, k_request_decode_global): one thread per
//     message, 256 messages per workgroup, the workgroup's byte span staged in
//     LDS as k_follower_decode stages it; a message outside the stage is
//     decoded from global memory by the second launch.  Writes the
//     message-aligned columns and the pass-1 status, and counts the group's
//     OK requests (kinds 1-3) into cnt.
//   scan + k_request_scatter: the counting sort by group of the follower steps
//     (qb_follower_impl.h F2-F3): perm holds each group's requests, in the
//     order the atomics took.
//   pass 2 (k_request_combine): a thread per group, capped grid.  A run of up
//     to kInline requests is sorted by batch index in place and walked: a
//     request is taken into the dense columns or, by the rules of the header,
//     deferred with every later one of its group.  A group without requests
//     reads its count and writes the nine dense defaults.  A longer run is
//     listed for k_request_long: a workgroup per listed group sorts the run
//     (fol::block_bitonic) and one thread walks it — the fallback for any
//     skew: one group may hold the whole batch.
#include "qb_follower_impl.h"
#include "qb_scan.h"
#include "qb_span_tile.h"
#include "qb_wire_decode.h"

namespace qb {
namespace rqw {

using wire::Fields;
using wire::K_MESSAGE;
using wire::kStage;
using wire::LdsSrc;
using wire::WinSrc;

constexpr u32 kInline = 16;        // k_request_combine sorts and walks runs up to this itself
constexpr u32 kLdsRun = 4096;      // k_request_long sorts runs up to this in LDS
constexpr unsigned kCombineBlocks = 2048;
constexpr unsigned kLongBlocks = 256;
constexpr u32 kNoCc = 0xFFFFFFFFu;  // cc_at of a MsgProp without a conf change
constexpr u8 kLocal = 0xFF, kNoSlot = 0xFE;
constexpr u64 kMaxM = 0xFFFFFFFEull;

struct Args {
  u64 M, nbytes, G;
  const u8* bytes;
  const u64* moff;
  const u32* mgroup;
  const u32* off;
  const u64* ids;
  u32 max_reads, concat;
  qb_request_wire_out o;
  u64* stats;   // nullable
  u32* cnt;     // [G + 1] counts -> run starts -> run ends
  u32* perm;    // [M] batch indices, grouped
  u32* longs;   // [M / (kInline + 1) + 1] groups with a run past kInline
  u32* nlong;
};

// ConfChange (V1), ConfChangeV2 and ConfChangeSingle.Unmarshal on [i, l):
// varint fields, one bytes field (Context), V2's repeated ConfChangeSingle;
// everything else skipRaft.  *changes counts V2's field-2 fields.
enum CcKind : u32 { CC_V1 = 0, CC_V2 = 1, CC_SINGLE = 2 };
template <u32 KIND, class Src>
__device__ __forceinline__ bool unmarshal_cc(const Src& s, u64 i, const u64 l, u32* changes) {
  while (i < l) {
    const u64 pre = i;
    u64 key;
    if (!wire::varint(s, i, l, key)) return false;
    const int fnum = int(u32(key >> 3));
    const u32 wt = u32(key & 7u);
    if (wt == 4) return false;
    if (fnum <= 0) return false;
    const bool is_varint = KIND == CC_V1 ? (fnum >= 1 && fnum <= 3)
                                         : (KIND == CC_V2 ? fnum == 1 : (fnum == 1 || fnum == 2));
    const bool is_bytes = KIND == CC_V1 ? fnum == 4 : (KIND == CC_V2 && fnum == 3);
    const bool is_nested = KIND == CC_V2 && fnum == 2;
    if (is_varint) {
      u64 v;
      if (wt != 0 || !wire::varint(s, i, l, v)) return false;
    } else if (is_bytes || is_nested) {
      u64 len;
      if (wt != 2 || !wire::varint(s, i, l, len)) return false;
      if (int64_t(len) < 0) return false;
      const u64 post = i + len;
      if (post < i || post > l) return false;
      if constexpr (KIND == CC_V2) {
        if (is_nested) {
          if (!unmarshal_cc<CC_SINGLE>(s, i, post, nullptr)) return false;
          ++*changes;
        }
      }
      i = post;
    } else {
      i = pre;
      if (!wire::skip_field_body(s, i, l)) return false;  // (inline, as for a kWantsBody sink)
    }
  }
  return true;
}

// The entry sink: the entries' count, byte range and payload, and the conf
// change among them.  A conf-change entry is validated wherever it stands (the
// message's Type may come behind it); only a MsgProp uses the result.
template <class Src>
struct ReqSink {
  static constexpr bool kWantsBody = true;
  const Src& s;
  u64 e_term = 0, e_index = 0, e_type = 0, e_data_pos = 0, e_data_len = 0;
  u64 lo = 0, hi = 0, payload = 0, cc_payload = 0;
  u32 n = 0, cc_n = 0, cc_at = 0;
  bool gap = false, cc_bad = false, cc_leave = false;
  __device__ __forceinline__ explicit ReqSink(const Src& s_) : s(s_) {}
  __device__ __forceinline__ void entry(u64 pre, u64 post) {
    if (n == 0) lo = pre;
    else gap |= pre != hi;
    hi = post;
    payload += e_data_len;  // PayloadSize (util.go:160)
    const u32 t = u32(e_type);  // EntryType is an int32
    if (t == 1u || t == 2u) {
      u32 changes = 0;
      const bool ok = t == 1u ? unmarshal_cc<CC_V1>(s, e_data_pos, e_data_pos + e_data_len, nullptr)
                              : unmarshal_cc<CC_V2>(s, e_data_pos, e_data_pos + e_data_len, &changes);
      if (!ok || cc_n) cc_bad = true;
      if (cc_n == 0) {
        cc_at = n;
        cc_payload = e_data_len;
        cc_leave = t == 2u && changes == 0;  // len(cc.AsV2().Changes) == 0 (raft.go:1053)
      }
      ++cc_n;
    }
    ++n;
  }
};

struct Rec {
  u32 st, group;
  u8 kind, type, slot, cc_leave;
  u64 from, term, ctx, index, payload, epos, cc_payload;
  u32 en, ebytes, cc_at;
};

// From's slot among ids[off[g] .. off[g + 1]) (at most QB_MAX_SLOTS of them,
// as the requests step reads a config), kNoSlot for a non-member.
__device__ __forceinline__ u8 slot_of(const Args& A, u32 g, u64 from) {
  if (u64(g) >= A.G) return kNoSlot;
  const u32 s0 = A.off[g], s1 = A.off[g + 1];
  const u32 n = clamp_slots(s0, s1);
  u32 slot = kNoSlot;
  for (u32 j = 0; j < n && slot == kNoSlot; j += 4) {  // four IDs per round trip
    u64 v[4];
#pragma unroll
    for (u32 q = 0; q < 4; ++q) v[q] = A.ids[u64(s0) + (j + q < n ? j + q : n - 1)];
#pragma unroll
    for (u32 q = 4; q-- > 0;)
      if (j + q < n && v[q] == from) slot = j + q;
  }
  return u8(slot);
}

// The one entry of a read request or its response: 8 bytes of Data, not all
// zero, as a big-endian id.
template <class Src>
__device__ __forceinline__ bool read_ctx(const Src& s, const ReqSink<Src>& k, u64* ctx) {
  if (k.n != 1 || k.e_data_len != 8) return false;
  *ctx = wire::load_be64(s, k.e_data_pos);
  return *ctx != 0;
}

template <class Src>
__device__ __forceinline__ Rec decode_request(const Args& A, const Src& s, u64 p0, u64 p1, u32 mg) {
  Rec r{QB_WIRE_UNMARSHAL, 0xFFFFFFFFu, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  Fields f = Fields{};
  ReqSink<Src> sink(s);
  bool ok = p0 <= p1 && p1 <= A.nbytes;
  if (ok) {
    u64 i = p0;
    ok = wire::fast_prefix(s, i, p1, f);
    if (ok) ok = wire::fast_tail12(s, i, p1, f);
    if (ok) ok = wire::unmarshal<K_MESSAGE>(s, i, p1, &f, &sink);
  }
  if (!ok) return r;
  const u32 t = u32(f.type);  // MessageType is an int32: the varint's low 32 bits
  r.st = QB_WIRE_OK;
  r.group = mg;
  r.type = u8(t);
  r.from = f.from;
  r.term = f.term;
  switch (t) {
    case 2: {  // MsgProp
      r.kind = QB_RQ_PROP;
      r.en = sink.n;
      r.payload = sink.payload;
      const bool whole = sink.n != 0 && !sink.gap;
      r.epos = whole ? sink.lo : 0ull;
      r.ebytes = whole ? u32(sink.hi - sink.lo) : 0u;
      const bool cc = sink.cc_n != 0 && !sink.cc_bad;
      r.cc_at = cc ? sink.cc_at : kNoCc;
      r.cc_payload = cc ? sink.cc_payload : 0ull;
      r.cc_leave = cc && sink.cc_leave;
      if (f.term != 0) r.st = QB_WIRE_TERM;
      else if (!whole) r.st = QB_WIRE_ENTRIES;
      else if (sink.cc_bad) r.st = QB_WIRE_CONF_CHANGE;
      break;
    }
    case 15: {  // MsgReadIndex
      r.kind = QB_RQ_READ;
      const bool good = read_ctx(s, sink, &r.ctx);
      if (!good) r.ctx = 0;
      r.slot = f.from == 0 ? kLocal : slot_of(A, mg, f.from);
      if (f.term != 0) r.st = QB_WIRE_TERM;
      else if (!good) r.st = QB_WIRE_CTX;
      break;
    }
    case 13:  // MsgTransferLeader
      r.kind = QB_RQ_TRANSFER;
      r.slot = f.from == 0 ? kNoSlot : slot_of(A, mg, f.from);  // (None is nobody's ID)
      break;
    case 16: {  // MsgReadIndexResp: decoded, the host steps it
      r.kind = QB_RQ_READ_RESP;
      r.index = f.index;
      if (!read_ctx(s, sink, &r.ctx)) {
        r.ctx = 0;
        r.st = QB_WIRE_CTX;
      }
      break;
    }
    default:
      r.st = QB_WIRE_TYPE;
      break;
  }
  // the dense columns have no place for it (a response takes none)
  if (r.st == QB_WIRE_OK && r.kind != QB_RQ_READ_RESP && u64(mg) >= A.G) r.st = QB_WIRE_GROUP;
  return r;
}

// A message pass 1's first launch leaves to its second (the status between
// the two launches only; never returned).
constexpr u8 kPending = 0xFF;

__device__ __forceinline__ bool grouped(u32 st, u32 kind) {
  return st == QB_WIRE_OK && kind >= QB_RQ_PROP && kind <= QB_RQ_TRANSFER;
}

// One message's columns (write-once, read by a later launch: nontemporal),
// and its place in its group's count.
__device__ __forceinline__ void emit(const Args& A, u64 m, const Rec& r) {
  const qb_request_wire_out& o = A.o;
  A.o.kind[m] = r.kind;  // pass 2 reads these two back
  A.o.status[m] = u8(r.st);
  __builtin_nontemporal_store(r.group, o.group + m);
  __builtin_nontemporal_store(r.from, reinterpret_cast<u64*>(o.from) + m);
  __builtin_nontemporal_store(r.term, reinterpret_cast<u64*>(o.term) + m);
  __builtin_nontemporal_store(r.type, o.msg_type + m);
  __builtin_nontemporal_store(r.slot, o.slot + m);
  __builtin_nontemporal_store(r.ctx, reinterpret_cast<u64*>(o.ctx) + m);
  __builtin_nontemporal_store(r.index, reinterpret_cast<u64*>(o.index) + m);
  __builtin_nontemporal_store(r.en, o.ent_n + m);
  __builtin_nontemporal_store(r.payload, reinterpret_cast<u64*>(o.payload) + m);
  __builtin_nontemporal_store(r.epos, reinterpret_cast<u64*>(o.ent_pos) + m);
  __builtin_nontemporal_store(r.ebytes, o.ent_bytes + m);
  __builtin_nontemporal_store(r.cc_at, o.cc_at + m);
  __builtin_nontemporal_store(r.cc_payload, reinterpret_cast<u64*>(o.cc_payload) + m);
  __builtin_nontemporal_store(r.cc_leave, o.cc_leave + m);
  o.rd_k[m] = 0;  // pass 2 writes the taken ones
  o.ent_base[m] = 0;
  if (grouped(r.st, r.kind)) atomicAdd(A.cnt + r.group, 1u);  // (group < G: QB_WIRE_GROUP otherwise)
}

// The final statuses pass 1 knows (a response's OK among them; the requests'
// OK and DEFERRED are pass 2's).
constexpr int kP1 = 9;
__device__ __forceinline__ void tally_flush(const Args& A, u32* lds, u32 st_, u32 kind) {
  BlockTally<kP1> tally;
  const bool resp = st_ == QB_WIRE_OK && kind == QB_RQ_READ_RESP;
  tally.add(0, st_ == QB_WIRE_UNMARSHAL);
  tally.add(1, st_ == QB_WIRE_TYPE);
  tally.add(2, st_ == QB_WIRE_CTX);
  tally.add(3, st_ == QB_WIRE_ENTRIES);
  tally.add(4, st_ == QB_WIRE_TERM);
  tally.add(5, st_ == QB_WIRE_CONF_CHANGE);
  tally.add(6, st_ == QB_WIRE_GROUP);
  tally.add(7, resp);
  tally.add(8, resp);
  const int slot[kP1] = {QB_WIRE_UNMARSHAL, QB_WIRE_TYPE,  QB_WIRE_CTX, QB_WIRE_ENTRIES,     QB_WIRE_TERM,
                         QB_WIRE_CONF_CHANGE, QB_WIRE_GROUP, QB_WIRE_OK,  QB_RWSTAT_READ_RESPS};
  if (A.stats) tally.flush(lds, A.stats, slot);
}

// Pass 1, first launch: k_follower_decode's shape.  Round trips per
// workgroup: the message offsets and groups, then the LDS-DMA stage of the
// byte span; the messages are parsed from LDS.  A message outside the staged
// span (its block's span does not fit) is left to the second launch.
__global__ __launch_bounds__(kBlock) void k_request_decode(Args A) {
  __shared__ __attribute__((aligned(16))) u8 stage[kStage + 48];  // + window over-reads (<= 24 B past a message)
  __shared__ u32 lds[kP1];
  const u64 m0 = u64(blockIdx.x) * kBlock;
  const u64 m = m0 + threadIdx.x;
  const u64 mlast = (m0 + kBlock < A.M ? m0 + kBlock : A.M);
  const u64 mc = m < A.M ? m : A.M - 1;  // lanes past M re-read the last message
  const u64 b0 = A.moff[m0], b1 = A.moff[mlast];
  const u64 p0 = __builtin_nontemporal_load(A.moff + mc);
  const u64 p1 = __builtin_nontemporal_load(A.moff + mc + 1);
  const u32 mg = __builtin_nontemporal_load(A.mgroup + mc);
  // Stage the block's byte span [b0, b1) when it fits (block-uniform).
  u64 lbase = 0, lend = 0;  // staged span (empty: nothing staged)
  if (b1 > b0 && b1 - b0 <= kStage - 16) {
    const u64 a0 = b0 & ~u64(15);  // 16-byte aligned window
    const u64 a1 = (b1 + 15) & ~u64(15);
    const u64 n16 = (a1 - a0) / 16;
    // Pieces wholly inside the byte buffer go by LDS-DMA (an aligned buffer)
    // or plain loads; only the buffer's last piece can be partial, and offsets
    // past the buffer stage nothing from it.
    const u64 whole = a0 < A.nbytes ? (A.nbytes - a0) / 16 : 0;
    const u32 nfull = u32(n16 < whole ? n16 : whole);
    if ((reinterpret_cast<uintptr_t>(A.bytes) & 15u) == 0) {
      constexpr int kIt = int((kStage + 16) / 16 / kBlock) + 1;
      stage16_lds<kBlock, kIt>(stage, A.bytes + a0, nfull);
    } else {
      const uint4* gsrc = reinterpret_cast<const uint4*>(A.bytes + a0);
      for (u64 k = threadIdx.x; k < nfull; k += kBlock) reinterpret_cast<uint4*>(stage)[k] = gsrc[k];
    }
    for (u64 k = nfull + threadIdx.x; k < n16; k += kBlock)
      for (u32 t = 0; t < 16; ++t) {
        const u64 p = a0 + 16 * k + t;
        stage[16 * k + t] = p < A.nbytes ? A.bytes[p] : 0;
      }
    lbase = a0;
    lend = a1 < A.nbytes ? a1 : A.nbytes;
  }
  __syncthreads();
  u32 st_ = kPending, kind = 0;
  if (m < A.M) {
    if (p0 >= lbase && p1 <= lend && p0 <= p1) {
      const Rec r = decode_request(A, LdsSrc{stage, lbase}, p0, p1, mg);
      st_ = r.st;
      kind = r.kind;
      emit(A, m, r);
    } else {
      A.o.status[m] = kPending;
    }
  }
  tally_flush(A, lds, st_, kind);
}

// Pass 1, second launch: the messages the first left, each decoded from
// global memory through the 8-byte window (wire::WinSrc).  With nothing left
// the launch reads the status column once.
__global__ __launch_bounds__(kBlock) void k_request_decode_global(Args A) {
  __shared__ u32 lds[kP1];
  const u64 m = u64(blockIdx.x) * kBlock + threadIdx.x;
  u32 st_ = kPending, kind = 0;
  if (m < A.M && A.o.status[m] == kPending) {
    const Rec r = decode_request(A, WinSrc(A.bytes, A.nbytes), A.moff[m], A.moff[m + 1], A.mgroup[m]);
    st_ = r.st;
    kind = r.kind;
    emit(A, m, r);
  }
  tally_flush(A, lds, st_, kind);
}

// F3 of the follower steps: perm[cnt[group]++] = batch index.  After it
// cnt[g] is the end of group g's run (its start is cnt[g - 1]).
__global__ __launch_bounds__(kBlock) void k_request_scatter(Args A) {
  const u64 i = u64(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= A.M || !grouped(A.o.status[i], A.o.kind[i])) return;
  const u32 g = A.o.group[i];
  if (u64(g) >= A.G) return;  // (never: pass 1 answered QB_WIRE_GROUP)
  const u32 pos = atomicAdd(A.cnt + g, 1u);
  if (u64(pos) < A.M) A.perm[pos] = u32(i);
}

// group g's run [b, e) of perm; an inconsistent table yields an empty run
__device__ __forceinline__ void run_of(const Args& A, u64 g, u32& b, u32& e) {
  b = g ? A.cnt[g - 1] : 0u;
  e = A.cnt[g];
  if (e < b || u64(e) > A.M) e = b = 0;
}

// what pass 2 counts per thread
struct Counts {
  u32 props = 0, reads = 0, xfers = 0, deferred = 0;
  u64 ents = 0;
};

// Group g's nine dense words (rd_ctx / rd_from rows are the walk's): a thread
// per group, so each is a coalesced store.
__device__ __forceinline__ void write_dense(const Args& A, u64 g, u8 n_reads, u8 xf_from, u64 xf_term,
                                            u8 action, u32 n_ents, u64 payload, u32 cc_at,
                                            u64 cc_payload, u8 gflags) {
  const qb_request_wire_out& o = A.o;
  o.n_reads[g] = n_reads;
  o.xf_from[g] = xf_from;
  reinterpret_cast<u64*>(o.xf_term)[g] = xf_term;
  o.action[g] = action;
  o.n_ents[g] = n_ents;
  reinterpret_cast<u64*>(o.g_payload)[g] = payload;
  o.g_cc_at[g] = cc_at;
  reinterpret_cast<u64*>(o.g_cc_payload)[g] = cc_payload;
  o.gflags[g] = gflags;
}

// Group g's requests run[0, n), ascending batch indices: each is taken or, by
// the header's rules, deferred with every later one.
__device__ __forceinline__ void walk_group(const Args& A, u64 g, const u32* run, u32 n, Counts& c) {
  const qb_request_wire_out& o = A.o;
  u32 nr = 0, n_ents = 0, cc_at = 0;
  u64 payload = 0, cc_payload = 0, xf_term = 0;
  u8 action = QB_PROP_NONE, xf_from = kLocal;
  bool prop = false, cc = false, xfer = false, deferred = false;
  u32 j = 0;
  for (; j < n; ++j) {
    const u32 i = run[j];
    if (u64(i) >= A.M) continue;  // (never, for a batch that does not change under the call)
    const u32 kind = o.kind[i];
    if (kind == QB_RQ_READ) {
      if (prop || nr >= A.max_reads) break;
      const u64 at = u64(nr) * A.G + g;
      reinterpret_cast<u64*>(o.rd_ctx)[at] = reinterpret_cast<const u64*>(o.ctx)[i];
      o.rd_from[at] = o.slot[i];
      o.rd_k[i] = u8(nr);
      ++nr;
      ++c.reads;
    } else if (kind == QB_RQ_TRANSFER) {
      if (prop || xfer) break;
      xfer = true;
      xf_from = o.slot[i];
      xf_term = reinterpret_cast<const u64*>(o.term)[i];
      ++c.xfers;
    } else {  // QB_RQ_PROP
      const u32 en = o.ent_n[i];
      const u32 at = o.cc_at[i];
      if (prop && (!A.concat || (at != kNoCc && cc) || u64(n_ents) + en > 0xFFFFFFFFull)) break;
      if (at != kNoCc) {
        cc = true;
        cc_at = n_ents + at;
        cc_payload = reinterpret_cast<const u64*>(o.cc_payload)[i];
        action |= u8(QB_PROP_CONF_CHANGE | (o.cc_leave[i] ? QB_PROP_CC_LEAVE_JOINT : 0u));
      }
      prop = true;
      action |= QB_PROP_ENTRIES;
      o.ent_base[i] = n_ents;
      n_ents += en;
      payload += reinterpret_cast<const u64*>(o.payload)[i];
      ++c.props;
      c.ents += en;
    }
  }
  const bool took = j != 0;
  for (; j < n; ++j) {
    if (u64(run[j]) < A.M) o.status[run[j]] = QB_WIRE_DEFERRED;
    deferred = true;
    ++c.deferred;
  }
  write_dense(A, g, u8(nr), xf_from, xf_term, action, n_ents, payload, cc_at, cc_payload,
              u8((took ? QB_RWFLAG_TAKEN : 0u) | (deferred ? QB_RWFLAG_DEFERRED : 0u)));
}

// Every thread of the block calls it.  lds: 5 u32 and one u64.
__device__ __forceinline__ void flush_counts(const Args& A, const Counts& c, u32* lds, u64* lds64) {
  if (!A.stats) return;  // (kernel-uniform)
  BlockTally<5> t;
  t.add_n(0, c.props);
  t.add_n(1, c.reads);
  t.add_n(2, c.xfers);
  t.add_n(3, c.deferred);
  t.add_n(4, c.props + c.reads + c.xfers);
  const int slot[5] = {QB_RWSTAT_TAKEN_PROPS, QB_RWSTAT_TAKEN_READS, QB_RWSTAT_TAKEN_TRANSFERS,
                       QB_WIRE_DEFERRED, QB_WIRE_OK};
  t.flush(lds, A.stats, slot);
  u64 ents = c.ents;  // a u64 sum per wave, per workgroup in LDS, one atomic per workgroup
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ents += u64(__shfl_xor(ents, o, 64));
  if (threadIdx.x == 0) *lds64 = 0;
  __syncthreads();
  if ((threadIdx.x & 63) == 0 && ents) atomicAdd(lds64, ents);
  __syncthreads();
  if (threadIdx.x == 0 && *lds64) atomicAdd(A.stats + QB_RWSTAT_ENTRIES_TAKEN, *lds64);
}

__global__ __launch_bounds__(kBlock) void k_request_combine(Args A) {
  __shared__ u32 sh[5];
  __shared__ u64 she;
  const u64 ntiles = (A.G + kBlock - 1) / kBlock;
  Counts c;
  for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const u64 g = tile * kBlock + threadIdx.x;
    if (g >= A.G) continue;
    u32 b, e;
    run_of(A, g, b, e);
    const u32 n = e - b;
    if (n == 0) {
      write_dense(A, g, 0, kLocal, 0, QB_PROP_NONE, 0, 0, 0, 0, 0);
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
      walk_group(A, g, run, n, c);
    } else {
      const u32 s = atomicAdd(A.nlong, 1u);
      A.longs[s] = u32(g);  // (at most M / (kInline + 1) such groups)
    }
  }
  flush_counts(A, c, sh, &she);
}

__global__ __launch_bounds__(kBlock) void k_request_long(Args A) {
  __shared__ u32 run[kLdsRun];
  __shared__ u32 sh[5];
  __shared__ u64 she;
  const u32 nl = *A.nlong;
  Counts c;
  for (u32 q = blockIdx.x; q < nl; q += gridDim.x) {
    const u64 g = A.longs[q];
    u32 b, e;
    run_of(A, g, b, e);
    const u32 n = e - b;  // > kInline
    u32* pg = A.perm + b;
    if (n <= kLdsRun) {
      for (u32 i = threadIdx.x; i < n; i += kBlock) run[i] = pg[i];
      __syncthreads();
      fol::block_bitonic(n, [&](u32 i) { return run[i]; }, [&](u32 i, u32 v) { run[i] = v; });
      if (threadIdx.x == 0 && n) walk_group(A, g, run, n, c);
    } else {
      // in the workspace: device-scope accesses, so no lane reads a line its
      // CU cached before another wave's store
      __syncthreads();
      fol::block_bitonic(
          n, [&](u32 i) { return __hip_atomic_load(pg + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
          [&](u32 i, u32 v) { __hip_atomic_store(pg + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); });
      __threadfence();
      __syncthreads();
      if (threadIdx.x == 0) walk_group(A, g, pg, n, c);
    }
    __syncthreads();  // the LDS run is free for the next group
  }
  flush_counts(A, c, sh, &she);
}

}  // namespace rqw
}  // namespace qb

using namespace qb;

namespace {
// Workspace: the follower steps' layout (fol::carve: [cnt (G + 1) | nlong]
// zeroed per call, the scan's block sums, the long-run list, perm), whose
// kInline this file's list bound shares.
using Carve = fol::Carve;
static_assert(rqw::kInline == fol::kInline, "fol::carve sizes the long-run list by fol::kInline");
Carve carve(u64 G, u64 M) { return fol::carve(G, M); }
// M + 1 offsets, batch indices and counts of 32 bits; G + 1 counts of the 32-bit scan.
bool fits(u64 G, u64 M) { return M <= rqw::kMaxM && G <= rqw::kMaxM; }
}  // namespace

extern "C" size_t qb_wire_requests_scratch_bytes(uint64_t G, uint64_t M) {
  return fits(G, M) ? carve(G, M).total : 0;
}

extern "C" int qb_dev_ingest_requests(uint64_t M, const uint8_t* bytes, uint64_t nbytes,
                                      const uint64_t* msg_off, const uint32_t* msg_group, uint64_t G,
                                      const uint32_t* off, const uint64_t* ids, uint32_t max_reads,
                                      uint32_t concat, const qb_request_wire_out* out, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  static const char* who = "qb_dev_ingest_requests";
  QB_REQUIRE(out, "%s: out is NULL", who);
  QB_REQUIRE(max_reads >= 1 && max_reads <= QB_REQ_MAX_READS, "%s: max_reads %u outside 1..%d", who,
             max_reads, QB_REQ_MAX_READS);
  if (G == 0) return QB_OK;
  QB_REQUIRE(off && ids, "%s: off / ids is NULL", who);
  QB_REQUIRE(out->n_reads && out->rd_ctx && out->rd_from && out->xf_from && out->xf_term &&
                 out->action && out->n_ents && out->g_payload && out->g_cc_at && out->g_cc_payload &&
                 out->gflags,
             "%s: a dense output (n_reads, rd_ctx, rd_from, xf_from, xf_term, action, n_ents, "
             "g_payload, g_cc_at, g_cc_payload, gflags) is NULL",
             who);
  if (M) {
    QB_REQUIRE(msg_off && msg_group, "%s: msg_off / msg_group is NULL", who);
    QB_REQUIRE(nbytes == 0 || bytes, "%s: bytes is NULL", who);
    QB_REQUIRE(out->kind && out->status && out->group && out->from && out->term && out->msg_type &&
                   out->slot && out->ctx && out->index && out->ent_n && out->payload && out->ent_pos &&
                   out->ent_bytes && out->cc_at && out->cc_payload && out->cc_leave && out->rd_k &&
                   out->ent_base,
               "%s: a message column (kind, status, group, from, term, msg_type, slot, ctx, index, "
               "ent_n, payload, ent_pos, ent_bytes, cc_at, cc_payload, cc_leave, rd_k, ent_base) is NULL",
               who);
  }
  QB_REQUIRE(M <= rqw::kMaxM, "%s: %llu messages pass 2^32 - 2", who, (unsigned long long)M);
  QB_REQUIRE(G <= rqw::kMaxM, "%s: %llu groups pass 2^32 - 2", who, (unsigned long long)G);
  QB_REQUIRE(nbytes < (1ull << 32), "%s: %llu bytes pass 2^32 (ent_bytes and ent_n are 32-bit)", who,
             (unsigned long long)nbytes);
  const Carve cv = carve(G, M);
  QB_REQUIRE(workspace && workspace_bytes >= cv.total,
             "%s: workspace too small (qb_wire_requests_scratch_bytes)", who);
  hipStream_t st = as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  rqw::Args A{M, nbytes, G, bytes, reinterpret_cast<const u64*>(msg_off), msg_group, off,
              reinterpret_cast<const u64*>(ids), max_reads, concat, *out,
              reinterpret_cast<u64*>(out->stats), reinterpret_cast<u32*>(ws + cv.cnt),
              reinterpret_cast<u32*>(ws + cv.perm), reinterpret_cast<u32*>(ws + cv.longs),
              reinterpret_cast<u32*>(ws + cv.nlong)};
  hipError_t e = hipMemsetAsync(ws + cv.cnt, 0, cv.zero_end - cv.cnt, st);
  if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(request wire counts)");
  if (M) {
    hipLaunchKernelGGL(rqw::k_request_decode, dim3(grid_for(M)), dim3(kBlock), 0, st, A);
    QB_CHECK_LAUNCH("k_request_decode");
    hipLaunchKernelGGL(rqw::k_request_decode_global, dim3(grid_for(M)), dim3(kBlock), 0, st, A);
    QB_CHECK_LAUNCH("k_request_decode_global");
    scan::launch(A.cnt, G, reinterpret_cast<u32*>(ws + cv.bsum), st);
    QB_CHECK_LAUNCH("scan(request wire)");
    hipLaunchKernelGGL(rqw::k_request_scatter, dim3(grid_for(M)), dim3(kBlock), 0, st, A);
    QB_CHECK_LAUNCH("k_request_scatter");
  }
  const unsigned tiles = grid_for(G);
  hipLaunchKernelGGL(rqw::k_request_combine,
                     dim3(tiles < rqw::kCombineBlocks ? tiles : rqw::kCombineBlocks), dim3(kBlock), 0,
                     st, A);
  QB_CHECK_LAUNCH("k_request_combine");
  if (M > rqw::kInline) {
    const u64 most = M / (rqw::kInline + 1);  // groups that can hold a long run
    hipLaunchKernelGGL(rqw::k_request_long,
                       dim3(unsigned(most < rqw::kLongBlocks ? most : rqw::kLongBlocks)), dim3(kBlock),
                       0, st, A);
    QB_CHECK_LAUNCH("k_request_long");
  }
  return QB_OK;
}
