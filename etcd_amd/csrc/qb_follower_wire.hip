// qb_follower_wire.hip — follower wire ingest: raw raftpb.Message bytes ->
// the follower steps' inbox (qb_follower_inbox / qb_follower_app_inbox),
// gfx950.  DESIGN.md §3.8e.
//
// What non-leader nodes receive: MsgHeartbeat, MsgVote / MsgPreVote,
// MsgTimeoutNow and MsgApp (raft.Step, raft.go:847-984, checks no membership
// for them, so there is no From-to-slot lookup and no group-row gather: the
// decode is a pure stream).  Validation is Message.Unmarshal exactly as the
// leader's ingest has it (qb_wire_decode.h; raft.pb.go:1739-2061); the Message
// decoder's entry sink sees every Entry's Term, Index and byte range, Entry
// Data is skipped by its length and never read.
//
//   pass 1 (k_follower_decode, k_follower_decode_global): one thread per
//     message, 256 messages per workgroup, the workgroup's byte span staged in
//     LDS by LDS-DMA exactly as k_ingest stages it; a message outside the
//     stage is decoded from global memory by the second launch.  Writes the
//     message-aligned columns, the status and the message's term-run count
//     (into ent_off).
//   scan: ent_off <- exclusive prefix sums, ent_off[M] <- the batch's runs.
//   pass 2 (k_follower_runs): each MsgApp with runs walks its entry range
//     again and writes (term, length) at ent_off[i]; a message whose runs end
//     past ent_cap is downgraded to QB_FIN_HOST / QB_WIRE_NO_SPACE.  The OK /
//     NO_SPACE counters are tallied here, the final statuses of pass 1 there.
//
// Not k_ingest's canonical-first / deferred pair: a MsgApp with entries leaves
// the canonical field order at field 7, so a launch for the non-canonical
// would take every one of them; the generic loop sits in the LDS launch.  The
// two launches of pass 1 are split by byte source instead.
#include "qb_scan.h"
#include "qb_wire_decode.h"

namespace qb {
namespace fwire {

using wire::Fields;
using wire::K_MESSAGE;
using wire::kStage;
using wire::LdsSrc;
using wire::WinSrc;

struct Args {
  u64 M, nbytes;
  const u8* bytes;
  const u64* moff;
  const u32* mgroup;
  u32* rg;
  u8* rf;
  u64 *rfrom, *rterm, *rindex, *raux, *rcommit;
  u8* status;
  u8* mtype;       // nullable
  u64* ent_pos;    // the caller's column or the workspace's
  u32* ent_bytes;  // the same
  u32* ent_n;      // nullable
  u32* ent_off;
  u64* ent_term;
  u32* ent_len;
  u64 ent_cap;
  u64* ent_total;
  u64* stats;      // nullable
};

// Pass 1's entry sink: the entries' count, byte range, term runs, and whether
// they are one contiguous range of field-7 fields with consecutive indexes.
struct CountSink {
  u64 e_term, e_index;  // the entry being decoded (0 where the field is absent)
  u64 lo, hi, first, next, last_term;
  u32 n, runs;
  bool bad;
  __device__ __forceinline__ void entry(u64 pre, u64 post) {
    if (n == 0) {
      lo = pre;
      first = e_index;
      runs = 1;
    } else {
      bad |= pre != hi || e_index != next;
      runs += e_term != last_term ? 1u : 0u;
    }
    hi = post;
    next = e_index + 1;  // wraps as Go's uint64
    last_term = e_term;
    ++n;
  }
};

// Pass 2's sink: the runs written at [pos, end).
struct RunSink {
  u64 e_term, e_index;
  u64 cur_term;
  u32 cur_len, n;
  u64* term;
  u32* len;
  u32 pos, end;
  __device__ __forceinline__ void put() {
    if (pos < end) {
      __builtin_nontemporal_store(cur_term, term + pos);
      __builtin_nontemporal_store(cur_len, len + pos);
    }
    ++pos;
  }
  __device__ __forceinline__ void entry(u64, u64) {
    if (n != 0 && e_term != cur_term) {
      put();
      cur_len = 0;
    }
    cur_term = e_term;
    ++cur_len;
    ++n;
  }
};

struct Rec {
  u32 st, group;
  u8 flags, type;
  u64 from, term, index, aux, commit, epos;
  u32 ebytes, en, runs;
};

// "CampaignTransfer" (raft.go:854) as two little-endian words.
constexpr u64 kXferLo = 0x6E676961706D6143ull;  // "Campaign"
constexpr u64 kXferHi = 0x726566736E617254ull;  // "Transfer"

template <class Src>
__device__ __forceinline__ u64 load_le64(const Src& s, u64 i) {
  return __builtin_bswap64(wire::load_be64(s, i));
}

template <class Src>
__device__ __forceinline__ Rec decode_follower(u64 nbytes, const Src& s, u64 p0, u64 p1, u32 mg) {
  Rec r{QB_WIRE_UNMARSHAL, 0xFFFFFFFFu, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  Fields f = Fields{};
  CountSink sink{};
  bool ok = p0 <= p1 && p1 <= nbytes;
  if (ok) {
    u64 i = p0;
    ok = wire::fast_prefix(s, i, p1, f, &f.commit);
    if (ok) ok = wire::fast_tail12(s, i, p1, f);
    if (ok) ok = wire::unmarshal<K_MESSAGE>(s, i, p1, &f, &sink);
  }
  if (!ok) return r;
  const u32 t = u32(f.type);  // MessageType is an int32: the varint's low 32 bits
  r.st = QB_WIRE_OK;
  r.group = mg;
  r.flags = QB_FIN_HOST;
  r.type = u8(t);
  r.from = f.from;
  r.term = f.term;
  const u64 clen = f.has_ctx ? f.ctx_len : 0ull;
  switch (t) {
    case 8: {  // MsgHeartbeat
      u64 id = 0;
      if (clen == 8) id = wire::load_be64(s, f.ctx_pos);
      if (clen == 0 || (clen == 8 && id != 0)) {
        r.flags = QB_FIN_HEARTBEAT;
        r.index = f.commit;
        r.aux = id;
      } else {
        r.st = QB_WIRE_CTX;
      }
      break;
    }
    case 5:     // MsgVote
    case 17: {  // MsgPreVote
      bool force = false;
      if (clen == 16)
        force = load_le64(s, f.ctx_pos) == kXferLo && load_le64(s, f.ctx_pos + 8) == kXferHi;
      r.flags = u8((t == 5 ? QB_FIN_VOTE : QB_FIN_PREVOTE) | (force ? QB_FREC_FORCE : 0u));
      r.index = f.index;
      r.aux = f.log_term;
      break;
    }
    case 14:  // MsgTimeoutNow
      r.flags = QB_FIN_TIMEOUT_NOW;
      break;
    case 3: {  // MsgApp
      r.index = f.index;
      r.aux = f.log_term;
      r.commit = f.commit;
      r.en = sink.n;
      const bool bad = sink.bad || (sink.n != 0 && sink.first != f.index + 1);
      if (bad) {
        r.st = QB_WIRE_ENTRIES;
      } else {
        r.flags = QB_FIN_APP;
        r.runs = sink.runs;
        r.epos = sink.n ? sink.lo : 0ull;
        r.ebytes = sink.n ? u32(sink.hi - sink.lo) : 0u;
      }
      break;
    }
    default:
      r.st = QB_WIRE_TYPE;
      break;
  }
  return r;
}

// A message pass 1's first launch leaves to its second (the status between
// the two launches only; never returned).
constexpr u8 kDeferred = 0xFF;

// One record's columns.  Write-once, read by a later launch: nontemporal.
__device__ __forceinline__ void emit(const Args& A, u64 m, const Rec& r) {
  __builtin_nontemporal_store(r.group, A.rg + m);
  __builtin_nontemporal_store(r.flags, A.rf + m);
  __builtin_nontemporal_store(r.from, A.rfrom + m);
  __builtin_nontemporal_store(r.term, A.rterm + m);
  __builtin_nontemporal_store(r.index, A.rindex + m);
  __builtin_nontemporal_store(r.aux, A.raux + m);
  __builtin_nontemporal_store(r.commit, A.rcommit + m);
  __builtin_nontemporal_store(u8(r.st), A.status + m);
  if (A.mtype) __builtin_nontemporal_store(r.type, A.mtype + m);
  if (A.ent_n) __builtin_nontemporal_store(r.en, A.ent_n + m);
  A.ent_pos[m] = r.epos;  // pass 2 reads these two and the count
  A.ent_bytes[m] = r.ebytes;
  A.ent_off[m] = r.runs;
}

// The four final statuses pass 1 knows (OK and NO_SPACE are pass 2's).
__device__ __forceinline__ void tally_flush(const Args& A, u32* lds, u32 st_) {
  BlockTally<4> tally;
  tally.add(0, st_ == QB_WIRE_UNMARSHAL);
  tally.add(1, st_ == QB_WIRE_TYPE);
  tally.add(2, st_ == QB_WIRE_CTX);
  tally.add(3, st_ == QB_WIRE_ENTRIES);
  const int slot[4] = {QB_WIRE_UNMARSHAL, QB_WIRE_TYPE, QB_WIRE_CTX, QB_WIRE_ENTRIES};
  if (A.stats) tally.flush(lds, A.stats, slot);
}

// Pass 1, first launch.  Round trips per workgroup: the message offsets and
// groups, then the LDS-DMA stage of the byte span; the messages are parsed
// from LDS.  A message outside the staged span (a MsgApp with payloads: its
// block's span does not fit) is left to the second launch.
__global__ __launch_bounds__(kBlock) void k_follower_decode(Args A) {
  __shared__ __attribute__((aligned(16))) u8 stage[kStage + 48];  // + window over-reads (<= 24 B past a message)
  __shared__ u32 lds[4];
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
    // Pieces wholly inside the byte buffer go by LDS-DMA, all issued before
    // the barrier's one wait; only the buffer's last piece can be partial.
    // (A byte buffer that is not 16-byte aligned stages with plain loads;
    // offsets past the buffer — a caller error the decode reports as
    // UNMARSHAL — stage nothing from it.)
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
  u32 st_ = 0xFFu;
  if (m < A.M) {
    if (p0 >= lbase && p1 <= lend && p0 <= p1) {
      const Rec r = decode_follower(A.nbytes, LdsSrc{stage, lbase}, p0, p1, mg);
      st_ = r.st;
      emit(A, m, r);
    } else {
      A.status[m] = kDeferred;
    }
  }
  tally_flush(A, lds, st_);
}

// Pass 1, second launch: the messages the first left, each decoded from
// global memory through the 8-byte window (wire::WinSrc).  Split by byte
// source, not by canonical form: the generic loop sits in both launches, but
// the window's registers stay out of the LDS launch (with both sources in
// one kernel it took 114 VGPRs, 4 waves per SIMD).  With nothing left the
// launch reads the status column once.
__global__ __launch_bounds__(kBlock) void k_follower_decode_global(Args A) {
  __shared__ u32 lds[4];
  const u64 m = u64(blockIdx.x) * kBlock + threadIdx.x;
  u32 st_ = 0xFFu;
  if (m < A.M && A.status[m] == kDeferred) {
    const Rec r = decode_follower(A.nbytes, WinSrc(A.bytes, A.nbytes), A.moff[m], A.moff[m + 1],
                                  A.mgroup[m]);
    st_ = r.st;
    emit(A, m, r);
  }
  tally_flush(A, lds, st_);
}

// Pass 2: the runs of every MsgApp that has some, the NO_SPACE downgrade, the
// batch's run total and the OK / NO_SPACE counters.
__global__ __launch_bounds__(kBlock) void k_follower_runs(Args A) {
  __shared__ u32 lds[2];
  BlockTally<2> tally;
  const u64 m = u64(blockIdx.x) * kBlock + threadIdx.x;
  bool ok = false, nospace = false;
  if (m == 0) *A.ent_total = u64(A.ent_off[A.M]);
  if (m < A.M) {
    ok = A.status[m] == QB_WIRE_OK;
    const u32 o0 = A.ent_off[m], o1 = A.ent_off[m + 1];
    // (only an OK MsgApp has a non-empty range)
    if (ok && o1 > o0) {
      if (u64(o1) > A.ent_cap) {
        nospace = true;
        A.rf[m] = QB_FIN_HOST;
        A.status[m] = QB_WIRE_NO_SPACE;
      } else {
        const u64 pos = A.ent_pos[m];
        Fields f = Fields{};
        RunSink sink{0, 0, 0, 0, 0, A.ent_term, A.ent_len, o0, o1};
        // the range holds field-7 fields only, each validated by pass 1
        wire::unmarshal<K_MESSAGE>(WinSrc(A.bytes, A.nbytes), pos, pos + A.ent_bytes[m], &f, &sink);
        if (sink.n) sink.put();
      }
    }
  }
  tally.add(0, ok && !nospace);
  tally.add(1, nospace);
  const int slot[2] = {QB_WIRE_OK, QB_WIRE_NO_SPACE};
  if (A.stats) tally.flush(lds, A.stats, slot);
}

}  // namespace fwire
}  // namespace qb

using namespace qb;

namespace {
// Workspace: the run counts' scan block sums, and the entry ranges pass 2
// reads where the caller takes no ent_pos / ent_bytes columns.
struct Carve {
  size_t bsum, pos, len, total;
};
Carve carve(u64 M) {
  Carve c{};
  Carver k;
  c.bsum = k.take(sizeof(u32) * (scan::blocks(M) + 1));
  c.pos = k.take(sizeof(u64) * M);
  c.len = k.take(sizeof(u32) * M);
  c.total = k.o;
  return c;
}
// M + 1 offsets and the follower steps' M <= 2^32 - 2.
bool fits(u64 M) { return M <= 0xFFFFFFFEull; }
}  // namespace

extern "C" size_t qb_wire_follower_scratch_bytes(uint64_t M) { return fits(M) ? carve(M).total : 0; }

extern "C" int qb_dev_ingest_follower(uint64_t M, const uint8_t* bytes, uint64_t nbytes,
                                      const uint64_t* msg_off, const uint32_t* msg_group,
                                      uint64_t G, const qb_follower_wire_out* out, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  static const char* who = "qb_dev_ingest_follower";
  (void)G;  // groups >= G are passed through: the step's BAD_GROUP
  QB_REQUIRE(out, "%s: out is NULL", who);
  QB_REQUIRE(out->ent_off && out->ent_total, "%s: ent_off / ent_total is NULL", who);
  hipStream_t st = as_stream(stream);
  if (M == 0) {
    hipError_t e = hipMemsetAsync(out->ent_total, 0, sizeof(u64), st);
    if (e == hipSuccess) e = hipMemsetAsync(out->ent_off, 0, sizeof(u32), st);
    return e == hipSuccess ? QB_OK : hip_fail(e, "hipMemsetAsync(ent_total)");
  }
  QB_REQUIRE(msg_off && msg_group, "%s: msg_off / msg_group is NULL", who);
  QB_REQUIRE(nbytes == 0 || bytes, "%s: bytes is NULL", who);
  QB_REQUIRE(out->group && out->flags && out->from && out->term && out->index && out->aux &&
                 out->commit && out->status,
             "%s: group, flags, from, term, index, aux, commit and status are required", who);
  QB_REQUIRE(out->ent_cap == 0 || (out->ent_term && out->ent_len),
             "%s: ent_term / ent_len is NULL with ent_cap %llu", who,
             (unsigned long long)out->ent_cap);
  QB_REQUIRE(fits(M), "%s: %llu messages pass 2^32 - 2", who, (unsigned long long)M);
  QB_REQUIRE(nbytes < (1ull << 32),
             "%s: %llu bytes pass 2^32 (ent_bytes and the run counts' scan are 32-bit)", who,
             (unsigned long long)nbytes);
  const Carve cv = carve(M);
  QB_REQUIRE(workspace && workspace_bytes >= cv.total,
             "%s: workspace too small (qb_wire_follower_scratch_bytes)", who);
  char* ws = static_cast<char*>(workspace);
  fwire::Args A{M, nbytes, bytes, reinterpret_cast<const u64*>(msg_off), msg_group,
                out->group, out->flags, reinterpret_cast<u64*>(out->from),
                reinterpret_cast<u64*>(out->term), reinterpret_cast<u64*>(out->index),
                reinterpret_cast<u64*>(out->aux), reinterpret_cast<u64*>(out->commit),
                out->status, out->msg_type,
                out->ent_pos ? reinterpret_cast<u64*>(out->ent_pos) : reinterpret_cast<u64*>(ws + cv.pos),
                out->ent_bytes ? out->ent_bytes : reinterpret_cast<u32*>(ws + cv.len),
                out->ent_n, out->ent_off, reinterpret_cast<u64*>(out->ent_term), out->ent_len,
                out->ent_cap, reinterpret_cast<u64*>(out->ent_total),
                reinterpret_cast<u64*>(out->stats)};
  hipLaunchKernelGGL(fwire::k_follower_decode, dim3(grid_for(M)), dim3(kBlock), 0, st, A);
  QB_CHECK_LAUNCH("k_follower_decode");
  hipLaunchKernelGGL(fwire::k_follower_decode_global, dim3(grid_for(M)), dim3(kBlock), 0, st, A);
  QB_CHECK_LAUNCH("k_follower_decode_global");
  scan::launch(A.ent_off, M, reinterpret_cast<u32*>(ws + cv.bsum), st);
  QB_CHECK_LAUNCH("scan(follower wire)");
  hipLaunchKernelGGL(fwire::k_follower_runs, dim3(grid_for(M)), dim3(kBlock), 0, st, A);
  QB_CHECK_LAUNCH("k_follower_runs");
  return QB_OK;
}
