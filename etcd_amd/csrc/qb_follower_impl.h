// qb_follower_impl.h — raft.Step for the non-leader inbox of G groups at once
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
//
// qb_dev_follower_log_step is the same pipeline with one more record kind,
// QB_FIN_APP (pb.MsgApp): every kernel is a template on LOG, and LOG = false
// is qb_dev_follower_step as it was.  handleAppendEntries (raft.go:1475-1511)
// needs only the log's term index, which the caller keeps as a run table
// (run-major, up to QB_LEADER_MAX_RUNS runs, as qb_leader_groups).  The table
// stays in global memory and is walked a run at a time, only by a record that
// needs it: a MsgApp at Index == last_index with LogTerm == last_term whose
// entries carry last_term (steady replication) reads and writes none of it.
#pragma once
#include <type_traits>

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
// with LOG four more u32 counters (ENTRIES_APPENDED is summed as u64 apart)
constexpr int kLogStats = kStepStats + 4;
constexpr int kCAccepted = kStepStats, kCRejected = kStepStats + 1, kCBelow = kStepStats + 2,
              kCTruncated = kStepStats + 3;
template <bool LOG>
constexpr int kStats = LOG ? kLogStats : kStepStats;
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

// what qb_dev_follower_log_step passes beside Args
struct LogArgs : Args {
  qb_follower_log lg;
  qb_follower_app_inbox app;
  qb_follower_app_out out;
};
template <bool LOG>
using ArgsT = std::conditional_t<LOG, LogArgs, Args>;

// a record F4 / F5 step: in range and of a known kind
template <bool LOG>
__device__ __forceinline__ bool rec_ok(const Args& A, u64 i, u32& g, bool& badg, bool& badk) {
  g = A.in.group[i];
  const u32 kind = A.in.flags[i] & QB_FREC_KIND_MASK;
  badg = u64(g) >= A.fg.G;
  badk = !badg && kind > (LOG ? QB_FIN_APP : QB_FIN_HOST);
  return !badg && !badk;
}

template <bool LOG>
__global__ __launch_bounds__(kBlock) void k_count(ArgsT<LOG> A) {
  __shared__ u32 sh[2];
  const u64 i = u64(blockIdx.x) * kBlock + threadIdx.x;
  bool badg = false, badk = false;
  if (i < A.in.M) {
    u32 g;
    if (rec_ok<LOG>(A, i, g, badg, badk)) {
      atomicAdd(A.cnt + g, 1u);
    } else {
      A.resp_type[i] = 0;
      A.resp_term[i] = 0;
      if constexpr (LOG) {
        A.out.resp_index[i] = 0;
        A.out.app_from[i] = 0;
      }
    }
  }
  BlockTally<2> t;
  t.add(0, badg);
  t.add(1, badk);
  const int slot[2] = {QB_FSTAT_BAD_GROUP, QB_FSTAT_BAD_KIND};
  t.flush(sh, A.stats, slot);
}

template <bool LOG>
__global__ __launch_bounds__(kBlock) void k_scatter(ArgsT<LOG> A) {
  const u64 i = u64(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= A.in.M) return;
  u32 g;
  bool badg, badk;
  if (!rec_ok<LOG>(A, i, g, badg, badk)) return;
  const u32 pos = atomicAdd(A.cnt + g, 1u);
  if (u64(pos) < A.in.M) A.perm[pos] = u32(i);  // (always, for a batch that does not change under the call)
}

struct Rec {
  u64 from, term, index, aux;
  u8 fl;
};
// with LOG: Message.Commit, the record's entry runs [e0, e1) (clamped to E)
// and the first of them
struct LogRec : Rec {
  u64 commit, fterm;
  u32 e0, e1, flen;
};
template <bool LOG>
using RecT = std::conditional_t<LOG, LogRec, Rec>;

template <bool LOG>
__device__ __forceinline__ RecT<LOG> load_rec(const ArgsT<LOG>& A, u32 i) {
  const qb_follower_inbox& in = A.in;
  RecT<LOG> r;
  r.fl = in.flags[i];
  r.from = reinterpret_cast<const u64*>(in.from)[i];
  r.term = reinterpret_cast<const u64*>(in.term)[i];
  r.index = reinterpret_cast<const u64*>(in.index)[i];
  r.aux = reinterpret_cast<const u64*>(in.aux)[i];
  if constexpr (LOG) {
    const qb_follower_app_inbox& ap = A.app;
    const u32 E = ap.E < 0xFFFFFFFFull ? u32(ap.E) : 0xFFFFFFFFu;
    u32 e0 = ap.ent_off[i], e1 = ap.ent_off[u64(i) + 1];
    r.commit = reinterpret_cast<const u64*>(ap.commit)[i];
    e0 = e0 < E ? e0 : E;
    e1 = e1 < E ? e1 : E;
    r.e0 = e0;
    r.e1 = e1 > e0 ? e1 : e0;
    r.fterm = 0;
    r.flen = 0;
    if (e0 < e1) {  // the first run travels with the record
      r.fterm = reinterpret_cast<const u64*>(ap.ent_term)[e0];
      r.flen = ap.ent_len[e0];
    }
  }
  return r;
}

// ---- handleAppendEntries over the run table (LOG only) --------------------
enum : u8 { kAppBelow = 1, kAppAccept = 2, kAppReject = 3 };

// What one MsgApp does to the group, decided before anything is applied.
struct AppPlan {
  u64 ci;       // findConflict, 0 = the log keeps its entries
  u64 lastnew;  // Index + number of entries
  u64 com;      // committed behind the record
  u64 lt;       // last_term behind the record
  u64 kterm;    // term of the last run kept
  u64 hint, hterm;
  u32 keep, add;  // runs kept / appended (when table)
  u32 meta;
  u8 what, stop;  // kApp* / the QB_FFLAG_* of a stop
  bool table;     // the run table or its count changes
};

// run q of the message: (term, length)
__device__ __forceinline__ void ent_run(const LogArgs& A, const LogRec& r, u32 q, u64& et, u32& len) {
  if (q == r.e0) {
    et = r.fterm;
    len = r.flen;
  } else {
    et = reinterpret_cast<const u64*>(A.app.ent_term)[q];
    len = A.app.ent_len[q];
  }
}

// raft.go:1475-1511 -> raftLog.maybeAppend (log.go:88-107) for the record r
// of group g whose log ends at (li, lt) and is committed to com.  Reads the
// table only where the answer depends on it; writes nothing.
__device__ __forceinline__ void plan_app(const LogArgs& A, u64 g, const LogRec& r, u64 li, u64 lt,
                                         u64 com, AppPlan& p) {
  const u64 G = A.fg.G;
  const u64* rs = reinterpret_cast<const u64*>(A.lg.run_start) + g;  // run q at rs[q * G]
  const u64* rt = reinterpret_cast<const u64*>(A.lg.run_term) + g;
  p.ci = 0;
  p.stop = 0;
  p.table = false;
  p.com = com;
  p.lt = lt;
  p.lastnew = 0;
  if (r.index < com) {  // raft.go:1476-1479
    p.what = kAppBelow;
    return;
  }
  u64 dummy = 0;  // firstIndex - 1, the run count and meta: read on first use
  u32 nr = 0, meta = 0;
  bool have = false;
  auto table = [&] {
    if (!have) {
      dummy = reinterpret_cast<const u64*>(A.lg.first_index)[g] - 1;
      meta = A.lg.meta[g];
      nr = (meta >> 16) & 0xFu;
      nr = nr < 1 ? 1u : (nr > u32(QB_LEADER_MAX_RUNS) ? u32(QB_LEADER_MAX_RUNS) : nr);
      have = true;
    }
  };
  // raftLog.term (log.go:268-274): 0 outside [dummy, li]; end = the last
  // index of i's run (li outside)
  auto term_at = [&](u64 i, u64& end) -> u64 {
    table();
    end = li;
    if (i < dummy || i > li) return 0;
    u64 t = 0;
#pragma unroll 1
    for (u32 q = 0; q < nr; ++q) {
      const u64 s = rs[q * G];
      if (s > i) {
        end = s - 1;
        break;
      }
      t = rt[q * G];
    }
    return t;
  };
  u64 end;
  // matchTerm (log.go:320-326); the last entry's term is lt without the table
  const bool match = (r.index == li && r.aux == lt) || term_at(r.index, end) == r.aux;
  if (!match) {  // raft.go:1496-1509
    u64 idx = r.index < li ? r.index : li;
    table();
    // findConflictByTerm (log.go:150-171) a run at a time: a run whose term
    // is above LogTerm is skipped whole, down to the dummy entry
#pragma unroll 1
    for (u32 it = 0; it <= nr; ++it) {
      if (idx < dummy || idx > li) break;
      u64 t = 0, start = 0;
#pragma unroll 1
      for (u32 q = 0; q < nr; ++q) {
        const u64 s = rs[q * G];
        if (s <= idx) {
          t = rt[q * G];
          start = s;
        }
      }
      if (t <= r.aux) break;
      idx = (start > dummy ? start : dummy) - 1;  // wraps at 0 as the reference's index--
    }
    p.hint = idx;
    p.hterm = term_at(idx, end);
    p.what = kAppReject;
    return;
  }
  p.what = kAppAccept;
  // findConflict (log.go:130-141): the first entry whose term differs from
  // the log's, message run by message run against the log's runs
  u64 n = 0, ci = 0;
  bool found = false;
#pragma unroll 1
  for (u32 q = r.e0; q < r.e1; ++q) {
    u64 et;
    u32 len;
    ent_run(A, r, q, et, len);
    if (!len) continue;
    const u64 s = r.index + 1 + n;
    n += len;
    if (found) continue;
    const u64 e = s + (len - 1);
    u64 y = s;
#pragma unroll 1
    for (u32 it = 0; it <= u32(QB_LEADER_MAX_RUNS) + 1; ++it) {  // (a log run per round)
      if (y > li) {  // term() is 0 there: only a zero term "matches"
        if (et != 0) {
          found = true;
          ci = y;
        }
        break;
      }
      const u64 t = term_at(y, end);
      if (t != et) {
        found = true;
        ci = y;
        break;
      }
      if (end >= e) break;
      y = end + 1;
    }
  }
  p.lastnew = r.index + n;
  p.ci = ci;  // (a conflict at a wrapped index 0 reads as none, log.go:93)
  u64 newlast = li;
  if (ci != 0) {
    // log.go:94-95, and unstable.truncateAndAppend's bounds for a gap
    if (ci <= com || ci - 1 > li) {
      p.stop = QB_FFLAG_LOG_CONFLICT;
      return;
    }
    const bool trunc = ci - 1 < li;
    u32 keep = 0;
    u64 prev = lt;
    if (trunc) {  // runs starting at or after ci are dropped
      table();
#pragma unroll 1
      for (u32 q = 0; q < nr; ++q)
        if (rs[q * G] < ci) {
          keep = q + 1;
          prev = rt[q * G];
        }
      if (keep == 0) keep = 1;  // (run 0 holds the dummy entry)
    }
    p.kterm = prev;
    u32 add = 0;
    u64 m = 0;
#pragma unroll 1
    for (u32 q = r.e0; q < r.e1; ++q) {  // the message's runs from ci on, merged by term
      u64 et;
      u32 len;
      ent_run(A, r, q, et, len);
      if (!len) continue;
      const u64 e = r.index + m + len;
      m += len;
      if (e < ci) continue;
      if (et != prev) {
        ++add;
        prev = et;
      }
    }
    p.lt = prev;
    if (add || trunc) {
      table();
      if (!trunc) keep = nr;
      if (keep + add > u32(QB_LEADER_MAX_RUNS)) {
        p.stop = QB_FFLAG_LOG_RUNS;
        return;
      }
      p.table = true;
      p.keep = keep;
      p.add = add;
      p.meta = meta;
    }
    newlast = p.lastnew;
  }
  // commitTo(min(Commit, lastnewi)), log.go:103, 236-244
  const u64 toc = r.commit < p.lastnew ? r.commit : p.lastnew;
  if (com < toc) {
    if (newlast < toc) {
      p.stop = QB_FFLAG_COMMIT_RANGE;
      return;
    }
    p.com = toc;
  }
}

// The table's part of an accepted append (p.table): the message's runs from
// p.ci on behind the p.keep kept runs, and the run count in meta.
__device__ __forceinline__ void append_runs(const LogArgs& A, u64 g, const LogRec& r, const AppPlan& p) {
  const u64 G = A.fg.G;
  u64* rs = reinterpret_cast<u64*>(A.lg.run_start) + g;
  u64* rt = reinterpret_cast<u64*>(A.lg.run_term) + g;
  u32 w = p.keep;
  u64 prev = p.kterm, m = 0;
#pragma unroll 1
  for (u32 q = r.e0; q < r.e1; ++q) {
    u64 et;
    u32 len;
    ent_run(A, r, q, et, len);
    if (!len) continue;
    const u64 s = r.index + 1 + m, e = r.index + m + len;
    m += len;
    if (e < p.ci) continue;
    if (et != prev && w < u32(QB_LEADER_MAX_RUNS)) {  // (keep + add <= 8: always)
      rs[u64(w) * G] = s > p.ci ? s : p.ci;
      rt[u64(w) * G] = et;
      ++w;
      prev = et;
    }
  }
  if (w != ((p.meta >> 16) & 0xFu)) A.lg.meta[g] = (p.meta & ~0xF0000u) | (w << 16);
}

// Group g's run (n >= 1 batch indices, ascending) stepped in order.
// (ents: ENTRIES_APPENDED, LOG only.)
template <bool LOG>
__device__ __forceinline__ void step_group(const ArgsT<LOG>& A, u64 g, const u32* run, u32 n,
                                           u32 (&c)[kStats<LOG>], u64& ents) {
  const qb_follower_groups& fg = A.fg;
  u64* gterm = reinterpret_cast<u64*>(fg.term);
  u64* gvote = reinterpret_cast<u64*>(fg.vote);
  u64* glead = reinterpret_cast<u64*>(fg.lead);
  u64* gcom = reinterpret_cast<u64*>(fg.committed);
  // every word of the group and the first record in one round trip
  RecT<LOG> nx = load_rec<LOG>(A, run[0]);
  const u64 term0 = gterm[g], vote0 = gvote[g], lead0 = glead[g], com0 = gcom[g];
  const u64 li0 = reinterpret_cast<const u64*>(fg.last_index)[g];
  const u64 lt0 = reinterpret_cast<const u64*>(fg.last_term)[g];
  u64 li = li0, lt = lt0;  // (an append moves them: LOG only)
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
    const RecT<LOG> r = nx;
    if (k + 1 < n) nx = load_rec<LOG>(A, run[k + 1]);
    const u32 kind = r.fl & QB_FREC_KIND_MASK;
    const bool is_vote = kind == QB_FIN_VOTE || kind == QB_FIN_PREVOTE;
    const bool is_app = LOG && kind == QB_FIN_APP;
    u8 rt = 0;
    u64 rterm = 0;
    const bool higher = r.term != 0 && r.term > term;  // raft.go:850-852
    [[maybe_unused]] AppPlan p;
    [[maybe_unused]] u64 ridx = 0, afrom = 0;
    if constexpr (LOG) {
      p.what = 0;
      p.stop = 0;
      // a MsgApp that reaches handleAppendEntries: its stops are found before
      // the term filter's effect is applied (which does not touch the log)
      if (is_app && !(r.term != 0 && r.term < term) && (higher || (role & 3u) != QB_ROLE_LEADER))
        plan_app(A, g, r, li, lt, com, p);
    }
    if (kind == QB_FIN_HOST) {
      stop = i;
      gf |= QB_FFLAG_HOST_MSG;
    } else if (r.term != 0 && r.term < term) {  // raft.go:883-919
      if ((cq || pv) && (kind == QB_FIN_HEARTBEAT || is_app)) {
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
    } else if (is_app && p.stop) {
      stop = i;  // an append Go panics on, or one the table cannot hold: nothing is applied
      gf |= p.stop;
    } else {
      if (higher && kind != QB_FIN_PREVOTE)  // raft.go:864-881
        become_follower(r.term, kind == QB_FIN_HEARTBEAT || is_app ? r.from : 0ull);
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
      } else if (is_app) {
        if constexpr (LOG) {
          if ((role & 3u) == QB_ROLE_LEADER) {  // stepLeader has no case for it
            ++c[QB_FSTAT_ROLE_IGNORED];
          } else {
            if ((role & 3u) != QB_ROLE_FOLLOWER) {  // stepCandidate, raft.go:1390-1392
              become_follower(r.term, r.from);
            } else {  // stepFollower, raft.go:1433-1435
              ee = 0;
              lead = r.from;
            }
            rt = QB_FRESP_APP_RESP;  // handleAppendEntries, raft.go:1475-1511
            rterm = term;
            if (p.what == kAppBelow) {
              ridx = com;
              ++c[kCBelow];
            } else if (p.what == kAppReject) {
              rt |= QB_FRESP_REJECT;
              ridx = r.index;
              reinterpret_cast<u64*>(A.out.resp_hint)[i] = p.hint;
              reinterpret_cast<u64*>(A.out.resp_log_term)[i] = p.hterm;
              ++c[kCRejected];
            } else {
              if (p.ci != 0) {  // log.go:96-101
                if (p.table) append_runs(A, g, r, p);
                if (p.ci - 1 < li) ++c[kCTruncated];
                ents += p.lastnew - p.ci + 1;
                li = p.lastnew;
                lt = p.lt;
                afrom = p.ci;
                gf |= QB_FFLAG_APPENDED;
              }
              com = p.com;
              ridx = p.lastnew;
              ++c[kCAccepted];
            }
          }
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
    if constexpr (LOG) {
      reinterpret_cast<u64*>(A.out.resp_index)[i] = ridx;
      reinterpret_cast<u64*>(A.out.app_from)[i] = afrom;
    }
  }
  for (; k < n; ++k) {  // behind the stop: the host re-submits them
    const u32 i = run[k];
    A.resp_type[i] = 0;
    A.resp_term[i] = 0;
    if constexpr (LOG) {
      reinterpret_cast<u64*>(A.out.resp_index)[i] = 0;
      reinterpret_cast<u64*>(A.out.app_from)[i] = 0;
    }
    ++c[QB_FSTAT_AFTER_STOP];
  }
  if constexpr (LOG) {
    if (li != li0) reinterpret_cast<u64*>(A.lg.last_index)[g] = li;
    if (lt != lt0) reinterpret_cast<u64*>(A.lg.last_term)[g] = lt;
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
  for (int j = 0; j < K; ++j)  // (the log step's counters sit behind BAD_GROUP / BAD_KIND)
    slot[j] = j < kStepStats ? j : j == kCTruncated ? int(QB_FLSTAT_APP_TRUNCATED) : j + 2;
  t.flush(lds, stats, slot);
}

// ENTRIES_APPENDED: a u64 sum per wave, per workgroup in LDS, one atomic per
// workgroup.  Every thread of the block calls it.
__device__ __forceinline__ void flush_ents(u64 ents, u64* lds, u64* stats) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ents += u64(__shfl_xor(static_cast<unsigned long long>(ents), o, 64));
  if (threadIdx.x == 0) *lds = 0;
  __syncthreads();
  if ((threadIdx.x & 63) == 0 && ents) atomicAdd(reinterpret_cast<unsigned long long*>(lds), ents);
  __syncthreads();
  if (threadIdx.x == 0 && *lds)
    atomicAdd(reinterpret_cast<unsigned long long*>(stats + QB_FLSTAT_ENTRIES_APPENDED), *lds);
}

template <bool LOG>
__global__ __launch_bounds__(kBlock) void k_step(ArgsT<LOG> A) {
  __shared__ u32 sh[kStats<LOG>];
  const u64 G = A.fg.G;
  const u64 ntiles = (G + kBlock - 1) / kBlock;
  u32 c[kStats<LOG>];
  u64 ents = 0;
#pragma unroll
  for (int j = 0; j < kStats<LOG>; ++j) c[j] = 0;
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
      step_group<LOG>(A, g, run, n, c, ents);
    } else {
      const u32 s = atomicAdd(A.nlong, 1u);
      A.longs[s] = u32(g);  // (at most M / (kInline + 1) such groups)
    }
  }
  flush_counts(c, sh, A.stats);
  if constexpr (LOG) {
    __shared__ u64 she;
    flush_ents(ents, &she, A.stats);
  }
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

template <bool LOG>
__global__ __launch_bounds__(kBlock) void k_long(ArgsT<LOG> A) {
  __shared__ u32 run[kLdsRun];
  __shared__ u32 sh[kStats<LOG>];
  const u32 nl = *A.nlong;
  u32 c[kStats<LOG>];
  u64 ents = 0;
#pragma unroll
  for (int j = 0; j < kStats<LOG>; ++j) c[j] = 0;
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
      if (threadIdx.x == 0 && n) step_group<LOG>(A, g, run, n, c, ents);
    } else {
      // in the workspace: device-scope accesses, so no lane reads a line its
      // CU cached before another wave's store
      __syncthreads();
      block_bitonic(
          n, [&](u32 i) { return __hip_atomic_load(pg + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
          [&](u32 i, u32 v) { __hip_atomic_store(pg + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); });
      __threadfence();
      __syncthreads();
      if (threadIdx.x == 0) step_group<LOG>(A, g, pg, n, c, ents);
    }
    __syncthreads();  // the LDS run is free for the next group
  }
  flush_counts(c, sh, A.stats);
  if constexpr (LOG) {
    __shared__ u64 she;
    flush_ents(ents, &she, A.stats);
  }
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

inline void bind(Args& A, const qb_follower_groups* fg, const qb_follower_inbox* in, uint8_t* resp_type,
                 uint64_t* resp_term, uint32_t* stop_at, uint8_t* gflags, uint64_t* stats, char* ws,
                 const Carve& cv) {
  A.fg = *fg;
  A.in = *in;
  A.resp_type = resp_type;
  A.resp_term = reinterpret_cast<u64*>(resp_term);
  A.stop_at = stop_at;
  A.gflags = gflags;
  A.stats = reinterpret_cast<u64*>(stats);
  A.cnt = reinterpret_cast<u32*>(ws + cv.cnt);
  A.perm = reinterpret_cast<u32*>(ws + cv.perm);
  A.longs = reinterpret_cast<u32*>(ws + cv.longs);
  A.nlong = reinterpret_cast<u32*>(ws + cv.nlong);
}

// F1-F5 on the stream
template <bool LOG>
int launch(const ArgsT<LOG>& A, const Carve& cv, char* ws, hipStream_t st, const char* memset_what) {
  const u64 G = A.fg.G, M = A.in.M;
  hipError_t e = hipMemsetAsync(ws + cv.cnt, 0, cv.zero_end - cv.cnt, st);
  if (e != hipSuccess) return hip_fail(e, memset_what);
  if (M) {
    hipLaunchKernelGGL(k_count<LOG>, dim3(grid_for(M)), dim3(kBlock), 0, st, A);
    QB_CHECK_LAUNCH("k_count");
    scan::launch(A.cnt, G, reinterpret_cast<u32*>(ws + cv.bsum), st);
    QB_CHECK_LAUNCH("follower scan");
    hipLaunchKernelGGL(k_scatter<LOG>, dim3(grid_for(M)), dim3(kBlock), 0, st, A);
    QB_CHECK_LAUNCH("k_scatter");
  }
  const unsigned tiles = grid_for(G);
  hipLaunchKernelGGL(k_step<LOG>, dim3(tiles < kStepBlocks ? tiles : kStepBlocks), dim3(kBlock), 0, st,
                     A);
  QB_CHECK_LAUNCH("k_step");
  if (M > kInline) {
    const u64 most = M / (kInline + 1);  // groups that can hold a long run
    hipLaunchKernelGGL(k_long<LOG>, dim3(unsigned(most < kLongBlocks ? most : kLongBlocks)),
                       dim3(kBlock), 0, st, A);
    QB_CHECK_LAUNCH("k_long");
  }
  return QB_OK;
}

}  // namespace fol
}  // namespace qb
