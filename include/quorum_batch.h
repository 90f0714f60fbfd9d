/*
 * quorum_batch.h — C ABI of libquorumbatch, the MI355X batched quorum engine.
 *
 * This is the drop-in boundary for etcd's raft quorum/tracker hot path
 * evaluated over G independent raft groups at once.  It is the ABI a
 * ``raft/quorum/batch`` cgo package binds; every entry
 * point names the reference interface it replaces (paths relative to the
 * reference's ``raft/``).  Plain C types only: no torch, no HIP types.
 *
 * Conventions (mirroring the reference):
 *   - Every call returns int: QB_OK (0) or a negative QB_E* code; the text of
 *     the most recent failure on the calling thread is qb_last_error().
 *   - Quorum semantics never error: an empty majority config yields
 *     QB_INDEX_INF (MaxUint64) and VoteWon, exactly as majority.go:128-133 and
 *     majority.go:179-184.  Only malformed inputs (bad sizes, null required
 *     pointers, HIP failures) produce an error code.
 *   - Indexes are quorum.Index (uint64, unsigned compare over the full range);
 *     vote results are quorum.VoteResult: 1 Pending, 2 Lost, 3 Won
 *     (quorum.go:45-58).
 *   - "qb_dev_*" calls take DEVICE pointers and a hipStream_t passed as
 *     void* (NULL = the null stream); they only enqueue work.  Ownership stays
 *     with the caller.  One stream per host thread; no internal locking
 *     (single owner, like raft's RawNode, rawnode.go:31).
 *
 * Device layouts (structure of arrays, all little-endian):
 *
 *   FIXED  (every group is one n-voter MajorityConfig, 1 <= n <= 16, no
 *           learners; slot j = the j-th smallest voter ID, MajorityConfig.Slice
 *           majority.go:106-113):
 *     match[n][G]   uint64, slot-major: match[j*G + g] = Progress.Match
 *     voted[G], granted[G]   bitmask per group, bit j = slot j; uint8 when
 *                   n <= 8, uint16 when n > 8.  granted bits count only where
 *                   the voted bit is set (votes map: present -> voted).
 *
 *   CSR    (ragged: voters + learners, joint configs; 0 <= s_g <= 16 slots;
 *           s_g == 0 is the empty config):
 *     off[G+1]      uint32, slots of group g are off[g] .. off[g+1]-1
 *     match[off[G]] uint64, group-major
 *     cfg[G]        uint32 = mask_in | mask_out << 16  (JointConfig halves
 *                   Voters[0] / Voters[1], tracker.go:27-78; a slot with
 *                   neither bit is a learner; mask_out == 0 is a plain
 *                   majority config — identical results by joint.go:49-56)
 *     votes[G]      uint32 = voted | granted << 16
 *     active[G]     uint16 RecentActive bits (tracker.go:215-225)
 *
 *   WIDE   (configs with more than 16 slots, up to QB_WIDE_MAX_SLOTS; one
 *           wavefront per group):
 *     off[G+1]      uint32, match[off[G]] uint64 as CSR
 *     flags[off[G]] uint8 per slot: bit 0 incoming voter, bit 1 outgoing
 *                   voter, bit 2 voted, bit 3 granted
 *
 *   MsgAppResp batch records (M records, any order):
 *     rec_group[M]  uint32 group index within the shard
 *     rec_flags[M]  uint8: bits 0-3 = slot, bit 7 = Reject
 *     rec_index[M]  uint64 Message.Index
 *     rec_term[M]   uint64 Message.Term
 */
#ifndef QUORUM_BATCH_H
#define QUORUM_BATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QB_ABI_VERSION 1

#define QB_OK 0
#define QB_EINVAL (-1)   /* malformed arguments */
#define QB_EHIP (-2)     /* HIP runtime error (text in qb_last_error) */
#define QB_ENOMEM (-3)   /* device allocation failed */

#define QB_INDEX_INF UINT64_MAX  /* quorum.Index "∞", quorum.go:25-30 */

#define QB_VOTE_PENDING 1  /* quorum.VotePending, quorum.go:53 */
#define QB_VOTE_LOST 2     /* quorum.VoteLost,    quorum.go:55 */
#define QB_VOTE_WON 3      /* quorum.VoteWon,     quorum.go:57 */

#define QB_MAX_SLOTS 16
#define QB_WIDE_MAX_SLOTS 1024
#define QB_REC_REJECT 0x80u
#define QB_REC_NO_PROGRESS 0x40u /* leader inbox: From has no Progress (wire ingest) */

/* Counters filled by qb_dev_fixed_apply_appresp (device memory, uint64 each;
 * accumulated, so zero them before a batch if per-batch numbers are wanted). */
enum {
  QB_STAT_APPLIED = 0,     /* non-reject, same-term, member: MaybeUpdate ran   */
  QB_STAT_REJECTED = 1,    /* Reject=true: RecentActive only (raft.go:1107-1109) */
  QB_STAT_STALE_TERM = 2,  /* m.Term < group term: dropped (raft.go:883-921)    */
  QB_STAT_NON_MEMBER = 3,  /* no Progress for the slot: dropped (raft.go:1100) */
  QB_STAT_HIGHER_TERM = 4, /* m.Term > group term: leader steps down (raft.go:852-880) */
  QB_STAT_BAD_GROUP = 5,   /* group index >= G: dropped                        */
  QB_STAT_AFTER_STEPDOWN = 6, /* same-term record behind a higher-term one     */
  QB_STAT_COUNT = 8
};

/* Counters filled by qb_dev_record_votes (device uint64 each, accumulated). */
enum {
  QB_VSTAT_RECORDED = 0,       /* RecordVote stored the slot's first vote        */
  QB_VSTAT_DUPLICATE = 1,      /* the slot had already voted (first vote wins)   */
  QB_VSTAT_STALE_TERM = 2,     /* m.Term < group term: dropped                   */
  QB_VSTAT_HIGHER_TERM = 3,    /* the candidate steps down (raft.go:872-879)     */
  QB_VSTAT_AFTER_STEPDOWN = 4, /* any record behind the group's step-down        */
  QB_VSTAT_BAD = 5,            /* group index >= G                               */
  QB_VSTAT_AFTER_DECISION = 6, /* behind the group's VoteWon / VoteLost          */
  QB_VSTAT_COUNT = 8
};

#define QB_VOTE_MODE_VOTE 0     /* MsgVoteResp to a candidate (raft.go:1391) */
#define QB_VOTE_MODE_PREVOTE 1  /* MsgPreVoteResp to a pre-candidate         */

/* ----------------------------------------------------------------------- */
/* Library                                                                 */
/* ----------------------------------------------------------------------- */

int qb_abi_version(void);
/* Text of the last error on this thread ("" if none). */
const char* qb_last_error(void);
/* Number of visible HIP devices (0 without a GPU); never fails. */
int qb_device_count(void);

/* Device memory and streams for callers without their own HIP runtime
 * bindings (the Go cgo package).  Thin wrappers over hipMalloc / hipFree /
 * hipMemcpyAsync / hipStreamCreate; *_async copies are ordered on the stream
 * and the host buffer must stay alive until qb_stream_sync returns. */
int qb_set_device(int device);
int qb_malloc(size_t bytes, void** out);
int qb_free(void* ptr);
int qb_memset_async(void* dst, int value, size_t bytes, void* stream);
int qb_copy_h2d_async(void* dst, const void* src, size_t bytes, void* stream);
int qb_copy_d2h_async(void* dst, const void* src, size_t bytes, void* stream);
int qb_stream_create(void** out);
int qb_stream_destroy(void* stream);
int qb_stream_sync(void* stream);

/* ----------------------------------------------------------------------- */
/* Config compile (host)                                                   */
/* ----------------------------------------------------------------------- */

/* tracker.Config per group (tracker/tracker.go:27-78) -> the CSR layout:
 * slots = the sorted union of Voters[0], Voters[1] and Learners (the order of
 * MajorityConfig.Slice, quorum/majority.go:106-113; LearnersNext members are
 * outgoing voters until LeaveJoint, so they are in Voters[1]); cfg[g] =
 * mask_in | mask_out << 16 over those slots; a learner is in neither mask.
 * Each input is a CSR of IDs: group g's Voters[0] are in_ids[in_off[g] ..
 * in_off[g+1]) (out_off/out_ids, lrn_off/lrn_ids nullable = empty sets);
 * duplicate IDs within a list are one member.  Writes off[G+1], cfg[G] and,
 * if slot_ids is non-NULL, the slot IDs (slot_cap entries available; call
 * once with slot_ids NULL to size it: off[G] = slots needed).  A group whose
 * learners intersect its voters (confchange.go:307-318: "%d is in Learners
 * and Voters[1]" / "[0]") or with more than QB_MAX_SLOTS members fails the
 * call with QB_EINVAL, *bad_group (nullable) = the first such group and the
 * reference's message in qb_last_error().  Host memory only; no device. */
int qb_host_compile_configs(uint64_t G, const uint32_t* in_off, const uint64_t* in_ids,
                            const uint32_t* out_off, const uint64_t* out_ids,
                            const uint32_t* lrn_off, const uint64_t* lrn_ids,
                            uint32_t* off, uint32_t* cfg, uint64_t* slot_ids,
                            uint64_t slot_cap, uint64_t* bad_group);

/* ----------------------------------------------------------------------- */
/* Quorum math (raft/quorum)                                               */
/* ----------------------------------------------------------------------- */

/* CommittedIndex and/or VoteResult for G groups of one n-voter
 * MajorityConfig shape (FIXED layout).
 * Replaces MajorityConfig.CommittedIndex (quorum/majority.go:126-172) and
 * MajorityConfig.VoteResult (quorum/majority.go:178-210).
 * n == 0 fills commit_out with QB_INDEX_INF and vote_out with VoteWon.
 * commit_out and/or vote_out may be NULL to skip that result; voted/granted
 * may be NULL only when vote_out is NULL. */
int qb_dev_fixed_committed_vote(uint32_t n, uint64_t G, const uint64_t* match,
                                const void* voted, const void* granted,
                                uint64_t* commit_out, uint8_t* vote_out,
                                void* stream);

/* Several FIXED batches of one shape in one call (one cgo call per tick for
 * an embedder holding several shards' batches, instead of one per batch):
 * batch i is qb_dev_fixed_committed_vote(n, G, batches[i]...) enqueued on
 * streams[i % nstreams] (nstreams >= 1; a NULL entry is the default stream),
 * in order; stops at the first failing batch and returns its code. */
typedef struct qb_fixed_batch {
  const uint64_t* match;  /* [n][G] */
  const void* voted;      /* [G] u8 (n <= 8) or u16 */
  const void* granted;
  uint64_t* commit_out;   /* [G] or NULL */
  uint8_t* vote_out;      /* [G] or NULL */
} qb_fixed_batch;
int qb_dev_fixed_committed_vote_batches(uint32_t n, uint64_t G, uint32_t count,
                                        const qb_fixed_batch* batches, void* const* streams,
                                        uint32_t nstreams);

/* CommittedIndex and/or VoteResult for G ragged/joint groups (CSR layout).
 * Replaces JointConfig.CommittedIndex (quorum/joint.go:49-56) and
 * JointConfig.VoteResult (quorum/joint.go:61-75), which reduce to the
 * MajorityConfig forms when mask_out == 0; learners are slots in neither mask
 * and never count (tracker.go:273, majority.go:186-200).
 * max_slots bounds every s_g of the table (0 = QB_MAX_SLOTS); it sizes the
 * kernel (LDS and networks), so pass the table's true bound: a group above it
 * gives an unspecified (never out-of-bounds) result, which
 * qb_dev_csr_validate detects (qb_dev_csr_committed_vote_checked: validate,
 * then QB_EINVAL instead of a result). */
int qb_dev_csr_committed_vote(uint64_t G, uint32_t max_slots,
                              const uint32_t* off, const uint64_t* match,
                              const uint32_t* cfg, const uint32_t* votes,
                              uint64_t* commit_out, uint8_t* vote_out,
                              void* stream);

/* Checks a CSR table: off[0] == 0 and 0 <= off[g+1] - off[g] <= max_slots
 * (0 = QB_MAX_SLOTS).  Writes the number of bad groups to *bad_out (device
 * uint64). */
int qb_dev_csr_validate(uint64_t G, uint32_t max_slots, const uint32_t* off,
                        uint64_t* bad_out, void* stream);

/* qb_dev_csr_committed_vote behind an opt-in validation: the table is checked
 * first (qb_dev_csr_validate into bad_scratch, one device uint64) and a table
 * breaking its bound returns QB_EINVAL — with the count in qb_last_error() —
 * and computes nothing.  It reads the verdict back, so it synchronises the
 * stream: a debug / once-per-config-change form, not the per-tick call. */
int qb_dev_csr_committed_vote_checked(uint64_t G, uint32_t max_slots,
                                      const uint32_t* off, const uint64_t* match,
                                      const uint32_t* cfg, const uint32_t* votes,
                                      uint64_t* commit_out, uint8_t* vote_out,
                                      uint64_t* bad_scratch, void* stream);

/* CommittedIndex and/or VoteResult for G WIDE groups (JointConfig
 * semantics as qb_dev_csr_committed_vote, quorum/joint.go:49-75 over
 * quorum/majority.go:126-210).  max_slots bounds every s_g (0 =
 * QB_WIDE_MAX_SLOTS) and sizes the per-lane register tile. */
int qb_dev_wide_committed_vote(uint64_t G, uint32_t max_slots,
                               const uint32_t* off, const uint64_t* match,
                               const uint8_t* flags, uint64_t* commit_out,
                               uint8_t* vote_out, void* stream);
int qb_dev_wide_validate(uint64_t G, uint32_t max_slots, const uint32_t* off,
                         uint64_t* bad_out, void* stream);

/* ----------------------------------------------------------------------- */
/* Progress tracking (raft/tracker)                                        */
/* ----------------------------------------------------------------------- */

/* ProgressTracker.QuorumActive (tracker/tracker.go:215-225) per group:
 * won_out[g] = 1 iff VoteResult(votes = RecentActive of every voter) is
 * VoteWon in both halves. */
int qb_dev_csr_quorum_active(uint64_t G, const uint32_t* cfg,
                             const uint16_t* active, uint8_t* won_out,
                             void* stream);

/* Apply a batch of MsgAppResp records to FIXED-layout leader state — the
 * quorum-facing part of stepLeader's MsgAppResp case (raft.go:1100-1109,
 * 1237-1239): Progress.MaybeUpdate (tracker/progress.go:144-153) as an
 * atomic scatter-max of match (and next, if non-NULL), RecentActive bits,
 * and the term filter of raft.Step (raft.go:847-921).  Batch-equivalent to
 * applying the records one by one in index order.
 *   group_term[G]   the leader's current term per group
 *   match[n][G], next[n][G] (nullable), active[G] (uint16 bits; the array
 *                   must be 4-byte aligned and padded to an even length)
 *   stepdown_at[G]  uint32 output, written for every group (no entry
 *                   requirement): the batch index of the first higher-term
 *                   record of a group that must step down (raft.go:875-879),
 *                   UINT32_MAX otherwise.  Records after it are not applied,
 *                   as in the sequential reference.
 *   stats[QB_STAT_COUNT] device uint64 counters (required; zero them per
 *                   batch — a non-zero HIGHER_TERM count only makes the
 *                   apply pass consult stepdown_at, it never changes results). */
int qb_dev_fixed_apply_appresp(uint32_t n, uint64_t G, uint64_t M,
                               const uint32_t* rec_group,
                               const uint8_t* rec_flags,
                               const uint64_t* rec_index,
                               const uint64_t* rec_term,
                               const uint64_t* group_term, uint64_t* match,
                               uint64_t* next, uint16_t* active,
                               uint32_t* stepdown_at, uint64_t* stats,
                               void* stream);

/* raft.maybeCommit (raft.go:585-588) -> raftLog.maybeCommit (log.go:328-334)
 * for every group of the FIXED layout: committed[g] = CI if CI > committed[g]
 * and term(CI) == Term, where term(CI) == Term <=> CI >= term_start[g]
 * (term_start = first index of the leader's current term, QB_INDEX_INF if the
 * leader has none; CI <= lastIndex holds because no voter acks past the
 * leader's log).  advanced_out[g] (nullable) = 1 where the commit moved
 * (maybeCommit's return value). */
int qb_dev_fixed_commit_advance(uint32_t n, uint64_t G, const uint64_t* match,
                                const uint64_t* term_start,
                                uint64_t* committed, uint8_t* advanced_out,
                                void* stream);

/* One leader tick for G groups of the FIXED layout: a batch of MsgAppResp
 * records applied (same semantics as qb_dev_fixed_apply_appresp) and
 * maybeCommit run for every group (as qb_dev_fixed_commit_advance), fused.
 * The records are bucketed by group on the device (counting sort into
 * LDS-sized chunks) so every MaybeUpdate is an LDS atomic; this is the path
 * for large batches (M ~ G).  Differences from the two-call form:
 *   - stepdown_at[g] must hold UINT32_MAX on entry (the two-call form
 *     initialises it itself) and is written only where it can change: for
 *     every group of a chunk (256-512 consecutive groups) holding a
 *     higher-term record it is reset to UINT32_MAX and then receives the
 *     step-down record's batch index; every other entry is left untouched
 *     (no per-group write in the steady state).  A caller re-arming a group
 *     that stepped down resets its entry; stats[QB_STAT_HIGHER_TERM] > 0 says
 *     whether any group stepped down;
 *   - workspace: device scratch of qb_fixed_tracker_workspace_bytes(n, G, M)
 *     bytes (caller-owned, reusable across calls of the same or smaller
 *     size; no allocation inside, so the call can be graph-captured).
 * Requires G, M < 2^32, and a batch whose reserved regions (about 2 x M
 * records) stay below 2^32 records: qb_fixed_tracker_workspace_bytes
 * returns 0 for a larger one and the step QB_EINVAL.
 * qb_dev_stepdown_check_armed is the opt-in check of that entry rule (for a
 * caller's debug builds): it counts the entries != UINT32_MAX on the device,
 * synchronises the stream and returns QB_EINVAL naming the count if any
 * (bad_scratch: one device uint64). */
int qb_dev_stepdown_check_armed(uint64_t G, const uint32_t* stepdown_at,
                                uint64_t* bad_scratch, void* stream);
size_t qb_fixed_tracker_workspace_bytes(uint32_t n, uint64_t G, uint64_t M);
int qb_dev_fixed_tracker_step(uint32_t n, uint64_t G, uint64_t M,
                              const uint32_t* rec_group,
                              const uint8_t* rec_flags,
                              const uint64_t* rec_index,
                              const uint64_t* rec_term,
                              const uint64_t* group_term,
                              const uint64_t* term_start, uint64_t* match,
                              uint64_t* next, uint16_t* active,
                              uint64_t* committed, uint32_t* stepdown_at,
                              uint8_t* advanced_out, uint64_t* stats,
                              void* workspace, size_t workspace_bytes,
                              void* stream);

/* qb_dev_fixed_tracker_step in two halves, for a caller that pipelines
 * ticks: _bucket sorts a batch by group into a workspace (reads only the
 * batch: K3-K4, no leader state — so, unlike the step, it does not fold a
 * hot group's repeated records, which needs the group terms), _apply
 * applies that workspace's batch to
 * the state (K5 + the exact slow path; the same batch pointers, which the
 * slow path re-reads).  step == bucket then apply on one stream.  With two
 * workspaces on two streams, tick k+1's bucketing can run while tick k is
 * applied: the caller orders apply(k+1) after bucket(k+1) and apply(k), and
 * bucket(k+2) after apply(k) (workspace reuse).  Each workspace carries its
 * own statistic shards, folded into `stats` by _apply.  (On one MI355X the
 * overlap measured slower than back-to-back steps, 706-712 vs 672-674 us per
 * 16M-group tick: the concurrent kernels contend for the CUs and HBM; the
 * split is for callers that interleave other work between the halves.) */
int qb_dev_fixed_tracker_bucket(uint32_t n, uint64_t G, uint64_t M,
                                const uint32_t* rec_group,
                                const uint8_t* rec_flags,
                                const uint64_t* rec_index,
                                const uint64_t* rec_term,
                                void* workspace, size_t workspace_bytes,
                                void* stream);
int qb_dev_fixed_tracker_apply(uint32_t n, uint64_t G, uint64_t M,
                               const uint32_t* rec_group,
                               const uint8_t* rec_flags,
                               const uint64_t* rec_index,
                               const uint64_t* rec_term,
                               const uint64_t* group_term,
                               const uint64_t* term_start, uint64_t* match,
                               uint64_t* next, uint16_t* active,
                               uint64_t* committed, uint32_t* stepdown_at,
                               uint8_t* advanced_out, uint64_t* stats,
                               void* workspace, size_t workspace_bytes,
                               void* stream);

/* The same leader tick over G groups of the CSR layout (ragged voter
 * counts, learners, joint configs): a MsgAppResp batch applied (MaybeUpdate on
 * the slot's Progress, learners included; a slot >= s_g has no Progress and
 * is dropped before the term filter, node.go:356-360) and maybeCommit for
 * every group with ProgressTracker.Committed = JointConfig.CommittedIndex
 * over the voters of both halves (tracker/tracker.go:162-179,
 * quorum/joint.go:49-56) — the commit advance a joint transition runs on
 * every ack (raft.go:1259, 1682).  An empty config (both masks 0) never
 * commits: its CommittedIndex is MaxUint64, past lastIndex, whose term is 0
 * (log.go:271-273, 328-334).
 *   off[G+1], cfg[G]   CSR config as qb_dev_csr_committed_vote; max_slots
 *                      bounds every s_g (0 = QB_MAX_SLOTS) and sizes the
 *                      kernel (a chunk whose slot run breaks the bound is
 *                      applied by the exact slow path);
 *   match[off[G]], next[off[G]] (nullable)  Progress per slot;
 *   group_term, term_start, active, committed, stepdown_at, advanced_out,
 *   stats, workspace: as qb_dev_fixed_tracker_step (same stepdown_at rule). */
size_t qb_csr_tracker_workspace_bytes(uint64_t G, uint32_t max_slots, uint64_t M);
int qb_dev_csr_tracker_step(uint64_t G, uint32_t max_slots, const uint32_t* off,
                            const uint32_t* cfg, uint64_t M,
                            const uint32_t* rec_group, const uint8_t* rec_flags,
                            const uint64_t* rec_index, const uint64_t* rec_term,
                            const uint64_t* group_term,
                            const uint64_t* term_start, uint64_t* match,
                            uint64_t* next, uint16_t* active,
                            uint64_t* committed, uint32_t* stepdown_at,
                            uint8_t* advanced_out, uint64_t* stats,
                            void* workspace, size_t workspace_bytes,
                            void* stream);

/* Elections.  A batch of vote responses of one kind (mode), records
 * {group, flags = slot | reject << 7, term} in batch order, applied to the
 * CSR votes words (voted | granted << 16) exactly as the sequential
 * (pre-)candidate does: raft.Step's term filter (raft.go:847-921, with the
 * MsgPreVoteResp exception of raft.go:866-871), stepCandidate -> poll ->
 * RecordVote with first-vote-wins (tracker/tracker.go:258-263) and
 * TallyVotes against cfg (mask_in | mask_out << 16, learners in neither).
 * At the first response after which the result is VoteWon / VoteLost the
 * node changes state (raft.go:1402-1414) and polls nothing more:
 *   decided_at[g]  batch index of that response (UINT32_MAX: still pending);
 *                  votes[g] is left as it stood there, so
 *                  qb_dev_csr_tally_votes gives the decision;
 *   stepdown_at[g] batch index of the response that makes the node
 *                  becomeFollower at a higher term (UINT32_MAX: none): before
 *                  the decision any response above the group term (a granted
 *                  MsgPreVoteResp excepted); after a pre-candidate's VoteWon
 *                  the node campaigned at term + 1 (raft.go:1403 ->
 *                  becomeCandidate), so only a rejection above term + 1; after
 *                  a candidate's VoteWon / any VoteLost, a response above the
 *                  group term.  Nothing after the step-down is applied.
 * Both outputs are written for every group (no entry requirement).  The
 * state change itself (campaign with ResetVotes, becomeLeader, becomeFollower)
 * is qb_dev_campaign's (QB_CAMP_WON / QB_CAMP_LOST), the step-down at a higher
 * term the host's.  workspace: qb_votes_workspace_bytes(M) bytes of device
 * scratch. */
size_t qb_votes_workspace_bytes(uint64_t M);
int qb_dev_record_votes(int mode, uint64_t G, uint64_t M,
                        const uint32_t* rec_group, const uint8_t* rec_flags,
                        const uint64_t* rec_term, const uint64_t* group_term,
                        const uint32_t* cfg, uint32_t* votes, uint32_t* stepdown_at,
                        uint32_t* decided_at, uint64_t* stats,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ProgressTracker.TallyVotes (tracker/tracker.go:267-288) per group:
 * granted / rejected among the voters of either half (learners never count)
 * and JointConfig.VoteResult.  Any output may be NULL. */
int qb_dev_csr_tally_votes(uint64_t G, const uint32_t* cfg,
                           const uint32_t* votes, uint8_t* granted_out,
                           uint8_t* rejected_out, uint8_t* result_out,
                           void* stream);

/* ----------------------------------------------------------------------- */
/* Leader inbox step                              */
/* ----------------------------------------------------------------------- */

/* The full leader side of the responses in a raft leader's inbox, for G
 * groups at once, with the reference's sequential per-message semantics:
 *   raft.Step term filter (raft.go:847-921), stepLeader (raft.go:1099-1342):
 *   MsgAppResp reject -> findConflictByTerm (log.go:150-171) + MaybeDecrTo
 *     (progress.go:163-191) + BecomeProbe + sendAppend;
 *   MsgAppResp accept -> MaybeUpdate, Probe->Replicate, Snapshot recovery,
 *     Inflights.FreeLE, maybeCommit (raft.go:585-588) + bcastAppend
 *     (raft.go:515-522) or the paused-peer sendAppend, the maybeSendAppend
 *     loop (raft.go:432-492), MsgTimeoutNow to the lead transferee;
 *   MsgHeartbeatResp -> RecentActive, ProbeSent, FreeFirstOne, sendAppend,
 *     ReadIndex acks: readOnly.recvAck + VoteResult + advance
 *     (read_only.go:68-121) + responseToReadIndexReq (raft.go:1737-1752);
 *   MsgSnapStatus, MsgUnreachable (raft.go:1310-1338).
 * Records of a group are applied in batch order; groups are independent.
 * The leader's log is a static view (this step never appends; the log grows
 * in qb_dev_leader_propose): firstIndex,
 * lastIndex, the terms of [firstIndex-1, lastIndex] as up to
 * QB_LEADER_MAX_RUNS runs, the storage snapshot, and max_ents = the number
 * of entries raftLog.entries(lo, MaxSizePerMsg) returns (entries of one size).
 * Outbound messages are written in group order, each group's in the order
 * the reference emits them. */

#define QB_LEADER_MAX_RUNS 8
#define QB_LEADER_MAX_READQ 16

/* Inbound kinds (rec flags bits 4-5). */
#define QB_IN_APP_RESP 0       /* pb.MsgAppResp                         */
#define QB_IN_HEARTBEAT_RESP 1 /* pb.MsgHeartbeatResp (index = Context) */
#define QB_IN_SNAP_STATUS 2    /* pb.MsgSnapStatus (local, Term 0)      */
#define QB_IN_UNREACHABLE 3    /* pb.MsgUnreachable (local, Term 0)     */

/* Progress state byte: StateType (tracker/state.go:26-33) | flags. */
#define QB_PR_PROBE 0
#define QB_PR_REPLICATE 1
#define QB_PR_SNAPSHOT 2
#define QB_PR_PROBE_SENT 0x04u
#define QB_PR_RECENT_ACTIVE 0x08u

/* Group meta word: leader slot (bits 0-7), lead transferee slot (8-15,
 * 0xFF = None), term runs (16-19, 1..8), pending ReadIndex requests (20-24,
 * at most readq_cap), bit 25: MsgReadIndex postponed until the first commit
 * of the term (raft.pendingReadIndexMessages).  A run count past
 * QB_LEADER_MAX_RUNS or a request count past readq_cap is read as that bound
 * (the step never reads or writes outside the caller's arrays). */
#define QB_META_PENDING_READINDEX (1u << 25)

/* Diagnostic switch: group the records with per-record global atomics (the
 * path used beyond the bucket geometry, > 134M groups per shard) even where
 * the LDS bucketing applies; results are identical, only slower. */
#define QB_LEADER_OPT_ATOMIC_GROUPING 1u

#define QB_READ_ONLY_SAFE 0
#define QB_READ_ONLY_LEASE_BASED 1

/* Outbound message types (raftpb MessageType, raft.pb.go:76-94) and a local
 * ReadState (raft.readStates). */
#define QB_MSG_APP 3
#define QB_MSG_SNAP 7
#define QB_MSG_TIMEOUT_NOW 14
#define QB_MSG_READ_INDEX_RESP 16
#define QB_READ_STATE 255

/* Per-group output flags. */
#define QB_LFLAG_ADVANCED 0x01u     /* maybeCommit returned true          */
#define QB_LFLAG_RELEASE_READS 0x02u /* postponed MsgReadIndex to release  */
#define QB_LFLAG_STEPPED_DOWN 0x04u  /* a higher-term response: becomeFollower */

enum {
  QB_LSTAT_APPLIED = 0,        /* reached stepLeader's handler             */
  QB_LSTAT_STALE_TERM = 1,     /* m.Term < group term: ignored            */
  QB_LSTAT_HIGHER_TERM = 2,    /* step-down record                         */
  QB_LSTAT_NON_MEMBER = 3,     /* no Progress for the slot                 */
  QB_LSTAT_AFTER_STEPDOWN = 4, /* behind the group's step-down             */
  QB_LSTAT_BAD_GROUP = 5,      /* group index >= G                          */
  QB_LSTAT_MSGS = 6,           /* outbound messages generated              */
  QB_LSTAT_MSGS_DROPPED = 7,   /* messages not written (msg_cap / pool)    */
  QB_LSTAT_COUNT = 8
};

typedef struct qb_leader_groups {
  uint64_t G;
  uint32_t inflight_cap; /* MaxInflightMsgs: ring size per slot, 1..4096  */
  uint32_t readq_cap;    /* pending ReadIndex slots per group, 0..16      */
  uint32_t read_only;    /* QB_READ_ONLY_SAFE / QB_READ_ONLY_LEASE_BASED  */
  uint32_t options;      /* QB_LEADER_OPT_* (0 = defaults)                */
  /* configuration, CSR as qb_dev_csr_committed_vote */
  const uint32_t* off;   /* [G+1] */
  const uint32_t* cfg;   /* [G] mask_in | mask_out << 16 */
  /* per group */
  uint32_t* meta;        /* [G] see QB_META_* (in/out)                     */
  const uint64_t* term;  /* [G] raft.Term                                  */
  uint64_t* committed;   /* [G] raftLog.committed (in/out)                 */
  const uint64_t* first_index; /* [G] raftLog.firstIndex()                 */
  const uint64_t* last_index;  /* [G] raftLog.lastIndex()                  */
  const uint64_t* snap_index;  /* [G] storage snapshot index, 0 = unavailable */
  const uint64_t* snap_term;   /* [G]                                      */
  const uint64_t* max_ents;    /* [G] entries per MsgApp (>= 1)            */
  const uint64_t* run_start;   /* [QB_LEADER_MAX_RUNS * G] run-major: run r of
                                  group g at r * G + g; ascending in r        */
  const uint64_t* run_term;    /* [QB_LEADER_MAX_RUNS * G] same layout      */
  /* per slot, S = off[G] (in/out) */
  uint64_t* match;
  uint64_t* next;
  uint64_t* pending_snapshot;
  uint8_t* pstate;       /* QB_PR_* */
  uint32_t* infl_pos;    /* start | count << 16; start < inflight_cap, count <=
                            inflight_cap (the ring's invariant, not checked here:
                            etcd_amd/quorum/leader.py checks it on the host) */
  uint64_t* infl_buf;    /* [S * inflight_cap] ring */
  /* pending ReadIndex queue, oldest first: [G * readq_cap] (in/out) */
  uint64_t* rq_ctx;
  uint64_t* rq_index;
  uint32_t* rq_meta;     /* ack slot bits (0-15) | request From slot << 16 (0xFF = local) */
} qb_leader_groups;

typedef struct qb_leader_inbox {
  uint64_t M;
  const uint32_t* group;
  const uint8_t* flags;  /* slot (0-3) | kind << 4 | QB_REC_NO_PROGRESS | QB_REC_REJECT */
  const uint64_t* index; /* Message.Index; MsgHeartbeatResp: Context (0 = empty) */
  const uint64_t* term;  /* Message.Term (0 = local message)                */
  const uint64_t* hint;  /* Message.RejectHint (nullable: no rejections)    */
  const uint64_t* log_term; /* Message.LogTerm (nullable)                   */
} qb_leader_inbox;

typedef struct qb_msg_out {
  uint64_t index;    /* MsgApp: Index (= Next-1); MsgSnap: snapshot index; reads: read index */
  uint64_t log_term; /* MsgApp: LogTerm; MsgSnap: snapshot term */
  uint64_t commit;   /* MsgApp: Commit */
  uint64_t aux;      /* MsgApp: number of entries (Index+1 ..); reads: request ctx */
  uint32_t group;
  uint8_t to;        /* destination slot (0xFF for a local ReadState) */
  uint8_t type;      /* QB_MSG_* */
  uint16_t reserved;
} qb_msg_out;

size_t qb_leader_workspace_bytes(uint64_t G, uint64_t M);
/* msgs: device buffer of msg_cap records; msg_total (device uint64) receives
 * the number generated (only the first msg_cap, in group order, are written);
 * msg_off (device [G+1], nullable) the first message of each group.
 * stepdown_at (device [G], nullable): batch index of the group's step-down
 * record or UINT32_MAX; gflags (device [G], nullable): QB_LFLAG_*.
 * stats: QB_LSTAT_COUNT device uint64 (accumulated). */
int qb_dev_leader_step(const qb_leader_groups* lg, const qb_leader_inbox* in,
                       qb_msg_out* msgs, uint64_t msg_cap, uint64_t* msg_total,
                       uint32_t* msg_off, uint32_t* stepdown_at, uint8_t* gflags,
                       uint64_t* stats, void* workspace, size_t workspace_bytes,
                       void* stream);

/* The same step with the messages left where the step writes them, in a
 * per-group outbox — the reference's per-node r.msgs slice (raft.go:393-420
 * r.send appends to it; Ready.Messages hands it over, node.go:573) as an
 * 8-message array per group plus an overflow list — instead of one
 * group-ordered array (qb_dev_leader_step compacts them in a second pass:
 * a scan of the counts, then every message read and written again).  Group
 * g's k-th message is slots[k * G + g] for k < QB_LEADER_OUTBOX_SLOTS; the
 * ones past it continue in QB_LEADER_OUTBOX_CHUNK-message chunks drawn from
 * chunks[] (chunk c holds chunks[c * 32 .. c * 32 + 31]; chunk_head[g] is
 * g's first chunk, chunk_next[c] the next), in the order the reference
 * emits them.  count[g] = messages stored for g (a group whose chunk could
 * not be drawn — all nchunks used — stops there; the rest is counted in
 * QB_LSTAT_MSGS_DROPPED); *chunks_used (device u32) = chunks drawn, at most
 * nchunks (chunks[0 .. chunks_used) hold messages).
 * read_states (nullable): the local reads' answers kept apart from the
 * messages, as the reference keeps them (responseToReadIndexReq appends a
 * ReadState to r.readStates, raft.go:1737-1745; Ready.ReadStates,
 * node.go:67,580): group g's k-th ReadState is read_states[k * G + g] for
 * k < read_count[g] (at most lg->readq_cap: a step releases no more reads
 * than the queue held), oldest first, and no QB_READ_STATE message is
 * emitted.  NULL keeps them in the messages as QB_READ_STATE (to 0xFF).
 * stepdown_at / gflags / stats as qb_dev_leader_step. */
#define QB_LEADER_OUTBOX_SLOTS 8
#define QB_LEADER_OUTBOX_CHUNK 32
typedef struct qb_read_state {
  uint64_t index;       /* ReadState.Index                                   */
  uint64_t ctx;         /* ReadState.RequestCtx (the request's 8-byte context) */
} qb_read_state;
typedef struct qb_leader_outbox {
  qb_msg_out* slots;    /* [QB_LEADER_OUTBOX_SLOTS * G], k-major             */
  uint32_t* count;      /* [G] messages per group                            */
  uint32_t* chunk_head; /* [G] (meaningful where count > 8)                  */
  uint32_t* chunk_next; /* [nchunks]                                         */
  qb_msg_out* chunks;   /* [nchunks * QB_LEADER_OUTBOX_CHUNK]                */
  uint64_t nchunks;     /* 0: no overflow (messages past the 8th dropped)    */
  uint32_t* chunks_used; /* device u32                                       */
  qb_read_state* read_states; /* nullable: [readq_cap * G], k-major          */
  uint32_t* read_count; /* [G] ReadStates per group (required with read_states) */
} qb_leader_outbox;
size_t qb_leader_outbox_workspace_bytes(uint64_t G, uint64_t M);
int qb_dev_leader_step_outbox(const qb_leader_groups* lg, const qb_leader_inbox* in,
                              const qb_leader_outbox* out, uint32_t* stepdown_at,
                              uint8_t* gflags, uint64_t* stats, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------------- */
/* Leader tick: heartbeats, CheckQuorum sweep, election timers             */
/* ----------------------------------------------------------------------- */

/* raft.tick() (tickElection / tickHeartbeat, raft.go:645-684) for G groups in
 * one call: what a multi-raft host runs once per tick interval for every
 * group it hosts.  Per group, groups independent:
 *   not a leader (tickElection): electionElapsed++; a promotable node past
 *     its randomized timeout (raft.go:1618-1621, 1714-1716) resets the
 *     counter and gets QB_TFLAG_HUP — the campaign (Step MsgHup) is the
 *     host's;
 *   leader (tickHeartbeat): both counters++.  At electionElapsed >=
 *     election_timeout the counter resets and, with check_quorum, the
 *     MsgCheckQuorum step runs (raft.go:997-1018): the leader's own Progress
 *     is marked RecentActive (if it has one), ProgressTracker.QuorumActive
 *     (tracker/tracker.go:215-225: RecentActive of every voter, learners
 *     skipped, VoteWon in both halves, an empty half wins — the rule of
 *     qb_dev_csr_quorum_active) decides whether the leader steps down, and
 *     QB_PR_RECENT_ACTIVE is cleared on every slot but the leader's
 *     (learners included).  A leader that stays one drops a pending
 *     leadership transfer (meta transferee := 0xFF, raft.go:669-671,
 *     QB_TFLAG_TRANSFER_ABORTED).  A leader that stays one and whose
 *     heartbeatElapsed >= heartbeat_timeout resets that counter and
 *     broadcasts (MsgBeat -> bcastHeartbeat, raft.go:994-996, 495-541): for
 *     every slot s but its own, voters and learners, hb_commit[s] =
 *     min(match[s], committed[g]), and hb_ctx[g] = the context of the newest
 *     pending ReadIndex request (read_only.go:116-121: rq_ctx[g * readq_cap +
 *     nq - 1], 0 if the queue is empty).
 * Step-down is becomeFollower(r.Term, None) -> reset (raft.go:590-619)
 * restricted to the fields this call owns: role := Follower (every other
 * bit of the role byte kept), both counters 0, meta transferee := 0xFF
 * (without QB_TFLAG_TRANSFER_ABORTED), QB_PR_RECENT_ACTIVE cleared on every
 * slot (reset zeroes the leader's own Progress too), QB_TFLAG_STEPPED_DOWN;
 * a leader that steps down sends no heartbeat on that tick.  The rest of
 * reset stays the host's, as stepdown_at is for the leader step: Match / Next
 * / Inflights, readOnly, the votes, lead and the new randomized timeout.
 *
 * The host forms the heartbeats of a group with QB_TFLAG_BEAT as
 *   pb.Message{Type: MsgHeartbeat (QB_MSG_HEARTBEAT), To: ids[s], From: its own
 *              ID, Term: term[g], Commit: hb_commit[s], Context: hb_ctx[g]}
 * for every slot s of the group but the leader's, ascending — the order of
 * ProgressTracker.Visit (tracker.go:191-212; ascending IDs are ascending CSR
 * slots); hb_ctx 0 is the empty context, anything else the request's 8-byte
 * big-endian id.  Heartbeats stay slot-aligned: 8 bytes per peer.
 *
 * A leader slot (meta bits 0-7) >= the group's slot count means the leader
 * has no Progress (raft.go:998-1006): nothing is self-activated and every
 * slot gets a heartbeat.  A slot count above QB_MAX_SLOTS is read as
 * QB_MAX_SLOTS and a request count above readq_cap as readq_cap; the tick
 * never reads or writes outside the caller's arrays. */
#define QB_MSG_HEARTBEAT 8 /* pb.MsgHeartbeat (raft.pb.go:76-94) */

/* role byte: raft.StateType (raft.go:39-45) in bits 0-1 | flags. */
#define QB_ROLE_FOLLOWER 0
#define QB_ROLE_CANDIDATE 1
#define QB_ROLE_LEADER 2
#define QB_ROLE_PRE_CANDIDATE 3
#define QB_ROLE_PROMOTABLE 0x80u /* raft.promotable(), maintained by the host */

/* Per-group output flags of the tick. */
#define QB_TFLAG_HUP 0x01u              /* election timeout: campaign (QB_CAMP_HUP) */
#define QB_TFLAG_BEAT 0x02u             /* heartbeats written                   */
#define QB_TFLAG_STEPPED_DOWN 0x04u     /* CheckQuorum failed (= QB_LFLAG_STEPPED_DOWN) */
#define QB_TFLAG_CHECK_QUORUM 0x08u     /* the MsgCheckQuorum step ran          */
#define QB_TFLAG_TRANSFER_ABORTED 0x10u /* the lead transfer timed out          */

enum {
  QB_TSTAT_LEADERS = 0,          /* groups ticked as leader (tickHeartbeat)    */
  QB_TSTAT_NON_LEADERS = 1,      /* groups ticked otherwise (tickElection)     */
  QB_TSTAT_BEATS = 2,            /* groups that broadcast                      */
  QB_TSTAT_HEARTBEATS = 3,       /* heartbeats sent (hb_commit entries written) */
  QB_TSTAT_CHECK_QUORUM = 4,     /* MsgCheckQuorum steps                       */
  QB_TSTAT_STEPPED_DOWN = 5,     /* leaders that stepped down                  */
  QB_TSTAT_TRANSFER_ABORTED = 6, /* lead transfers aborted                     */
  QB_TSTAT_HUPS = 7,             /* election timeouts                          */
  QB_TSTAT_COUNT = 8
};

/* The arrays are those of qb_leader_groups (same layouts: a caller passes the
 * same buffers) plus the tick's own per-group state. */
typedef struct qb_tick_groups {
  uint64_t G;
  uint32_t readq_cap;         /* 0..QB_LEADER_MAX_READQ                       */
  uint32_t election_timeout;  /* raft.electionTimeout (ticks, >= 1)           */
  uint32_t heartbeat_timeout; /* raft.heartbeatTimeout (ticks, >= 1)          */
  uint32_t check_quorum;      /* raft.checkQuorum: 0 / 1                      */
  const uint32_t* off;        /* [G+1] */
  const uint32_t* cfg;        /* [G] */
  uint32_t* meta;             /* [G] in/out: only bits 8-15 (transferee) may change */
  const uint64_t* committed;  /* [G] */
  const uint64_t* match;      /* [off[G]] */
  uint8_t* pstate;            /* [off[G]] in/out: only QB_PR_RECENT_ACTIVE may change */
  const uint64_t* rq_ctx;     /* [G * readq_cap]; NULL iff readq_cap == 0     */
  uint8_t* role;              /* [G] in/out: QB_ROLE_*                        */
  uint32_t* election_elapsed; /* [G] in/out */
  uint32_t* heartbeat_elapsed; /* [G] in/out */
  const uint32_t* rand_timeout; /* [G] raft.randomizedElectionTimeout         */
} qb_tick_groups;

/* tflags [G]: QB_TFLAG_*, written for every group (0 where nothing fired).
 * hb_commit [off[G]] / hb_ctx [G]: written only where a heartbeat is sent
 * (a beating group's peer slots / a beating group); every other element is
 * left untouched.  stats: QB_TSTAT_COUNT device uint64 (accumulated).
 * G == 0 is QB_OK and writes nothing; everything else is required. */
int qb_dev_leader_tick(const qb_tick_groups* tg, uint8_t* tflags, uint64_t* hb_commit,
                       uint64_t* hb_ctx, uint64_t* stats, void* stream);

/* ----------------------------------------------------------------------- */
/* Follower step: heartbeats, vote requests, MsgTimeoutNow                 */
/* ----------------------------------------------------------------------- */

/* raft.Step (raft.go:847-984) for the inbox of nodes that receive
 * MsgHeartbeat / MsgVote / MsgPreVote / MsgTimeoutNow, for G groups in one
 * call: the receiving side of qb_dev_leader_tick's heartbeats, of
 * QB_MSG_TIMEOUT_NOW and of the requests whose answers qb_dev_record_votes
 * consumes.  Each group's records are applied in batch order; groups are
 * independent.  No configuration and no Progress are read: Step checks no
 * membership for these types and learners vote too (raft.go:939-956).
 *
 * Term filter (raft.go:849-920), per record with Term != 0 (0 is a local
 * message and skips it):
 *   higher term: a MsgVote / MsgPreVote with check_quorum && lead != 0 &&
 *     election_elapsed < election_timeout and without QB_FREC_FORCE is
 *     dropped (the leader's lease).  MsgPreVote never changes the term; a
 *     heartbeat runs becomeFollower(m.Term, m.From), a MsgVote or
 *     MsgTimeoutNow becomeFollower(m.Term, None);
 *   lower term: a heartbeat with check_quorum || pre_vote is answered with
 *     MsgAppResp (raft.go:906; send stamps Term = term[g]), a MsgPreVote
 *     with MsgPreVoteResp, Reject, Term = term[g]; anything else is ignored.
 * becomeFollower -> reset (raft.go:686-693, 590-619), restricted to the
 * fields this call owns: term (and vote := 0) change only if the term
 * differs, lead is set, both counters 0, role := Follower with the other bits
 * of the byte kept, QB_FFLAG_RESET.  The rest of reset stays the host's, as
 * for the tick: Progress, the votes, readOnly, the transferee and the new
 * randomized timeout.
 * MsgVote / MsgPreVote (raft.go:930-978), in any role: canVote = vote == From
 *   || (vote == 0 && lead == 0) || (MsgPreVote && m.Term > term), and
 *   raftLog.isUpToDate(Index, LogTerm) (log.go:316-318) against last_term /
 *   last_index.  A grant answers with Term = m.Term, and for MsgVote only sets
 *   election_elapsed = 0 and vote = From; a rejection answers with Term =
 *   term[g] and Reject.
 * MsgHeartbeat at or above the term: a follower sets election_elapsed = 0 and
 *   lead = From (raft.go:1437-1440), a (pre-)candidate first runs
 *   becomeFollower(m.Term, m.From) (raft.go:1393-1395); then handleHeartbeat
 *   (raft.go:1513-1516): committed = max(committed, Commit) and a
 *   MsgHeartbeatResp with Term = term[g] (the host copies the record's
 *   context).  A leader ignores it (stepLeader has no case for it).
 * MsgTimeoutNow (raft.go:1415-1416, 1452-1457, 760-768): only a follower with
 *   QB_ROLE_PROMOTABLE acts on it; the campaign is the host's, so the group
 *   stops there (below).  Every other role ignores it.
 *
 * Stops.  stop_at[g] = batch index of the first record whose effect is the
 * host's, UINT32_MAX if none:
 *   a QB_FIN_HOST record (a message the host steps itself: MsgApp, MsgSnap,
 *     MsgProp, ...; it is in the batch only to keep the order): nothing of it
 *     is applied, QB_FFLAG_HOST_MSG;
 *   the MsgTimeoutNow of a promotable follower: the term filter's effect is
 *     kept, QB_FFLAG_CAMPAIGN;
 *   a heartbeat that would reach commitTo with committed < Commit &&
 *     last_index < Commit (Go panics, log.go:236-244): nothing of it is
 *     applied, QB_FFLAG_COMMIT_RANGE.
 * The group's records behind the stop are not applied, get no response and
 * count as QB_FSTAT_AFTER_STOP; the host re-submits them.
 *
 * Responses are record-aligned (a record yields at most one message):
 * resp_type[i] = pb MessageType | QB_FRESP_REJECT, 0 = no message;
 * resp_term[i] = Message.Term; To = from[i].  Both are written for every
 * record.  gflags[g] (QB_FFLAG_*) and stop_at[g] are written for every group.
 * QB_FFLAG_HARDSTATE: term, vote or committed differ from their values at
 * entry — what Ready persists before the responses may be sent. */
#define QB_FIN_HEARTBEAT 0
#define QB_FIN_VOTE 1
#define QB_FIN_PREVOTE 2
#define QB_FIN_TIMEOUT_NOW 3
#define QB_FIN_HOST 4
#define QB_FREC_KIND_MASK 0x07u
#define QB_FREC_FORCE 0x80u /* Context == "CampaignTransfer" (raft.go:854) */

#define QB_FRESP_APP_RESP 4        /* pb.MsgAppResp       */
#define QB_FRESP_VOTE_RESP 6       /* pb.MsgVoteResp      */
#define QB_FRESP_HEARTBEAT_RESP 9  /* pb.MsgHeartbeatResp */
#define QB_FRESP_PREVOTE_RESP 18   /* pb.MsgPreVoteResp   */
#define QB_FRESP_REJECT 0x80u

#define QB_FFLAG_HOST_MSG 0x01u     /* stopped at a QB_FIN_HOST record        */
#define QB_FFLAG_CAMPAIGN 0x02u     /* stopped at MsgTimeoutNow: QB_CAMP_TRANSFER */
#define QB_FFLAG_COMMIT_RANGE 0x04u /* stopped at a Commit past last_index    */
#define QB_FFLAG_RESET 0x08u        /* becomeFollower ran: the host's reset   */
#define QB_FFLAG_HARDSTATE 0x10u    /* term / vote / committed changed        */

enum {
  QB_FSTAT_HEARTBEATS = 0,      /* heartbeats handled (handleHeartbeat)       */
  QB_FSTAT_GRANTED = 1,         /* (pre-)votes granted                        */
  QB_FSTAT_REJECTED = 2,        /* (pre-)votes rejected at or above the term  */
  QB_FSTAT_LEASE_DROPPED = 3,   /* higher-term (pre-)votes dropped in lease   */
  QB_FSTAT_STALE_IGNORED = 4,   /* lower-term records ignored                 */
  QB_FSTAT_STALE_ANSWERED = 5,  /* lower-term records answered                */
  QB_FSTAT_ROLE_IGNORED = 6,    /* records the node's role ignores            */
  QB_FSTAT_BECAME_FOLLOWER = 7, /* becomeFollower calls                       */
  QB_FSTAT_AFTER_STOP = 8,      /* records behind their group's stop          */
  QB_FSTAT_BAD_GROUP = 9,       /* group >= G, dropped                        */
  QB_FSTAT_BAD_KIND = 10,       /* kind above QB_FIN_HOST, dropped            */
  QB_FSTAT_COUNT = 11
};

/* role / election_elapsed / heartbeat_elapsed are the tick's buffers (same
 * layouts: a caller passes the same arrays to both calls). */
typedef struct qb_follower_groups {
  uint64_t G;
  uint32_t election_timeout;   /* raft.electionTimeout (ticks, >= 1)          */
  uint32_t check_quorum;       /* raft.checkQuorum: 0 / 1                     */
  uint32_t pre_vote;           /* raft.preVote: 0 / 1                         */
  uint32_t reserved;           /* 0                                           */
  uint64_t* term;              /* [G] in/out                                  */
  uint64_t* vote;              /* [G] in/out: raft ID, 0 = None               */
  uint64_t* lead;              /* [G] in/out: raft ID, 0 = None               */
  uint64_t* committed;         /* [G] in/out                                  */
  const uint64_t* last_index;  /* [G] raftLog.lastIndex()                     */
  const uint64_t* last_term;   /* [G] raftLog.lastTerm()                      */
  uint8_t* role;               /* [G] in/out: QB_ROLE_*                       */
  uint32_t* election_elapsed;  /* [G] in/out */
  uint32_t* heartbeat_elapsed; /* [G] in/out */
} qb_follower_groups;

/* M records in arrival order (SoA). */
typedef struct qb_follower_inbox {
  uint64_t M;            /* <= 2^32 - 2                                       */
  const uint32_t* group; /* [M] */
  const uint8_t* flags;  /* [M] QB_FIN_* in bits 0-2 | QB_FREC_FORCE          */
  const uint64_t* from;  /* [M] sender ID                                     */
  const uint64_t* term;  /* [M] Message.Term; 0 = local message               */
  const uint64_t* index; /* [M] votes: Index; heartbeat: Commit               */
  const uint64_t* aux;   /* [M] votes: LogTerm; heartbeat: the 8-byte context
                          *     id (0 = empty), kept for the host             */
} qb_follower_inbox;

/* stats: QB_FSTAT_COUNT device uint64 (accumulated).  G == 0 or M == 0 is
 * QB_OK; with M == 0 and G > 0 the per-group outputs are still initialised.
 * No allocation inside the call (it can be graph-captured); nothing outside
 * the caller's arrays is read or written. */
size_t qb_follower_workspace_bytes(uint64_t G, uint64_t M);
int qb_dev_follower_step(const qb_follower_groups* fg, const qb_follower_inbox* in,
                         uint8_t* resp_type, uint64_t* resp_term, uint32_t* stop_at,
                         uint8_t* gflags, uint64_t* stats, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------------- */
/* Follower log step: the follower step plus MsgApp                        */
/* ----------------------------------------------------------------------- */

/* qb_dev_follower_step with one more record kind, QB_FIN_APP (pb.MsgApp): the
 * receiving side of qb_dev_leader_step's QB_MSG_APP.  Kinds 0-4 behave exactly
 * as above and all kinds of a group are stepped in one batch order, so a vote
 * request or a heartbeat behind an append sees the log it left.  The entries'
 * bytes stay the host's: the call decides accept or reject, where the append
 * starts, the log's new end and term index, the commit and the response.
 *
 * The log is its term index, as for the leader: the terms of
 * [first_index - 1, last_index] as up to QB_LEADER_MAX_RUNS runs (run-major;
 * the count in bits 16-19 of meta).  Run 0 starts at first_index - 1 (the
 * dummy entry), starts ascend, the last run's term is last_term, adjacent
 * runs differ in term, and first_index - 1 <= committed.  (The table is not
 * checked on the device; etcd_amd/quorum/follower.py checks it on the host.
 * Whatever it holds, nothing outside the caller's arrays is touched.)
 *
 * A QB_FIN_APP record: index = Message.Index, aux = Message.LogTerm,
 * commit[i] = Message.Commit, and the entries, which have the indexes
 * Index + 1, Index + 2, ..., run-length encoded by term in ent_term /
 * ent_len[ent_off[i] .. ent_off[i + 1]).  A message whose entries are not
 * consecutive from Index + 1 is the decoder's to send as QB_FIN_HOST.
 *
 * Term filter (raft.go:849-920): a higher term runs becomeFollower(m.Term,
 *   m.From) (raft.go:876-877); a lower term with check_quorum || pre_vote is
 *   answered with MsgAppResp, Term = term[g], resp_index 0 (raft.go:884, 906;
 *   QB_FSTAT_STALE_ANSWERED), any other lower term is ignored.
 * By role at or above the term: a leader ignores it (stepLeader has no case
 *   for it; QB_FSTAT_ROLE_IGNORED), a (pre-)candidate runs
 *   becomeFollower(m.Term, m.From) (raft.go:1390-1392), a follower sets
 *   election_elapsed = 0 and lead = From (raft.go:1433-1435).
 * handleAppendEntries (raft.go:1475-1511):
 *   Index < committed: MsgAppResp{Index: committed}.
 *   Accept, matchTerm(Index, LogTerm) (log.go:320-326; term() is 0 outside
 *     [first_index - 1, last_index], log.go:268-274): lastnewi = Index +
 *     number of entries; ci = findConflict (log.go:130-141), evaluated a run
 *     at a time.  ci != 0: the log is truncated behind ci - 1 and takes the
 *     entries from ci on (log.go:96-101, unstable.truncateAndAppend): runs
 *     starting at or after ci are dropped, the message's runs from ci on are
 *     appended, a run whose term equals the term before it is merged into
 *     it; last_index := lastnewi, last_term := the last entry's term, the
 *     run count in meta updated, app_from[i] = ci, QB_FFLAG_APPENDED.  Then
 *     committed := max(committed, min(Commit, lastnewi)) (log.go:103,
 *     236-244) and MsgAppResp{Index: lastnewi}.
 *   Reject (raft.go:1496-1509): hint = findConflictByTerm(min(Index,
 *     last_index), LogTerm) (log.go:150-171); resp_index = Index,
 *     QB_FRESP_REJECT, resp_hint = hint, resp_log_term = term(hint).
 *   resp_term = term[g] behind the filter, as send stamps it.
 * Four more stops, each found before anything of the record is applied (the
 * term filter's effect included), each with stop_at[g] = the record:
 *   QB_FFLAG_LOG_CONFLICT: 0 < ci <= committed (Go panics, log.go:94-95), or
 *     ci > last_index + 1: the append would leave a gap
 *     (unstable.truncateAndAppend's slice bounds) — where a zero LogTerm or
 *     entry term "matching" outside the log ends up;
 *   QB_FFLAG_LOG_RUNS: the table behind the append would hold more than
 *     QB_LEADER_MAX_RUNS runs (the host runs qb_dev_log_compact, or steps the
 *     message);
 *   QB_FFLAG_COMMIT_RANGE: commitTo's range panic (log.go:239-241) against
 *     the last index the record would leave.
 * Index arithmetic wraps as Go's uint64 does.
 *
 * resp_index[i] and app_from[i] are written for every record (0: none);
 * resp_hint[i] / resp_log_term[i] only with a rejected MsgAppResp.  The host
 * applies app_from in batch order. */
#define QB_FIN_APP 5                 /* pb.MsgApp; accepted by qb_dev_follower_log_step only */
#define QB_FFLAG_LOG_CONFLICT 0x20u  /* stopped: the append is one Go panics on          */
#define QB_FFLAG_LOG_RUNS     0x40u  /* stopped: the append needs a 9th term run         */
#define QB_FFLAG_APPENDED     0x80u  /* the log changed: entries to persist before the
                                        responses may be sent                            */

/* stats of the log step: QB_FSTAT_* (same meaning) and five more. */
enum {
  QB_FLSTAT_APP_ACCEPTED = 11,     /* MsgApp accepted (maybeAppend ok)           */
  QB_FLSTAT_APP_REJECTED = 12,     /* MsgApp rejected with a hint                */
  QB_FLSTAT_APP_BELOW_COMMIT = 13, /* Index < committed                          */
  QB_FLSTAT_ENTRIES_APPENDED = 14, /* entries the logs took (lastnewi - ci + 1)  */
  QB_FLSTAT_APP_TRUNCATED = 15,    /* appends that started at or below lastIndex */
  QB_FLSTAT_COUNT = 16
};

typedef struct qb_follower_log {
  uint32_t* meta;              /* [G] in/out: only bits 16-19 (term runs, 1..8) may change;
                                  0 is read as 1, above 8 as 8                              */
  const uint64_t* first_index; /* [G] raftLog.firstIndex()                                  */
  uint64_t* last_index;        /* [G] in/out; must be fg->last_index (same pointer)         */
  uint64_t* last_term;         /* [G] in/out; must be fg->last_term                         */
  uint64_t* run_start;         /* [QB_LEADER_MAX_RUNS * G] in/out, run-major as qb_leader_groups:
                                  run 0 starts at first_index - 1, ascending, last run's
                                  term == last_term                                          */
  uint64_t* run_term;          /* same layout                                                */
} qb_follower_log;

typedef struct qb_follower_app_inbox {   /* beside qb_follower_inbox, same M */
  const uint64_t* commit;   /* [M] Message.Commit (used for QB_FIN_APP only)                 */
  const uint32_t* ent_off;  /* [M+1] record i's entries, run-length encoded by term:
                               runs ent_off[i] .. ent_off[i+1]; offsets above E read as E   */
  const uint64_t* ent_term; /* [E] Entry.Term of the run                                     */
  const uint32_t* ent_len;  /* [E] entries in the run (0: skipped)                           */
  uint64_t E;
} qb_follower_app_inbox;

typedef struct qb_follower_app_out {
  uint64_t* resp_index;    /* [M] Message.Index of the response; written for every record (0 if none) */
  uint64_t* resp_hint;     /* [M] RejectHint; written only with a rejected MsgAppResp         */
  uint64_t* resp_log_term; /* [M] LogTerm of the hint; same                                   */
  uint64_t* app_from;      /* [M] first index the host's log takes from this message, 0 = none;
                              written for every record                                        */
} qb_follower_app_out;

/* stats: QB_FLSTAT_COUNT device uint64 (accumulated).  The conventions are
 * qb_dev_follower_step's: G == 0 or M == 0 is QB_OK, no allocation inside the
 * call, nothing outside the caller's arrays is read or written.  The
 * grouping is the follower step's and so is the workspace: its size is
 * qb_follower_workspace_bytes(G, M), there is no second size function. */
int qb_dev_follower_log_step(const qb_follower_groups* fg, const qb_follower_log* lg,
                             const qb_follower_inbox* in, const qb_follower_app_inbox* app,
                             uint8_t* resp_type, uint64_t* resp_term, const qb_follower_app_out* out,
                             uint32_t* stop_at, uint8_t* gflags, uint64_t* stats,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------------- */
/* Campaign: MsgHup and election outcomes                                  */
/* ----------------------------------------------------------------------- */

/* The state changes of an election for G groups in one call: Step(MsgHup) ->
 * hup -> campaign -> becomePreCandidate / becomeCandidate -> poll self ->
 * vote requests (raft.go:760-845), and becomeLeader (+ bcastAppend) or
 * becomeFollower once qb_dev_csr_tally_votes has the result (stepCandidate,
 * raft.go:1399-1414).  It is the piece between qb_dev_leader_tick's
 * QB_TFLAG_HUP / qb_dev_follower_step's QB_FFLAG_CAMPAIGN and the vote
 * requests that qb_dev_follower_step answers, and between the tally and the
 * new leader's first tick.  action[g], one byte per group, groups independent:
 *   QB_CAMP_NONE      nothing;
 *   QB_CAMP_HUP       Step(MsgHup): hup(campaignPreElection) with pre_vote,
 *                     else hup(campaignElection) (raft.go:922-928);
 *   QB_CAMP_TRANSFER  hup(campaignTransfer) (raft.go:1452-1457);
 *   QB_CAMP_WON       VoteWon: a pre-candidate runs campaign(campaignElection),
 *                     a candidate becomeLeader + bcastAppend;
 *   QB_CAMP_LOST      VoteLost: becomeFollower(term, None);
 *   | QB_CAMP_PENDING_CONF on HUP / TRANSFER: the host's answer to
 *                     numOfPendingConf(unapplied) != 0 && committed > applied
 *                     (raft.go:770-777; the log is the host's).
 * The code is action & 0x7F; QB_CAMP_PENDING_CONF on any other code means
 * nothing, and a code above QB_CAMP_LOST is treated as QB_CAMP_NONE and
 * counted (QB_CSTAT_BAD_ACTION).  WON / LOST on a group that is neither
 * candidate nor pre-candidate is ignored (QB_CFLAG_IGNORED).
 *
 * hup (raft.go:760-781) is ignored, in this order, by a leader, by a node that
 * is not promotable (promotable: QB_ROLE_PROMOTABLE is set, the own slot —
 * meta bits 0-7, "the leader slot" of the other calls, in every role — is
 * below the group's slot count and is a voter of either half) and under
 * QB_CAMP_PENDING_CONF; a (pre-)candidate whose timer fired again campaigns
 * again.
 * becomePreCandidate (raft.go:708-722): votes := 0, lead := 0, role :=
 *   PreCandidate with the other bits of the byte kept; nothing else changes.
 * becomeCandidate (raft.go:695-706): reset(term + 1), vote := self_id, role :=
 *   Candidate.
 * reset(t) (raft.go:590-619): term := t and vote := 0 if the term differs;
 *   lead := 0, both counters 0, meta transferee := 0xFF, meta pending-read
 *   count (bits 20-24) := 0, votes := 0, and for every slot of the group
 *   match := 0 (own slot: last_index), next := last_index + 1, pstate :=
 *   QB_PR_PROBE with no flag bits, pending_snapshot := 0, infl_pos := 0 (the
 *   ring's contents are dead).  No slot is read.
 * poll self (raft.go:803, 837-845) after either become: votes := bit | bit <<
 *   16 for the own slot (no bit for an own slot >= 16), then
 *   JointConfig.VoteResult against cfg.  VoteWon from a pre-campaign continues
 *   with becomeCandidate and polls again; VoteWon from a candidacy continues
 *   with becomeLeader, without bcastAppend (raft.go:803-811).  Otherwise the
 *   vote requests are per-group outputs (raft.go:813-834):
 *     req_type[g] = 5 (pb.MsgVote) or 17 (pb.MsgPreVote), | QB_CREQ_TRANSFER
 *                   when the Context is "CampaignTransfer";
 *     req_term[g] = term after the become, term + 1 for a pre-vote;
 *     req_mask[g] = the voters of either half minus the own slot: one message
 *                   per set bit, ascending (ascending IDs are ascending slots),
 *                   Index / LogTerm = last_index[g] / last_term[g].
 * becomeLeader (raft.go:724-758): reset(term), lead := self_id, role := Leader;
 *   the own slot, if there is one: pstate := QB_PR_REPLICATE, then
 *   appendEntry's MaybeUpdate(last_index + 1): match := last_index + 1, next :=
 *   last_index + 2 (through Go's comparisons, so a wrapped index moves
 *   neither back); maybeCommit: committed := last_index + 1 iff that exceeds
 *   it, the config has a voter and every non-empty half is {own slot}.  The
 *   empty entry itself, last_index / last_term, the term-run table and
 *   pendingConfIndex are the log's: qb_dev_leader_propose's
 *   QB_PROP_LEADER_ENTRY, or the host (QB_CFLAG_BECAME_LEADER); the call
 *   uses last_index as it stood at entry.
 * QB_CAMP_WON as a candidate also runs bcastAppend (raft.go:515-522, 432-492)
 *   on the Progress: every slot but the own becomes QB_PR_PROBE |
 *   QB_PR_PROBE_SENT, QB_CFLAG_BCAST_APPEND, and the host forms per such
 *   slot, ascending, MsgApp{Index: last_index, LogTerm: last_term, Commit:
 *   committed[g], one entry}.
 * becomeFollower(term, None) (raft.go:686-693): reset(term), role := Follower.
 * term + 1 and last_index + 1 wrap as Go's uint64 does.  A slot count above
 * QB_MAX_SLOTS is read as QB_MAX_SLOTS.
 *
 * The host's share of QB_CFLAG_RESET: the new randomized timeout,
 * uncommittedSize and the readOnly contents. */
#define QB_CAMP_NONE 0
#define QB_CAMP_HUP 1
#define QB_CAMP_TRANSFER 2
#define QB_CAMP_WON 3
#define QB_CAMP_LOST 4
#define QB_CAMP_PENDING_CONF 0x80u

#define QB_MSG_VOTE 5      /* pb.MsgVote    (raft.pb.go:76-94) */
#define QB_MSG_PREVOTE 17  /* pb.MsgPreVote                    */
#define QB_CREQ_TRANSFER 0x80u /* Context: "CampaignTransfer" (raft.go:829-832) */

#define QB_CFLAG_REQUESTS 0x01u      /* req_type / req_term / req_mask hold requests */
#define QB_CFLAG_BECAME_LEADER 0x02u /* the host appends the empty entry              */
#define QB_CFLAG_BCAST_APPEND 0x04u  /* the host sends the first MsgApp to every peer */
#define QB_CFLAG_RESET 0x08u         /* reset ran (= QB_FFLAG_RESET)                  */
#define QB_CFLAG_HARDSTATE 0x10u     /* term / vote / committed differ from entry     */
#define QB_CFLAG_IGNORED 0x20u       /* the action had no effect                      */

enum {
  QB_CSTAT_PRE_CAMPAIGNS = 0,        /* becomePreCandidate calls                  */
  QB_CSTAT_CAMPAIGNS = 1,            /* becomeCandidate calls                     */
  QB_CSTAT_BECAME_LEADER = 2,        /* becomeLeader calls                        */
  QB_CSTAT_BECAME_FOLLOWER = 3,      /* becomeFollower calls                      */
  QB_CSTAT_VOTE_REQUESTS = 4,        /* vote requests (set bits of req_mask)      */
  QB_CSTAT_IGNORED_LEADER = 5,       /* hup at a leader                           */
  QB_CSTAT_IGNORED_UNPROMOTABLE = 6, /* hup at a node that is not promotable      */
  QB_CSTAT_IGNORED_PENDING_CONF = 7, /* hup under QB_CAMP_PENDING_CONF            */
  QB_CSTAT_IGNORED_ROLE = 8,         /* WON / LOST at a follower or leader        */
  QB_CSTAT_BAD_ACTION = 9,           /* action code above QB_CAMP_LOST            */
  QB_CSTAT_COUNT = 10
};

/* The arrays are those of qb_leader_groups, qb_tick_groups and
 * qb_follower_groups (same layouts: a caller passes the same buffers) plus
 * self_id and the votes word of qb_dev_record_votes. */
typedef struct qb_campaign_groups {
  uint64_t G;
  uint32_t pre_vote;           /* raft.preVote: 0 / 1                         */
  uint32_t reserved;           /* 0                                           */
  const uint32_t* off;         /* [G+1] */
  const uint32_t* cfg;         /* [G] */
  uint32_t* meta;              /* [G] in/out: bits 8-15 and 20-24 may change  */
  const uint64_t* self_id;     /* [G] the node's raft ID                      */
  uint64_t* term;              /* [G] in/out */
  uint64_t* vote;              /* [G] in/out */
  uint64_t* lead;              /* [G] in/out */
  uint64_t* committed;         /* [G] in/out */
  const uint64_t* last_index;  /* [G] */
  const uint64_t* last_term;   /* [G] (the requests' LogTerm; not read here)  */
  uint8_t* role;               /* [G] in/out: QB_ROLE_*                       */
  uint32_t* election_elapsed;  /* [G] in/out */
  uint32_t* heartbeat_elapsed; /* [G] in/out */
  uint32_t* votes;             /* [G] in/out: voted | granted << 16           */
  /* per slot, S = off[G] (in/out; written only by reset) */
  uint64_t* match;
  uint64_t* next;
  uint64_t* pending_snapshot;
  uint8_t* pstate;
  uint32_t* infl_pos;
} qb_campaign_groups;

/* cflags [G] (QB_CFLAG_*) and req_type [G] (0 = no request) are written for
 * every group; req_term / req_mask only where req_type is non-zero.  stats:
 * QB_CSTAT_COUNT device uint64 (accumulated).  G == 0 is QB_OK and writes
 * nothing; everything else is required.  No workspace and no allocation
 * inside the call (it can be graph-captured); nothing outside the caller's
 * arrays is read or written. */
int qb_dev_campaign(const qb_campaign_groups* cg, const uint8_t* action, uint8_t* cflags,
                    uint8_t* req_type, uint64_t* req_term, uint16_t* req_mask, uint64_t* stats,
                    void* stream);

/* ----------------------------------------------------------------------- */
/* Propose: MsgProp, appendEntry and bcastAppend at the leader             */
/* ----------------------------------------------------------------------- */

/* Step(MsgProp) -> appendEntry -> bcastAppend (raft.go:1019-1077, 621-642,
 * 1761-1779, 432-522) and the log's share of becomeLeader (raft.go:745-756)
 * for G groups in one call: the call that lets a leader's log grow on the
 * device.  Dense, one action per group (a node receives at most one batched
 * proposal per group and call: the host concatenates a group's MsgProps),
 * groups independent.  The entries' bytes stay the host's; the call decides
 * whether they are taken, which indexes they get, the log's new end and term
 * index, the commit, and the MsgApp / MsgSnap of bcastAppend.
 *
 * action[g] & 0x3F:
 *   QB_PROP_NONE          nothing (pflags[g] = 0);
 *   QB_PROP_ENTRIES       Step(MsgProp) with n_ents[g] entries whose
 *                         PayloadSize sum is payload[g];
 *     | QB_PROP_CONF_CHANGE     entry cc_at[g] (0-based) is an EntryConfChange
 *                         / EntryConfChangeV2 of cc_payload[g] bytes
 *                         (cc_at >= n_ents reads as the bit being clear);
 *     | QB_PROP_CC_LEAVE_JOINT  that change has no Changes (wantsLeaveJoint).
 *                         A proposal with more than one conf-change entry
 *                         stays the host's;
 *   QB_PROP_LEADER_ENTRY  the log's share of becomeLeader, called after
 *                         qb_dev_campaign reported QB_CFLAG_BECAME_LEADER;
 *   any other code is treated as QB_PROP_NONE and counted
 *   (QB_PSTAT_BAD_ACTION).
 *
 * QB_PROP_ENTRIES by role (MsgProp is local, Term 0: the term filter passes
 * it).  A follower with lead == 0 or under disable_proposal_forwarding drops
 * it (raft.go:1423-1430), any other follower gets QB_PFLAG_FORWARD (the host
 * sends the message to lead[g]); a (pre-)candidate drops it (raft.go:1387-
 * 1389).  At a leader, in this order:
 *   1. n_ents == 0 (Go panics): QB_PFLAG_BAD, nothing applied.
 *   2. the own slot (meta bits 0-7) is >= the group's slot count (no
 *      Progress): dropped.
 *   3. the transferee (meta bits 8-15) is not 0xFF: dropped.
 *   4. last_term != term and the table already holds QB_LEADER_MAX_RUNS runs:
 *      QB_PFLAG_LOG_RUNS, nothing applied (qb_dev_log_compact makes room).
 *   5. the conf-change rule (raft.go:1050-1070): refused iff
 *      pending_conf_index > applied, or joint (cfg >> 16 != 0) without
 *      LEAVE_JOINT, or LEAVE_JOINT while not joint.  Refused:
 *      QB_PFLAG_CC_REFUSED (the host replaces that entry with an empty normal
 *      entry) and the size s below is payload - cc_payload; else
 *      pending_conf_index := last_index + cc_at + 1, which stands even if 6
 *      drops the proposal, as in Go.
 *   6. increaseUncommittedSize: dropped iff uncommitted_size > 0 && s > 0 &&
 *      uncommitted_size + s > max_uncommitted_size (the sum wraps as uint64;
 *      a limit of 0 is no limit, as Config.validate makes it); else
 *      uncommitted_size += s.
 *   7. append: last_term != term adds the run (last_index + 1, term);
 *      last_index += n_ents, last_term := term (QB_PFLAG_APPENDED: the
 *      entries take the indexes last_index - n_ents + 1 ..).
 *   8. MaybeUpdate(last_index) on the own slot, maybeCommit (the joint
 *      committed index over match, > committed, its term == term:
 *      QB_PFLAG_COMMITTED).
 *   9. bcastAppend (QB_PFLAG_BCAST): maybeSendAppend(to, true) for every slot
 *      but the own, exactly as qb_dev_leader_step sends (paused rule,
 *      term(next - 1), min(max_ents, last - next + 1) entries, the MsgSnap
 *      fallback with RecentActive and snap_index != 0, OptimisticUpdate +
 *      Inflights.Add in Replicate, ProbeSent in Probe).  At most one message
 *      per peer, so they are slot-indexed: msg_type[s] = 0 / QB_MSG_APP /
 *      QB_MSG_SNAP; a MsgApp is {Index: msg_index[s], LogTerm:
 *      msg_log_term[s], Commit: committed[g] after the call, msg_n[s]
 *      entries from Index + 1}, a MsgSnap carries the snapshot's index and
 *      term there.
 * QB_PROP_LEADER_ENTRY acts only at a leader (elsewhere ignored and counted):
 *   step 4's stop, then pending_conf_index := last_index as at entry, one
 *   entry appended as in 7, uncommitted_size := 0.  No Progress word is
 *   touched (qb_dev_campaign already ran MaybeUpdate(last_index + 1) and
 *   maybeCommit) and no message is produced.
 * The steady proposal (last_term == term, every peer's next - 1 at or past
 * the old last index) reads and writes no run table.  Index arithmetic wraps
 * as Go's uint64 does.  A run count of 0 in meta is read as 1, above 8 as 8;
 * a slot count above QB_MAX_SLOTS as QB_MAX_SLOTS. */
#define QB_PROP_NONE 0
#define QB_PROP_ENTRIES 1
#define QB_PROP_LEADER_ENTRY 2
#define QB_PROP_CONF_CHANGE 0x40u
#define QB_PROP_CC_LEAVE_JOINT 0x80u

#define QB_PFLAG_APPENDED 0x01u   /* the log grew: entries to persist            */
#define QB_PFLAG_BCAST 0x02u      /* bcastAppend ran: msg_type of the group's slots written */
#define QB_PFLAG_COMMITTED 0x04u  /* maybeCommit returned true                   */
#define QB_PFLAG_DROPPED 0x08u    /* ErrProposalDropped                          */
#define QB_PFLAG_FORWARD 0x10u    /* a follower: the host sends MsgProp to lead  */
#define QB_PFLAG_CC_REFUSED 0x20u /* the conf change becomes an empty normal entry */
#define QB_PFLAG_LOG_RUNS 0x40u   /* stopped: the append needs a 9th term run    */
#define QB_PFLAG_BAD 0x80u        /* stopped: an empty MsgProp (Go panics)       */

enum {
  QB_PSTAT_PROPOSALS = 0,           /* proposals appended                        */
  QB_PSTAT_ENTRIES = 1,             /* entries appended (leader entries included) */
  QB_PSTAT_DROP_NO_PROGRESS = 2,    /* the leader has no Progress of its own     */
  QB_PSTAT_DROP_TRANSFER = 3,       /* a leadership transfer is in progress      */
  QB_PSTAT_DROP_SIZE = 4,           /* over max_uncommitted_size                 */
  QB_PSTAT_DROP_NO_LEADER = 5,      /* a follower with lead == 0                 */
  QB_PSTAT_DROP_FORWARDING = 6,     /* a follower under disable_proposal_forwarding */
  QB_PSTAT_DROP_CANDIDATE = 7,      /* a (pre-)candidate                         */
  QB_PSTAT_FORWARDED = 8,
  QB_PSTAT_CC_ACCEPTED = 9,         /* pending_conf_index set                    */
  QB_PSTAT_CC_REFUSED = 10,
  QB_PSTAT_MSG_APP = 11,
  QB_PSTAT_MSG_SNAP = 12,
  QB_PSTAT_COMMITS = 13,
  QB_PSTAT_LEADER_ENTRIES = 14,
  QB_PSTAT_LOG_RUNS = 15,
  QB_PSTAT_EMPTY = 16,              /* n_ents == 0 at a leader                   */
  QB_PSTAT_IGNORED_ROLE = 17,       /* QB_PROP_LEADER_ENTRY at a non-leader      */
  QB_PSTAT_BAD_ACTION = 18,
  QB_PSTAT_COUNT = 19
};

/* The arrays are those of qb_leader_groups, qb_follower_groups and
 * qb_follower_log (same layouts: a caller passes the same buffers) plus
 * applied, uncommitted_size and pending_conf_index. */
typedef struct qb_propose_groups {
  uint64_t G;
  uint32_t inflight_cap;                /* 1..4096                              */
  uint32_t disable_proposal_forwarding; /* 0 / 1                                */
  uint64_t max_uncommitted_size;        /* 0 = no limit                         */
  const uint32_t* off;          /* [G+1] */
  const uint32_t* cfg;          /* [G] */
  const uint8_t* role;          /* [G] QB_ROLE_* */
  const uint64_t* term;         /* [G] */
  const uint64_t* lead;         /* [G] */
  const uint64_t* first_index;  /* [G] */
  const uint64_t* snap_index;   /* [G] */
  const uint64_t* snap_term;    /* [G] */
  const uint64_t* max_ents;     /* [G] */
  const uint64_t* applied;      /* [G] raftLog.applied */
  uint32_t* meta;               /* [G] in/out: only bits 16-19 may change */
  uint64_t* committed;          /* [G] in/out */
  uint64_t* last_index;         /* [G] in/out */
  uint64_t* last_term;          /* [G] in/out */
  uint64_t* run_start;          /* [QB_LEADER_MAX_RUNS * G] in/out, run-major */
  uint64_t* run_term;           /* same layout */
  uint64_t* uncommitted_size;   /* [G] in/out: raft.uncommittedSize */
  uint64_t* pending_conf_index; /* [G] in/out: raft.pendingConfIndex */
  /* per slot, S = off[G] (in/out) */
  uint64_t* match;
  uint64_t* next;
  uint64_t* pending_snapshot;
  uint8_t* pstate;
  uint32_t* infl_pos;
  uint64_t* infl_buf;           /* [S * inflight_cap] */
} qb_propose_groups;

typedef struct qb_propose_in {  /* all [G] */
  const uint8_t* action;      /* QB_PROP_* */
  const uint32_t* n_ents;     /* len(m.Entries) */
  const uint64_t* payload;    /* sum of PayloadSize over the entries */
  const uint32_t* cc_at;      /* with QB_PROP_CONF_CHANGE */
  const uint64_t* cc_payload; /* with QB_PROP_CONF_CHANGE */
} qb_propose_in;

typedef struct qb_propose_out {
  uint8_t* pflags;        /* [G] QB_PFLAG_*, written for every group */
  uint8_t* msg_type;      /* [S] written for every slot of a group with QB_PFLAG_BCAST
                             and for no other slot */
  uint64_t* msg_index;    /* [S] written only where msg_type != 0 */
  uint64_t* msg_log_term; /* [S] same */
  uint64_t* msg_n;        /* [S] same: entries of the MsgApp (0 for a MsgSnap) */
} qb_propose_out;

/* stats: QB_PSTAT_COUNT device uint64 (accumulated).  G == 0 is QB_OK and
 * writes nothing; every pointer is required.  No workspace and no allocation
 * inside the call (it can be graph-captured); nothing outside the caller's
 * arrays is read or written. */
int qb_dev_leader_propose(const qb_propose_groups* pg, const qb_propose_in* in,
                          const qb_propose_out* out, uint64_t* stats, void* stream);

/* ----------------------------------------------------------------------- */
/* Requests: MsgReadIndex and MsgTransferLeader                            */
/* ----------------------------------------------------------------------- */

/* Step(MsgReadIndex) and Step(MsgTransferLeader) for G groups in one call
 * (stepLeader raft.go:1078-1097 and 1339-1370, sendMsgReadIndexResponse
 * raft.go:1827-1843, readOnly.addRequest / recvAck read_only.go:56-76,
 * bcastHeartbeatWithCtx raft.go:495-541, stepFollower raft.go:1445-1464):
 * the call that enqueues what qb_dev_leader_step later acknowledges and
 * releases, and that sets the transferee whose catch-up qb_dev_leader_step
 * answers with QB_MSG_TIMEOUT_NOW.  Dense, groups independent: per group up
 * to max_reads read requests (the host concatenates a group's MsgReadIndex
 * as it concatenates MsgProps) and at most one transfer request.
 *
 * ORDER.  Within a group the call applies the reads in k order, then the
 * transfer.  The two kinds commute in every piece of state they touch (a
 * read never changes Progress or the transferee; a transfer never changes
 * committed, match or the read queue), so any interleaving of the same
 * messages in the reference ends in the same state and the same outputs.
 *
 * READS.  Request k of group g is rd_ctx[k * G + g] (the 8-byte context) from
 * rd_from[k * G + g]: the requesting slot, or 0xFF for a local request
 * (From == None); a request from the own slot counts as local
 * (responseToReadIndexReq, raft.go:1737-1752).  A forwarded MsgReadIndex
 * carries no term (raft.go:410-416), so there is no term filter.
 *   At a leader, request by request, a later one seeing what an earlier one
 *   queued:
 *   1. a context of 0 (this library's empty context): QB_RD_BAD, not applied.
 *   2. rd_from neither 0xFF nor below the group's slot count: QB_RD_HOST,
 *      not applied (rq_meta can only name a slot).
 *   3. IsSingleton (exactly one voter in the incoming half, none in the
 *      outgoing): answered at committed — QB_RD_READ_STATE for a local
 *      request, QB_RD_RESP (a MsgReadIndexResp to the slot) for a remote
 *      one; rd_index = committed.
 *   4. !committedEntryInCurrentTerm (term(committed) through the run table
 *      != term; term() is 0 outside [first_index - 1, last_index]):
 *      QB_META_PENDING_READINDEX is set, QB_RD_POSTPONED; the host keeps the
 *      message, as for QB_LFLAG_RELEASE_READS, and submits it again here.
 *   5. QB_READ_ONLY_LEASE_BASED: answered at committed as in 3.
 *   6. QB_READ_ONLY_SAFE: addRequest — a context already pending adds
 *      nothing; a new one is written at the queue's end (rq_ctx = ctx,
 *      rq_index = committed, rq_meta = from << 16) and the count in meta
 *      bits 20-24 grows; recvAck(r.id) — the own slot's ack bit is set on
 *      the entry, new or old (no bit for an own slot >= 16);
 *      bcastHeartbeatWithCtx — QB_RD_BCAST (new entry) or QB_RD_BCAST_DUP,
 *      QB_QFLAG_HEARTBEATS, and hb_commit[s] = min(match[s], committed[g])
 *      for every slot of the group but the own one, voters and learners, as
 *      the tick writes it.  The host forms one MsgHeartbeat per such slot and
 *      per broadcasting request, with that request's context.  A new context
 *      against a full queue (count == readq_cap, readq_cap 0 included):
 *      QB_RD_QUEUE_FULL, nothing applied, the host submits it again; a
 *      duplicate of a pending context behind a full queue still acks and
 *      broadcasts.
 *   At a follower (raft.go:1458-1464): lead != 0 is QB_RD_FORWARD (the host
 *   sends the request to lead[g]), else QB_RD_DROPPED.  At a (pre-)candidate:
 *   QB_RD_IGNORED (stepCandidate has no case for it).
 *
 * TRANSFER.  xf_from[g] is the transferee's slot (Message.From), 0xFF for no
 * request; xf_term[g] is Message.Term, 0 for a local message (a forwarded
 * MsgTransferLeader carries its sender's term).  In every role first Step's
 * term filter: a non-zero term below the group's is ignored, one above it is
 * the host's (QB_QFLAG_HOST: Step would becomeFollower) and nothing is
 * applied.  Then at a leader, in the reference's order:
 *   2. no Progress (slot >= the slot count) or a learner (in neither voter
 *      mask): ignored.
 *   3. a transfer is pending (meta bits 8-15 != 0xFF): to the same slot —
 *      ignored; else aborted (transferee := 0xFF, QB_QFLAG_TRANSFER_ABORTED)
 *      and the steps go on.
 *   4. the transferee is the own slot: ignored (after 3: a transfer to self
 *      still aborts a previous one).
 *   5. election_elapsed := 0, transferee := slot (QB_QFLAG_TRANSFER_STARTED);
 *      match[slot] == last_index sends QB_MSG_TIMEOUT_NOW, else sendAppend =
 *      maybeSendAppend(slot, true) exactly as qb_dev_leader_propose sends
 *      (paused rule, term(next - 1), min(max_ents, last - next + 1) entries,
 *      the MsgSnap fallback with RecentActive and snap_index != 0 and
 *      BecomeSnapshot, OptimisticUpdate + Inflights.Add in Replicate,
 *      ProbeSent in Probe).  xf_type[g] = 0 / QB_MSG_TIMEOUT_NOW / QB_MSG_APP
 *      / QB_MSG_SNAP; a MsgApp is {To: xf_from[g], Index: xf_index[g],
 *      LogTerm: xf_log_term[g], Commit: committed[g], xf_n[g] entries}, a
 *      MsgSnap carries the snapshot's index and term there.
 * At a follower: lead != 0 is QB_QFLAG_FORWARD, else dropped.  At a
 * (pre-)candidate: ignored.
 *
 * n_reads[g] > max_reads is read as max_reads and counted; a slot count above
 * QB_MAX_SLOTS is read as QB_MAX_SLOTS, a run count of 0 as 1 and above 8 as
 * 8, a request count above readq_cap as readq_cap.  Nothing outside the
 * caller's arrays is read or written, whatever they hold. */
#define QB_REQ_MAX_READS 16

/* rd_status */
#define QB_RD_READ_STATE 1  /* a ReadState{rd_index, ctx} for the local reader   */
#define QB_RD_RESP 2        /* MsgReadIndexResp{To: rd_from, Index: rd_index, ctx} */
#define QB_RD_BCAST 3       /* queued; heartbeats with the context               */
#define QB_RD_BCAST_DUP 4   /* already pending; acked, heartbeats again          */
#define QB_RD_POSTPONED 5   /* no commit in this term yet: the host keeps it     */
#define QB_RD_FORWARD 6     /* a follower: the host sends it to lead[g]          */
#define QB_RD_DROPPED 7     /* a follower without a leader                       */
#define QB_RD_IGNORED 8     /* a (pre-)candidate                                 */
#define QB_RD_QUEUE_FULL 9  /* not applied: submit again                         */
#define QB_RD_HOST 10       /* rd_from names no slot: the host's                 */
#define QB_RD_BAD 11        /* a context of 0                                    */

#define QB_QFLAG_HEARTBEATS 0x01u        /* hb_commit of the group's peer slots written */
#define QB_QFLAG_POSTPONED 0x02u         /* a read was postponed                 */
#define QB_QFLAG_TRANSFER_STARTED 0x04u  /* transferee set, xf_type says what was sent */
#define QB_QFLAG_TRANSFER_ABORTED 0x08u  /* the previous transfer was aborted    */
#define QB_QFLAG_FORWARD 0x10u           /* a request goes to lead[g]            */
#define QB_QFLAG_HOST 0x20u              /* a request is left to the host        */
#define QB_QFLAG_BAD 0x40u               /* a zero context / n_reads > max_reads */

enum {
  QB_QSTAT_READ_STATES = 0,        /* QB_RD_READ_STATE                        */
  QB_QSTAT_READ_RESPS = 1,         /* QB_RD_RESP                              */
  QB_QSTAT_BCAST = 2,              /* QB_RD_BCAST                             */
  QB_QSTAT_BCAST_DUP = 3,          /* QB_RD_BCAST_DUP                         */
  QB_QSTAT_POSTPONED = 4,
  QB_QSTAT_RD_FORWARD = 5,
  QB_QSTAT_RD_DROPPED = 6,
  QB_QSTAT_RD_IGNORED = 7,
  QB_QSTAT_QUEUE_FULL = 8,
  QB_QSTAT_RD_HOST = 9,
  QB_QSTAT_BAD_CTX = 10,           /* QB_RD_BAD                               */
  QB_QSTAT_BAD_COUNT = 11,         /* groups with n_reads > max_reads         */
  QB_QSTAT_BCAST_GROUPS = 12,      /* groups with QB_QFLAG_HEARTBEATS         */
  QB_QSTAT_XF_STARTED = 13,
  QB_QSTAT_XF_TIMEOUT_NOW = 14,
  QB_QSTAT_XF_MSG_APP = 15,
  QB_QSTAT_XF_MSG_SNAP = 16,
  QB_QSTAT_XF_ABORTED = 17,
  QB_QSTAT_XF_IGN_TERM = 18,       /* a lower term                            */
  QB_QSTAT_XF_IGN_NO_PROGRESS = 19,
  QB_QSTAT_XF_IGN_LEARNER = 20,
  QB_QSTAT_XF_IGN_SAME = 21,       /* already transferring to that slot       */
  QB_QSTAT_XF_IGN_SELF = 22,
  QB_QSTAT_XF_IGN_ROLE = 23,       /* a (pre-)candidate                       */
  QB_QSTAT_XF_FORWARD = 24,
  QB_QSTAT_XF_DROPPED = 25,        /* a follower without a leader             */
  QB_QSTAT_XF_HOST = 26,           /* a higher term                           */
  QB_QSTAT_COUNT = 27
};

/* The arrays are those of qb_leader_groups, qb_tick_groups,
 * qb_follower_groups and qb_propose_groups (same layouts: a caller passes
 * the same buffers). */
typedef struct qb_request_groups {
  uint64_t G;
  uint32_t inflight_cap;        /* 1..4096                                  */
  uint32_t readq_cap;           /* 0..QB_LEADER_MAX_READQ                   */
  uint32_t read_only;           /* QB_READ_ONLY_SAFE / QB_READ_ONLY_LEASE_BASED */
  uint32_t max_reads;           /* rows of rd_*: 1..QB_REQ_MAX_READS        */
  const uint32_t* off;          /* [G+1] */
  const uint32_t* cfg;          /* [G] */
  uint32_t* meta;               /* [G] in/out: bits 8-15, 20-24 and 25 may change */
  const uint8_t* role;          /* [G] QB_ROLE_* */
  const uint64_t* term;         /* [G] */
  const uint64_t* lead;         /* [G] */
  const uint64_t* committed;    /* [G] */
  const uint64_t* first_index;  /* [G] */
  const uint64_t* last_index;   /* [G] */
  const uint64_t* last_term;    /* [G] */
  const uint64_t* snap_index;   /* [G] */
  const uint64_t* snap_term;    /* [G] */
  const uint64_t* max_ents;     /* [G] */
  const uint64_t* run_start;    /* [QB_LEADER_MAX_RUNS * G] run-major */
  const uint64_t* run_term;     /* same layout */
  uint32_t* election_elapsed;   /* [G] in/out */
  /* per slot, S = off[G] */
  const uint64_t* match;
  uint64_t* next;               /* in/out */
  uint64_t* pending_snapshot;   /* in/out */
  uint8_t* pstate;              /* in/out */
  uint32_t* infl_pos;           /* in/out */
  uint64_t* infl_buf;           /* [S * inflight_cap] in/out */
  /* the pending ReadIndex queue, [G * readq_cap] (in/out); NULL iff readq_cap == 0 */
  uint64_t* rq_ctx;
  uint64_t* rq_index;
  uint32_t* rq_meta;
} qb_request_groups;

typedef struct qb_request_in {
  const uint8_t* n_reads;   /* [G] <= max_reads */
  const uint64_t* rd_ctx;   /* [max_reads * G] k-major, as qb_leader_outbox::read_states */
  const uint8_t* rd_from;   /* [max_reads * G] k-major: slot, 0xFF = local */
  const uint8_t* xf_from;   /* [G] transferee slot, 0xFF = no request */
  const uint64_t* xf_term;  /* [G] Message.Term, 0 = local; NULL: all local */
} qb_request_in;

typedef struct qb_request_out {
  uint8_t* rd_status;     /* [max_reads * G] QB_RD_*, written only for k < n_reads[g] */
  uint64_t* rd_index;     /* [max_reads * G] written where rd_status is QB_RD_READ_STATE / QB_RD_RESP */
  uint64_t* hb_commit;    /* [S] written only in the peer slots of groups with QB_QFLAG_HEARTBEATS */
  uint8_t* xf_type;       /* [G] written for every group: 0 / QB_MSG_TIMEOUT_NOW / QB_MSG_APP / QB_MSG_SNAP */
  uint64_t* xf_index;     /* [G] written where xf_type is QB_MSG_APP / QB_MSG_SNAP */
  uint64_t* xf_log_term;  /* [G] same */
  uint64_t* xf_n;         /* [G] same: entries of the MsgApp (0 for a MsgSnap) */
  uint8_t* qflags;        /* [G] QB_QFLAG_*, written for every group */
} qb_request_out;

/* stats: QB_QSTAT_COUNT device uint64 (accumulated).  G == 0 is QB_OK and
 * writes nothing; every pointer but xf_term (and the queue's with readq_cap
 * 0) is required.  No workspace and no allocation inside the call (it can be
 * graph-captured). */
int qb_dev_leader_requests(const qb_request_groups* rg, const qb_request_in* in,
                           const qb_request_out* out, uint64_t* stats, void* stream);

/* ----------------------------------------------------------------------- */
/* Ready and Advance: which groups have work, and what the host finished   */
/* ----------------------------------------------------------------------- */

/* RawNode.HasReady / readyWithoutAccept / acceptReady / Advance
 * (rawnode.go:125-179) for G groups: after the step calls, qb_dev_ready finds
 * the groups with work and lists them densely, so the host copies back R
 * records instead of scanning G groups; after its I/O, qb_dev_advance takes R
 * records back.  The entries' bytes, the messages and the ReadStates stay
 * where the step calls left them; these calls move cursors.
 *
 * STATE.  Beside the step calls' own arrays (read only here), per group:
 *   applied             raftLog.applied;
 *   unstable_offset     unstable.offset: the unstable entries are
 *                       [unstable_offset, last_index] (log_unstable.go:23-36);
 *   usnap_index / usnap_term  the pending unstable.snapshot, index 0 = none
 *                       (qb_dev_follower_snapshot's restore sets it);
 *   prev_term / prev_vote / prev_commit   RawNode.prevHardSt;
 *   prev_lead / prev_role                 RawNode.prevSoftSt (the role without
 *                       QB_ROLE_PROMOTABLE).  NewRawNode starts both prevs at
 *                       the current state (rawnode.go:52-53);
 *   pending             QB_RDP_MSGS: len(r.msgs) > 0, QB_RDP_READSTATES:
 *                       len(r.readStates) != 0.  The host sets the bits from
 *                       the step calls' outputs;
 *   uncommitted_size    qb_propose_groups::uncommitted_size.
 *
 * qb_dev_ready, per group, in newReady's terms (node.go:564-584):
 *   QB_RDF_SOFT        lead != prev_lead, or role without QB_ROLE_PROMOTABLE
 *                      != prev_role (SoftState.equal, node.go:45-47).
 *   QB_RDF_HARD        (term, vote, committed) is not all zero and differs
 *                      from (prev_term, prev_vote, prev_commit): HasReady's
 *                      rule (rawnode.go:150-152).  newReady sets rd.HardState
 *                      whenever it differs (node.go:573-575) and
 *                      containsUpdates then asks !IsEmptyHardState
 *                      (node.go:106-110): the same answer.
 *   QB_RDF_ENTRIES     unstable_offset <= last_index (unstableEntries,
 *                      log.go:173-178): the entries [unstable_offset,
 *                      last_index], the last one's term last_term.
 *   QB_RDF_SNAPSHOT    usnap_index != 0 (hasPendingSnapshot, log.go:203-205).
 *   QB_RDF_COMMITTED   off = max(applied + 1, first_index) and committed + 1 >
 *                      off (hasNextEnts / nextEnts, log.go:183-201): the range
 *                      [off, committed], not paginated — maxNextEntsSize needs
 *                      the entries' bytes, so the host trims the range and
 *                      reports the cursor it reached to qb_dev_advance.
 *   QB_RDF_MSGS, QB_RDF_READSTATES   copied from pending.
 *   QB_RDF_MUST_SYNC   MustSync (node.go:589-595): QB_RDF_ENTRIES, or vote !=
 *                      prev_vote, or term != prev_term.
 *   QB_RDF_BAD_LOG     a state Go panics on or cannot reach: committed >
 *                      last_index with something to apply (slice's bound,
 *                      log.go:384-397), or unstable_offset > last_index + 1.
 *                      The group carries this flag alone, is listed, and
 *                      nothing of it is accepted.
 * Index arithmetic wraps as Go's uint64 does.  rflags[g] is written for every
 * group; a group is ready iff a bit other than QB_RDF_MUST_SYNC is set
 * (containsUpdates).
 *
 * The ready groups are listed in ascending group order: record p of the list
 * (p < min(*ready_count, ready_cap)) is written in every column —
 *   ready_gid, rd_flags           the group and its rflags;
 *   hs_term, hs_vote, hs_commit   the HardState with QB_RDF_HARD, else 0, 0, 0;
 *   ent_lo, ent_hi, ent_last_term with QB_RDF_ENTRIES, else 0, 0, 0;
 *   apply_lo, apply_hi            with QB_RDF_COMMITTED, else 0, 0;
 *   snap_index                    usnap_index with QB_RDF_SNAPSHOT, else 0;
 *   lead, role                    the SoftState (role without
 *                                 QB_ROLE_PROMOTABLE), always
 * — and no record at or past that count is touched.  *ready_count (device)
 * gets the number of ready groups, listed or not.  A ready group whose
 * position is >= ready_cap is deferred: rflags[g] |= QB_RDF_DEFERRED, no
 * record, nothing accepted; the next call finds it again.
 *
 * accept != 0 runs acceptReady (rawnode.go:139-147) on every listed group
 * without QB_RDF_BAD_LOG: with QB_RDF_SOFT prev_lead := lead and prev_role :=
 * role without QB_ROLE_PROMOTABLE; pending[g] := 0.  No other state is
 * written.  accept == 0 is HasReady + readyWithoutAccept: no state array is
 * written at all. */
#define QB_RDF_SOFT 0x0001u
#define QB_RDF_HARD 0x0002u
#define QB_RDF_ENTRIES 0x0004u
#define QB_RDF_SNAPSHOT 0x0008u
#define QB_RDF_COMMITTED 0x0010u
#define QB_RDF_MSGS 0x0020u
#define QB_RDF_READSTATES 0x0040u
#define QB_RDF_MUST_SYNC 0x0080u
#define QB_RDF_BAD_LOG 0x0100u
#define QB_RDF_DEFERRED 0x0200u

#define QB_RDP_MSGS 0x01u
#define QB_RDP_READSTATES 0x02u

#define QB_READY_MAX_GROUPS 0xFFFFFFFEull /* ready_gid is a uint32 */

enum {
  QB_RSTAT_SOFT = 0,        /* groups by flag, over all G groups */
  QB_RSTAT_HARD = 1,
  QB_RSTAT_ENTRIES = 2,
  QB_RSTAT_SNAPSHOT = 3,
  QB_RSTAT_COMMITTED = 4,
  QB_RSTAT_MSGS = 5,
  QB_RSTAT_READSTATES = 6,
  QB_RSTAT_MUST_SYNC = 7,
  QB_RSTAT_BAD_LOG = 8,
  QB_RSTAT_DEFERRED = 9,    /* ready groups past ready_cap */
  QB_RSTAT_LISTED = 10,     /* records written             */
  QB_RSTAT_COUNT = 11
};

/* term .. pending_conf_index are the step calls' buffers (same layouts: a
 * caller passes the same pointers) and are only read. */
typedef struct qb_ready_groups {
  uint64_t G;                         /* <= QB_READY_MAX_GROUPS */
  const uint64_t* term;               /* [G] */
  const uint64_t* vote;               /* [G] */
  const uint64_t* committed;          /* [G] */
  const uint64_t* lead;               /* [G] */
  const uint8_t* role;                /* [G] QB_ROLE_* */
  const uint64_t* first_index;        /* [G] */
  const uint64_t* last_index;         /* [G] */
  const uint64_t* last_term;          /* [G] */
  const uint32_t* meta;               /* [G] bits 16-19: term runs (advance) */
  const uint64_t* run_start;          /* [QB_LEADER_MAX_RUNS * G] run-major (advance) */
  const uint64_t* run_term;           /* same layout */
  const uint64_t* pending_conf_index; /* [G] (advance) */
  const uint32_t* ext;                /* [G] nullable; bit 16: AutoLeave, as qb_dev_conf_change (advance) */
  uint64_t* applied;                  /* [G] in/out: advance */
  uint64_t* unstable_offset;          /* [G] in/out: advance, qb_dev_unstable_truncate */
  uint64_t* usnap_index;              /* [G] in/out: advance */
  uint64_t* usnap_term;               /* [G] in/out: advance */
  uint64_t* prev_term;                /* [G] in/out: advance */
  uint64_t* prev_vote;                /* [G] in/out: advance */
  uint64_t* prev_commit;              /* [G] in/out: advance */
  uint64_t* prev_lead;                /* [G] in/out: ready with accept */
  uint8_t* prev_role;                 /* [G] in/out: ready with accept */
  uint8_t* pending;                   /* [G] in/out: QB_RDP_*; ready with accept */
  uint64_t* uncommitted_size;         /* [G] in/out: advance */
} qb_ready_groups;

typedef struct qb_ready_out {
  uint16_t* rflags;        /* [G] QB_RDF_*, written for every group */
  /* the list, [ready_cap] each */
  uint32_t* ready_gid;
  uint16_t* rd_flags;
  uint64_t* hs_term;
  uint64_t* hs_vote;
  uint64_t* hs_commit;
  uint64_t* ent_lo;
  uint64_t* ent_hi;
  uint64_t* ent_last_term;
  uint64_t* apply_lo;
  uint64_t* apply_hi;
  uint64_t* snap_index;
  uint64_t* lead;
  uint8_t* role;
  uint64_t* ready_count;   /* device, one */
} qb_ready_out;

/* stats: QB_RSTAT_COUNT device uint64 (accumulated).  Every pointer but ext
 * is required (the list's columns too with ready_cap == 0: pass any valid
 * pointer); run_start, run_term, meta, pending_conf_index and
 * uncommitted_size are not read by qb_dev_ready.  G == 0 is QB_OK and sets
 * *ready_count = 0; G > QB_READY_MAX_GROUPS or a workspace below
 * qb_ready_scratch_bytes(G) is QB_EINVAL.  No allocation inside the call
 * (it can be graph-captured); nothing outside the caller's arrays is read or
 * written, whatever they hold. */
size_t qb_ready_scratch_bytes(uint64_t G);
int qb_dev_ready(const qb_ready_groups* rg, int accept, uint64_t ready_cap,
                 const qb_ready_out* out, uint64_t* stats, void* workspace,
                 size_t workspace_bytes, void* stream);

/* RawNode.Advance (rawnode.go:172-179) -> raft.advance (raft.go:543-580) for
 * the A groups the host finished, one dense record each.  adv_gid values are
 * distinct (two records of one group race); the Ready list's ascending order
 * is the fast case and is not required.  A record whose adv_gid >= G gets
 * QB_AFLAG_BAD_GROUP and is dropped.  Per record, in Go's order:
 *   0. appliedTo's panic (log.go:246-254), found before anything of the
 *      record is applied: applied_to != 0 and (committed < applied_to or
 *      applied_to < applied) is QB_AFLAG_APPLIED_RANGE and nothing below runs.
 *   1. (hs_term, hs_vote, hs_commit) not all zero: prev_term / prev_vote /
 *      prev_commit := it (rawnode.go:174-177).  The host passes the Ready's
 *      hs_* columns back.
 *   2. reduceUncommittedSize (raft.go:1783-1801) by applied_payload, the sum
 *      of PayloadSize over the entries handed to the application: nothing at
 *      uncommitted_size == 0, else uncommitted_size -= applied_payload,
 *      saturating at 0.
 *   3. applied_to != 0 (appliedCursor, node.go:112-123: the last index handed
 *      to the application — apply_hi, or less after the host paginated — or
 *      the snapshot's index): applied := applied_to.  With AutoLeave (ext bit
 *      16), oldApplied <= pending_conf_index <= applied_to and a leader's
 *      role: QB_AFLAG_AUTO_LEAVE — the empty ConfChangeV2 append and the new
 *      pending_conf_index stay the host's.
 *   4. stable_index != 0: stableTo(stable_index, stable_term) (log.go:256,
 *      log_unstable.go:77-89) against the log as it is now — it may have been
 *      truncated since the Ready.  unstable_offset := stable_index + 1 iff
 *      unstable_offset <= stable_index <= last_index and the term of
 *      stable_index (last_term at last_index, else the run table, 0 below
 *      first_index - 1) equals stable_term; else QB_AFLAG_STABLE_STALE and
 *      the offset stays: the next Ready lists the entries again.
 *   5. stable_snap != 0: stableSnapTo (log_unstable.go:109-113): usnap_index
 *      := 0 and usnap_term := 0 iff usnap_index == stable_snap.
 * aflags[i] is written for every record; nothing else is written but the
 * state named above. */
#define QB_AFLAG_APPLIED_RANGE 0x01u /* appliedTo would panic: nothing applied */
#define QB_AFLAG_AUTO_LEAVE 0x02u    /* the host proposes the empty ConfChangeV2 */
#define QB_AFLAG_STABLE_STALE 0x04u  /* stableTo matched nothing */
#define QB_AFLAG_BAD_GROUP 0x08u     /* adv_gid >= G: dropped */

enum {
  QB_ASTAT_HARDSTATE = 0,     /* prevHardSt replaced            */
  QB_ASTAT_APPLIED = 1,       /* applied moved (or re-set)      */
  QB_ASTAT_AUTO_LEAVE = 2,
  QB_ASTAT_STABLE = 3,        /* unstable_offset moved          */
  QB_ASTAT_STABLE_STALE = 4,
  QB_ASTAT_SNAP_STABLE = 5,   /* the pending snapshot cleared   */
  QB_ASTAT_APPLIED_RANGE = 6,
  QB_ASTAT_BAD_GROUP = 7,
  QB_ASTAT_COUNT = 8
};

typedef struct qb_advance_in {  /* all [A] */
  const uint32_t* adv_gid;
  const uint64_t* hs_term;         /* all three 0: an empty HardState */
  const uint64_t* hs_vote;
  const uint64_t* hs_commit;
  const uint64_t* applied_to;      /* 0 = none */
  const uint64_t* applied_payload;
  const uint64_t* stable_index;    /* 0 = none */
  const uint64_t* stable_term;
  const uint64_t* stable_snap;     /* 0 = none */
} qb_advance_in;

/* stats: QB_ASTAT_COUNT device uint64 (accumulated).  A == 0 is QB_OK and
 * writes nothing; every pointer of rg but ext is required.  No workspace, no
 * allocation (it can be graph-captured). */
int qb_dev_advance(const qb_ready_groups* rg, uint64_t A, const qb_advance_in* in,
                   uint8_t* aflags, uint64_t* stats, void* stream);

/* What qb_dev_follower_log_step leaves to the host for unstable_offset:
 * unstable.truncateAndAppend (log_unstable.go:121-145) sets, in each of its
 * three cases, offset := min(offset, index of the first appended entry).
 * For every record i < M with app_from[i] != 0 and group[i] < G:
 * unstable_offset[group[i]] := min(unstable_offset[group[i]], app_from[i]), a
 * 64-bit atomic min, so the records' order does not matter.  group and
 * app_from are the log step's rec_group column and app_from output.  M == 0
 * is QB_OK. */
int qb_dev_unstable_truncate(uint64_t M, const uint32_t* group, const uint64_t* app_from,
                             uint64_t G, uint64_t* unstable_offset, void* stream);

/* ----------------------------------------------------------------------- */
/* Follower snapshot: MsgSnap, handleSnapshot, restore                     */
/* ----------------------------------------------------------------------- */

/* raft.Step (raft.go:847-984) for MsgSnap at nodes that are not leading, for
 * R records in one call: the receiving side of the QB_MSG_SNAP that
 * qb_dev_leader_step, qb_dev_leader_propose and qb_dev_leader_requests emit,
 * and the writer of the unstable snapshot that qb_dev_ready lists
 * (QB_RDF_SNAPSHOT) and qb_dev_advance clears (stableSnapTo).  A record is one
 * MsgSnap; the records of one call name distinct groups, as qb_dev_advance's
 * do (two records of one group race): a second snapshot for a group waits for
 * the next call.  The snapshot's data stays the host's; the call decides what
 * the node does with it, moves the log's cursors and writes the response.
 *
 * The arrays are the step calls' own (same layouts: a caller passes the same
 * buffers): qb_follower_groups, qb_follower_log, self_id of
 * qb_campaign_groups, and unstable_offset / usnap_index / usnap_term / pending
 * of qb_ready_groups.  This is the one call that writes first_index.
 *
 * A record: from / term = Message.From / Message.Term, snap_index / snap_term
 * = Snapshot.Metadata.Index / Term, and Snapshot.Metadata.ConfState as the IDs
 * cs_id[cs_off[i] .. cs_off[i + 1]) with cs_set[k] naming the list that holds
 * ID k (QB_CS_*; any other value is in no list).  Offsets above C read as C.
 *
 * Per record, in Go's order:
 *   Bad group: group >= G is QB_SNF_BAD_GROUP; nothing else happens.
 *   Term filter (raft.go:849-920), with Term != 0 (0 skips it, as for any
 *     message with Term 0):
 *     higher term: becomeFollower(m.Term, m.From) (raft.go:876-877) -> reset
 *       (raft.go:686-693, 590-619), restricted to the fields this call owns,
 *       exactly as qb_dev_follower_step states it: term (and vote := 0) change
 *       only if the term differs, lead is set, both counters 0, role :=
 *       Follower with the other bits of the byte kept, QB_SNF_RESET;
 *     lower term: ignored whatever check_quorum / pre_vote say — those
 *       branches name MsgApp, MsgHeartbeat and MsgPreVote only (raft.go:884,
 *       907).  QB_SNF_STALE, no response, nothing written.
 *   By role at or above the term: a leader ignores it (stepLeader has no case
 *     for it): QB_SNF_ROLE_IGNORED, no response, nothing written.  A
 *     (pre-)candidate runs becomeFollower(m.Term, m.From) (raft.go:1396-1398;
 *     QB_SNF_RESET), a follower sets election_elapsed = 0 and lead = From
 *     (raft.go:1441-1444).
 *   handleSnapshot -> restore (raft.go:1518-1614):
 *     1. snap_index <= committed (raft.go:1535-1537): QB_SNF_OLD,
 *        MsgAppResp{Index: committed}.
 *     2. self_id[g] is in none of Voters / Learners / VotersOutgoing
 *        (raft.go:1554-1580; LearnersNext does not count): QB_SNF_NOT_MEMBER,
 *        MsgAppResp{Index: committed}.
 *     3. matchTerm(snap_index, snap_term) (raft.go:1584-1589, log.go:320-326),
 *        the term of snap_index being last_term at last_index, the run
 *        table's inside the log and 0 outside [first_index - 1, last_index]
 *        (log.go:268-274): commitTo(snap_index), i.e. committed := snap_index;
 *        QB_SNF_FAST_FORWARD, MsgAppResp{Index: committed}.
 *     4. Else raftLog.restore + unstable.restore (log.go:336-340,
 *        log_unstable.go:115-119): committed := snap_index, unstable_offset :=
 *        snap_index + 1, usnap_index := snap_index, usnap_term := snap_term,
 *        last_index := snap_index, last_term := snap_term, first_index :=
 *        snap_index + 1 (maybeFirstIndex, log_unstable.go:35-40), the run
 *        table one run (snap_index, snap_term) with the count in meta bits
 *        16-19 set to 1 — rows 1..7 of the table keep what they hold — and
 *        QB_ROLE_PROMOTABLE cleared: promotable() is false while a snapshot
 *        is pending (raft.go:1618-1621; TestRestore: "It should not campaign
 *        before actually applying data").  QB_SNF_RESTORED,
 *        MsgAppResp{Index: last_index}.
 *     The r.state != StateFollower branch of restore (raft.go:1538-1549) is
 *     unreachable: both callers have made the node a follower.  It is not
 *     modelled.
 *   Stop, QB_SNF_COMMIT_RANGE: the one state Go panics on.  A record that
 *     reaches step 3 with snap_index > last_index matches exactly when
 *     snap_term == 0 (term() is 0 outside the log), and commitTo then panics
 *     (log.go:239-241).  It is found before anything of the record is
 *     applied, the term filter's effect included, as the log step's stops
 *     are: this flag alone, no response, nothing written.
 *   Response: resp_type = QB_FRESP_APP_RESP or 0 (none), resp_term = term[g]
 *     behind the filter (as send stamps it), resp_index; To = from[i].  With
 *     pending != NULL a record with a response ORs QB_RDP_MSGS into
 *     pending[g].
 *   QB_SNF_HARDSTATE: term, vote or committed differ from their values at
 *     entry — what Ready persists before the response may be sent.
 * Index arithmetic wraps as Go's uint64 does.
 *
 * What stays the host's behind QB_SNF_RESTORED: the
 * ProgressTracker reset and confchange.Restore of the record's ConfState
 * (raft.go:1593-1606: the qb_dev_conf_change sequence with LastIndex =
 * snap_index), the own slot's MaybeUpdate(Next - 1) (raft.go:1608-1609), and
 * setting QB_ROLE_PROMOTABLE again once the snapshot is stable and the config
 * is in; behind QB_SNF_RESET the rest of reset, as for the follower step. */
#define QB_CS_VOTERS 0          /* ConfState.Voters         */
#define QB_CS_LEARNERS 1        /* ConfState.Learners       */
#define QB_CS_VOTERS_OUTGOING 2 /* ConfState.VotersOutgoing */
#define QB_CS_LEARNERS_NEXT 3   /* ConfState.LearnersNext   */

#define QB_SNF_RESTORED 0x0001u     /* the log is the snapshot now             */
#define QB_SNF_FAST_FORWARD 0x0002u /* the log held it: committed moved        */
#define QB_SNF_OLD 0x0004u          /* snap_index <= committed                 */
#define QB_SNF_NOT_MEMBER 0x0008u   /* the node is not in the ConfState        */
#define QB_SNF_STALE 0x0010u        /* lower term: ignored                     */
#define QB_SNF_ROLE_IGNORED 0x0020u /* a leader: ignored                       */
#define QB_SNF_RESET 0x0040u        /* becomeFollower ran: the host's reset    */
#define QB_SNF_COMMIT_RANGE 0x0080u /* stopped: commitTo would panic           */
#define QB_SNF_BAD_GROUP 0x0100u    /* group >= G: dropped                     */
#define QB_SNF_HARDSTATE 0x0200u    /* term / vote / committed changed         */

enum {
  QB_SSTAT_RESTORED = 0,        /* records by flag: the first nine bits */
  QB_SSTAT_FAST_FORWARD = 1,
  QB_SSTAT_OLD = 2,
  QB_SSTAT_NOT_MEMBER = 3,
  QB_SSTAT_STALE = 4,
  QB_SSTAT_ROLE_IGNORED = 5,
  QB_SSTAT_BECAME_FOLLOWER = 6, /* becomeFollower calls (QB_SNF_RESET)  */
  QB_SSTAT_COMMIT_RANGE = 7,
  QB_SSTAT_BAD_GROUP = 8,
  QB_SSTAT_COUNT = 9
};

typedef struct qb_snapshot_groups {
  uint64_t G;                   /* <= QB_READY_MAX_GROUPS                       */
  uint32_t election_timeout;    /* as qb_follower_groups; not read by MsgSnap   */
  uint32_t check_quorum;        /* same                                         */
  uint32_t pre_vote;            /* same                                         */
  uint32_t reserved;            /* 0                                            */
  const uint64_t* self_id;      /* [G] the node's raft ID                       */
  uint64_t* term;               /* [G] in/out */
  uint64_t* vote;               /* [G] in/out */
  uint64_t* lead;               /* [G] in/out */
  uint64_t* committed;          /* [G] in/out */
  uint8_t* role;                /* [G] in/out: QB_ROLE_*                        */
  uint32_t* election_elapsed;   /* [G] in/out */
  uint32_t* heartbeat_elapsed;  /* [G] in/out */
  uint64_t* first_index;        /* [G] in/out */
  uint64_t* last_index;         /* [G] in/out */
  uint64_t* last_term;          /* [G] in/out */
  uint32_t* meta;               /* [G] in/out: only bits 16-19 (term runs) may change */
  uint64_t* run_start;          /* [QB_LEADER_MAX_RUNS * G] run-major, in/out: row 0 only */
  uint64_t* run_term;           /* same layout */
  uint64_t* unstable_offset;    /* [G] in/out */
  uint64_t* usnap_index;        /* [G] in/out */
  uint64_t* usnap_term;         /* [G] in/out */
  uint8_t* pending;             /* [G] in/out: QB_RDP_*; nullable               */
} qb_snapshot_groups;

typedef struct qb_snapshot_inbox {
  uint64_t R;                 /* <= 2^32 - 2                                    */
  const uint32_t* group;      /* [R] distinct                                   */
  const uint64_t* from;       /* [R] sender ID                                  */
  const uint64_t* term;       /* [R] Message.Term; 0 skips the term filter      */
  const uint64_t* snap_index; /* [R] Snapshot.Metadata.Index                    */
  const uint64_t* snap_term;  /* [R] Snapshot.Metadata.Term                     */
  const uint32_t* cs_off;     /* [R+1] record i's ConfState IDs: cs_off[i] ..
                                 cs_off[i+1]; offsets above C read as C         */
  const uint64_t* cs_id;      /* [C] the ConfState's IDs                        */
  const uint8_t* cs_set;      /* [C] QB_CS_*: the list the ID is in             */
  uint64_t C;
} qb_snapshot_inbox;

typedef struct qb_snapshot_out { /* all [R], written for every record */
  uint16_t* sflags;     /* QB_SNF_*                                  */
  uint8_t* resp_type;   /* 0 or QB_FRESP_APP_RESP                    */
  uint64_t* resp_term;  /* Message.Term of the response (0 if none)  */
  uint64_t* resp_index; /* Message.Index of the response (0 if none) */
} qb_snapshot_out;

/* stats: QB_SSTAT_COUNT device uint64 (accumulated).  R == 0 or G == 0 is
 * QB_OK and writes nothing.  Every pointer but pending is required (cs_id and
 * cs_set only with C > 0); a NULL struct, G > QB_READY_MAX_GROUPS or R > 2^32
 * - 2 is QB_EINVAL.  No workspace and no allocation inside the call (it can be
 * graph-captured); nothing outside the caller's arrays is read or written,
 * whatever they hold. */
int qb_dev_follower_snapshot(const qb_snapshot_groups* sg, const qb_snapshot_inbox* in,
                             const qb_snapshot_out* out, uint64_t* stats, void* stream);

/* ----------------------------------------------------------------------- */
/* Log compaction: CreateSnapshot, Compact and etcdserver's trigger        */
/* ----------------------------------------------------------------------- */

/* MemoryStorage.CreateSnapshot and Compact (storage.go:190-236) and
 * etcdserver's policy around them (server/etcdserver/server.go:1096-1117
 * triggerSnapshot / shouldSnapshot, 1993-2067 snapshot()) for G groups in one
 * call: what the host runs behind QB_FFLAG_LOG_RUNS and QB_PFLAG_LOG_RUNS, and
 * the one call that moves snap_index / snap_term and advances first_index on
 * the node's own account.  The snapshot's data, the WAL and the entries' bytes
 * stay the host's; the call decides, moves the cursors, shifts the term-run
 * table and lists the groups that changed.
 *
 * The arrays are the other calls' own (same layouts: a caller passes the same
 * buffers): first_index / meta / run_start / run_term of qb_follower_log and
 * qb_leader_groups, snap_index / snap_term of qb_leader_groups, and applied /
 * unstable_offset / usnap_index of qb_ready_groups.
 *
 * THE REQUEST, by qb_compact_in::mode.
 *   QB_CM_EXPLICIT: two independent Storage calls per group, the snapshot
 *     first: snap_at[g] = CreateSnapshot's i, compact_at[g] = Compact's
 *     compactIndex, 0 = none; a NULL column is a column of zeros.
 *   QB_CM_TRIGGER: with snapi = snap_index[g] and appl = applied[g], a group
 *     triggers iff (force[g] && appl != snapi) || (appl - snapi >
 *     snapshot_count), the subtraction wrapping as Go's uint64 does
 *     (shouldSnapshot, server.go:1115-1117; force is forceSnapshot).  A
 *     triggering group snapshots at appl (server.go:1111), then compacts at
 *     appl > catch_up_entries ? appl - catch_up_entries : 1
 *     (server.go:2047-2053).  With hold[g] != 0 (inflightSnapshots != 0,
 *     server.go:2042-2045) the compaction is skipped behind a snapshot that
 *     succeeded: QB_CMF_HELD.  A snapshot that does not succeed, for any
 *     reason, cancels the compaction (snapshot()'s early return,
 *     server.go:2016-2023).  NULL force / hold are columns of zeros.
 *
 * PER GROUP, in this order, with off = first_index - 1 (ms.ents[0].Index) and
 * stable_last = unstable_offset - 1 (ms.lastIndex(): MemoryStorage holds the
 * stable entries only):
 *   1. No request: cmflags[g] = 0; nothing of the group but the request
 *      columns is read.
 *   2. first_index == 0, stable_last < off or stable_last > last_index:
 *      QB_CMF_BAD_LOG, nothing applied.
 *   3. usnap_index != 0: QB_CMF_PENDING_SNAPSHOT, nothing applied.  A restored
 *      snapshot has not reached storage yet; the reference's Ready loop
 *      applies it before triggerSnapshot can run (applyAll,
 *      server.go:903-915).
 *   4. Snapshot at s (CreateSnapshot, storage.go:194-213):
 *        s <= snap_index: QB_CMF_SNAP_OUT_OF_DATE (ErrSnapOutOfDate,
 *          storage.go:197-199);
 *        s > stable_last or s < off: QB_CMF_OUT_OF_BOUND (Go panics:
 *          storage.go:202-204, or the slice index of storage.go:207);
 *        s > applied: QB_CMF_PAST_APPLIED.  An engine rule: a snapshot is the
 *          applied state, and etcd only ever passes appliedi;
 *        else QB_CMF_SNAPPED: snap_index := s, snap_term := term(s) — the term
 *          of the last run of the table whose start is <= s, run 0 taken to
 *          start at off.
 *   5. Compact at c (Compact, storage.go:218-236):
 *        c <= off: QB_CMF_ALREADY_COMPACTED (ErrCompacted, storage.go:222-224);
 *        c > stable_last: QB_CMF_OUT_OF_BOUND (storage.go:225-227);
 *        c > applied: QB_CMF_PAST_APPLIED.  storage.go:216-217 leaves this to
 *          the application; the table's invariant first_index - 1 <= committed
 *          needs it;
 *        else QB_CMF_COMPACTED.  With n runs (meta bits 16-19; 0 is read as 1,
 *          above QB_LEADER_MAX_RUNS as that) and k the last run whose start is
 *          <= c (run 0 taken to start at off): new row 0 is (c, run_term[k]),
 *          new row j is old row k + j for 0 < j < n - k, rows at or above
 *          n - k keep what they hold, meta bits 16-19 := n - k, first_index :=
 *          c + 1.  The entry at c becomes the dummy entry, as ents[0] does.
 *   6. QB_CMF_OUT_OF_BOUND or QB_CMF_PAST_APPLIED from either half: the group
 *      is not changed at all (Go would not have returned) and carries neither
 *      QB_CMF_SNAPPED nor QB_CMF_COMPACTED.  QB_CMF_SNAP_OUT_OF_DATE and
 *      QB_CMF_ALREADY_COMPACTED are plain errors: in explicit mode the other
 *      half still runs.
 * Both halves are decided against the state at entry (the snapshot reads the
 * table before the compaction shifts it).  Index arithmetic wraps as Go's
 * uint64 does.
 *
 * OUTPUTS.  cmflags[g] is written for every group.  The groups with
 * QB_CMF_SNAPPED or QB_CMF_COMPACTED are listed in ascending group order:
 * record p (p < min(*list_count, list_cap)) is written in every column —
 *   gid, flags        the group and its cmflags;
 *   snap_index, snap_term   the group's snapshot after the call;
 *   compact_index     c with QB_CMF_COMPACTED, else 0;
 *   first_before      first_index at entry
 * — and no record at or past that count is touched.  It is the host's work
 * list: save the snapshot and release the WAL behind
 * QB_CMF_SNAPPED, drop the entries below compact_index + 1 behind
 * QB_CMF_COMPACTED.  *list_count (device) gets the number of such groups,
 * listed or not.  A group whose position is >= list_cap is deferred:
 * cmflags[g] |= QB_CMF_DEFERRED, no record, nothing of it applied; the next
 * call finds it again. */
#define QB_CM_EXPLICIT 0
#define QB_CM_TRIGGER 1

#define QB_CMF_SNAPPED 0x0001u           /* snap_index / snap_term moved          */
#define QB_CMF_COMPACTED 0x0002u         /* first_index and the table moved       */
#define QB_CMF_SNAP_OUT_OF_DATE 0x0004u  /* ErrSnapOutOfDate                      */
#define QB_CMF_ALREADY_COMPACTED 0x0008u /* ErrCompacted                          */
#define QB_CMF_OUT_OF_BOUND 0x0010u      /* stopped: Go panics; nothing applied   */
#define QB_CMF_PAST_APPLIED 0x0020u      /* stopped: index > applied              */
#define QB_CMF_HELD 0x0040u              /* trigger: compaction skipped by hold   */
#define QB_CMF_PENDING_SNAPSHOT 0x0080u  /* usnap_index != 0: nothing applied     */
#define QB_CMF_BAD_LOG 0x0100u           /* the cursors contradict each other     */
#define QB_CMF_DEFERRED 0x0200u          /* past list_cap: nothing applied        */

enum {
  QB_CMSTAT_SNAPPED = 0,          /* groups by flag, over all G groups, deferred ones included */
  QB_CMSTAT_COMPACTED = 1,
  QB_CMSTAT_SNAP_OUT_OF_DATE = 2,
  QB_CMSTAT_ALREADY_COMPACTED = 3,
  QB_CMSTAT_OUT_OF_BOUND = 4,
  QB_CMSTAT_PAST_APPLIED = 5,
  QB_CMSTAT_HELD = 6,
  QB_CMSTAT_PENDING_SNAPSHOT = 7,
  QB_CMSTAT_BAD_LOG = 8,
  QB_CMSTAT_DEFERRED = 9,
  QB_CMSTAT_LISTED = 10,          /* records written                                  */
  QB_CMSTAT_ENTRIES_DROPPED = 11, /* sum of c - off over the compactions applied      */
  QB_CMSTAT_RUNS_DROPPED = 12,    /* sum of k over the compactions applied            */
  QB_CMSTAT_COUNT = 13
};

typedef struct qb_compact_groups {
  uint64_t G;                      /* <= QB_READY_MAX_GROUPS                          */
  uint64_t* first_index;           /* [G] in/out                                      */
  uint64_t* snap_index;            /* [G] in/out: qb_leader_groups::snap_index        */
  uint64_t* snap_term;             /* [G] in/out                                      */
  uint32_t* meta;                  /* [G] in/out: only bits 16-19 (term runs) may change */
  uint64_t* run_start;             /* [QB_LEADER_MAX_RUNS * G] run-major, in/out      */
  uint64_t* run_term;              /* same layout                                     */
  const uint64_t* last_index;      /* [G]                                             */
  const uint64_t* applied;         /* [G] qb_ready_groups::applied                    */
  const uint64_t* unstable_offset; /* [G] qb_ready_groups::unstable_offset            */
  const uint64_t* usnap_index;     /* [G] qb_ready_groups::usnap_index                */
} qb_compact_groups;

typedef struct qb_compact_in {
  uint32_t mode;               /* QB_CM_EXPLICIT / QB_CM_TRIGGER                      */
  uint32_t reserved;           /* 0                                                   */
  const uint64_t* snap_at;     /* [G] explicit: CreateSnapshot(i), 0 = none; nullable */
  const uint64_t* compact_at;  /* [G] explicit: Compact(i), 0 = none; nullable        */
  uint64_t snapshot_count;     /* trigger: Cfg.SnapshotCount                          */
  uint64_t catch_up_entries;   /* trigger: Cfg.SnapshotCatchUpEntries                 */
  const uint8_t* force;        /* [G] trigger: forceSnapshot; nullable                */
  const uint8_t* hold;         /* [G] trigger: inflightSnapshots != 0; nullable       */
} qb_compact_in;

typedef struct qb_compact_out {
  uint16_t* cmflags;       /* [G] QB_CMF_*, written for every group */
  /* the list, [list_cap] each */
  uint32_t* gid;
  uint16_t* flags;
  uint64_t* snap_index;
  uint64_t* snap_term;
  uint64_t* compact_index;
  uint64_t* first_before;
  uint64_t* list_count;    /* device, one */
} qb_compact_out;

/* stats: QB_CMSTAT_COUNT device uint64 (accumulated).  Every pointer is
 * required but the four request columns (the list's columns too with list_cap
 * == 0: pass any valid pointer); the columns of the mode not chosen are not
 * read.  G == 0 is QB_OK and sets *list_count = 0.  A NULL struct, a mode
 * other than the two, G > QB_READY_MAX_GROUPS (gid is a uint32), a missing
 * pointer or a workspace below qb_log_compact_scratch_bytes(G) is QB_EINVAL,
 * found before any HIP call.  No allocation inside the call (it can be
 * graph-captured); nothing outside the caller's arrays is read or written,
 * whatever they hold.
 *
 * What stays the host's: the snapshot's data and ConfState,
 * SaveSnap and the WAL release, dropping the entries' bytes, clearing
 * forceSnapshot, and setting snap_index / snap_term once a restored snapshot
 * (qb_dev_follower_snapshot) has reached storage — ApplySnapshot
 * (storage.go:174-188) is not this call. */
size_t qb_log_compact_scratch_bytes(uint64_t G);
int qb_dev_log_compact(const qb_compact_groups* cg, const qb_compact_in* in, uint64_t list_cap,
                       const qb_compact_out* out, uint64_t* stats, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------------- */
/* Wire ingest                                       */
/* ----------------------------------------------------------------------- */

/* Raw protobuf-encoded raftpb.Message bytes (raft/raftpb/raft.proto:68-86)
 * -> leader-inbox records for qb_dev_leader_step.  Message i is
 * bytes[msg_off[i] .. msg_off[i+1]) and belongs to group msg_group[i] (the
 * multi-raft envelope's group).  Validation is exactly Message.Unmarshal
 * (raftpb/raft.pb.go:1739-2061, nested Entry / Snapshot / SnapshotMetadata /
 * ConfState bodies included, unknown fields skipped as skipRaft).  From is
 * mapped to its slot among the group's CSR slot IDs (ids[off[g] ..
 * off[g+1]), ascending); a non-member gets QB_REC_NO_PROGRESS.  MsgAppResp /
 * MsgHeartbeatResp / MsgSnapStatus / MsgUnreachable become records (a
 * heartbeat response's Context must be empty or an 8-byte non-zero
 * big-endian request id, which becomes rec_index); any other status leaves
 * rec_group = UINT32_MAX (dropped by the step as a bad group).
 * msg_type (nullable) receives the low byte of Message.Type;
 * stats (nullable, 4 device uint64, accumulated) counts each status.
 * A message whose slice is not inside the buffer (msg_off[i+1] < msg_off[i]
 * or msg_off[i+1] > nbytes: a caller error — Go would panic slicing it) gets
 * QB_WIRE_UNMARSHAL; nothing outside [bytes, bytes + nbytes) is read. */
#define QB_WIRE_OK 0
#define QB_WIRE_UNMARSHAL 1 /* Message.Unmarshal returns an error           */
#define QB_WIRE_TYPE 2      /* not a leader-inbox response type             */
#define QB_WIRE_CTX 3       /* Context neither empty nor an 8-byte id       */
int qb_dev_ingest_messages(uint64_t M, const uint8_t* bytes, uint64_t nbytes,
                           const uint64_t* msg_off, const uint32_t* msg_group,
                           uint64_t G, const uint32_t* off, const uint64_t* ids,
                           uint32_t* rec_group, uint8_t* rec_flags,
                           uint64_t* rec_index, uint64_t* rec_term,
                           uint64_t* rec_hint, uint64_t* rec_log_term,
                           uint8_t* status, uint8_t* msg_type, uint64_t* stats,
                           void* stream);
/* The same ingest over a 64-byte group-row table built once per config
 * (qb_dev_wire_group_rows: row g = member count | first slot << 32, then the
 * first 7 member IDs; 16-byte aligned, qb_wire_group_rows_bytes(G)).  Each
 * message then gathers one row instead of a row of off and one or two lines
 * of ids; members past the 7th are still read from ids.  Rebuild the rows
 * whenever off / ids change. */
size_t qb_wire_group_rows_bytes(uint64_t G);
int qb_dev_wire_group_rows(uint64_t G, const uint32_t* off, const uint64_t* ids,
                           uint64_t* rows, void* stream);
int qb_dev_ingest_messages_rows(uint64_t M, const uint8_t* bytes, uint64_t nbytes,
                                const uint64_t* msg_off, const uint32_t* msg_group,
                                uint64_t G, const uint64_t* rows, const uint64_t* ids,
                                uint32_t* rec_group, uint8_t* rec_flags,
                                uint64_t* rec_index, uint64_t* rec_term,
                                uint64_t* rec_hint, uint64_t* rec_log_term,
                                uint8_t* status, uint8_t* msg_type, uint64_t* stats,
                                void* stream);

/* The composed per-tick path in one call (round 6): a tick's M encoded
 * responses decoded and stepped into the FIXED ProgressTracker of G groups
 * with n voters, the commit advanced — what a multi-raft host runs per tick
 * between the transport (server/etcdserver/api/rafthttp/stream.go:466:
 * Message.Unmarshal, raft.pb.go:1739-2061) and Ready (node.go:564-568:
 * raft.Step -> stepLeader MsgAppResp -> maybeCommit, raft.go:847-921,
 * 1100-1109, 1237-1259, 585-588).  Replaces qb_dev_ingest_messages[_rows]
 * followed by qb_dev_fixed_tracker_step on its records, with the same
 * result, minus the decoded record columns between them: the decoder writes
 * the tracker step's level-1 buckets directly.
 *   bytes, nbytes, msg_off [M+1], msg_group [M]: as qb_dev_ingest_messages;
 *   rows (qb_dev_wire_group_rows, 16-byte aligned) or off [G+1] + ids: the
 *     groups' slot IDs (rows preferred; ids are also read for members past
 *     the row's 7);
 *   group_term .. advanced_out, stats: as qb_dev_fixed_tracker_step
 *     (stepdown_at[g] = the message index of the first higher-term response;
 *     entry rule as there);
 *   status [M] (required): QB_WIRE_* per message, as the ingest;
 *   wire_stats [4] (nullable): QB_WIRE_* counts added, as the ingest's stats.
 * A message that is not a decoded MsgAppResp steps nothing and counts as
 * QB_STAT_BAD_GROUP (the ingest gives it group ~0); a From that is not a
 * member of the group (QB_REC_NO_PROGRESS) counts as QB_STAT_NON_MEMBER.
 * Workspace: qb_wire_fixed_tracker_workspace_bytes(n, G, M) bytes (0: the
 * batch is too large for one call). */
size_t qb_wire_fixed_tracker_workspace_bytes(uint32_t n, uint64_t G, uint64_t M);
int qb_dev_ingest_fixed_tracker_step(uint32_t n, uint64_t G, uint64_t M, const uint8_t* bytes,
                                     uint64_t nbytes, const uint64_t* msg_off,
                                     const uint32_t* msg_group, const uint64_t* rows,
                                     const uint32_t* off, const uint64_t* ids,
                                     const uint64_t* group_term, const uint64_t* term_start,
                                     uint64_t* match, uint64_t* next, uint16_t* active,
                                     uint64_t* committed, uint32_t* stepdown_at,
                                     uint8_t* advanced_out, uint8_t* status,
                                     uint64_t* wire_stats, uint64_t* stats, void* workspace,
                                     size_t workspace_bytes, void* stream);
/* The same one-call tick for the CSR tracker (ragged / learner / joint
 * configs, qb_dev_csr_tracker_step's layout and arguments): off [G+1] are
 * both the tracker's slot offsets and the groups' slot-ID ranges (ids
 * ascending per group, required; rows, the 64-byte row table of (off, ids),
 * nullable).  Workspace: qb_wire_csr_tracker_workspace_bytes(G, max_slots, M). */
size_t qb_wire_csr_tracker_workspace_bytes(uint64_t G, uint32_t max_slots, uint64_t M);
int qb_dev_ingest_csr_tracker_step(uint64_t G, uint32_t max_slots, const uint32_t* off,
                                   const uint32_t* cfg, uint64_t M, const uint8_t* bytes,
                                   uint64_t nbytes, const uint64_t* msg_off,
                                   const uint32_t* msg_group, const uint64_t* rows,
                                   const uint64_t* ids, const uint64_t* group_term,
                                   const uint64_t* term_start, uint64_t* match, uint64_t* next,
                                   uint16_t* active, uint64_t* committed, uint32_t* stepdown_at,
                                   uint8_t* advanced_out, uint8_t* status, uint64_t* wire_stats,
                                   uint64_t* stats, void* workspace, size_t workspace_bytes,
                                   void* stream);

/* The follower's ingest: raw raftpb.Message bytes -> the inbox of
 * qb_dev_follower_step / qb_dev_follower_log_step, with no host pass between
 * them.  bytes, nbytes, msg_off [M+1], msg_group [M] and the validation
 * (Message.Unmarshal, raftpb/raft.pb.go:1739-2061, with Entry.Unmarshal
 * 1360-1500 and the nested Snapshot bodies; unknown fields as skipRaft
 * 2909-2988) are qb_dev_ingest_messages'.  raft.Step checks no membership
 * for the types a non-leader receives (raft.go:847-984, 939-956), so no
 * config is read: group[i] = msg_group[i] as given, and a group >= G stays
 * the step's QB_FSTAT_BAD_GROUP (G is not used otherwise).  Classification
 * goes by Message.Type as Go holds it, an int32 (the varint's low 32 bits):
 *
 *   does not unmarshal, or the slice is not inside the buffer:
 *     QB_WIRE_UNMARSHAL; group = UINT32_MAX, every other column 0 (the
 *     transport drops it before Step: rafthttp/stream.go:466).
 *   MsgHeartbeat (8), Context nil / empty or 8 bytes not all zero:
 *     QB_FIN_HEARTBEAT, index = Commit, aux = the big-endian id (0: none).
 *     Any other Context: QB_FIN_HOST, QB_WIRE_CTX.
 *   MsgVote (5) / MsgPreVote (17): QB_FIN_VOTE / QB_FIN_PREVOTE, index =
 *     Index, aux = LogTerm; QB_FREC_FORCE iff Context is exactly the 16 bytes
 *     "CampaignTransfer" (raft.go:854; any other context is not force).
 *   MsgTimeoutNow (14): QB_FIN_TIMEOUT_NOW; Context ignored (raft.go:1452).
 *   MsgApp (3): index = Index, aux = LogTerm, commit = Commit, ent_n = the
 *     number of field-7 fields, whatever the status.  Where those fields are
 *     one contiguous byte range (or there are none) and their Entry.Index
 *     are Index + 1, Index + 2, ... (uint64 wrap): QB_FIN_APP, with ent_pos /
 *     ent_bytes = that range inside bytes (0 / 0 without entries) and the
 *     entries run-length encoded by Entry.Term in ent_term / ent_len[ent_off[i]
 *     .. ent_off[i+1]), adjacent runs differing (a Term of 0 is passed on: the
 *     log step has a rule for it; more than QB_LEADER_MAX_RUNS runs are legal
 *     here).  Otherwise — a gap, a repeated or out-of-order Index, another
 *     field between two entries — QB_FIN_HOST, QB_WIRE_ENTRIES, no runs,
 *     ent_pos = ent_bytes = 0.  A message whose runs end past ent_cap:
 *     QB_FIN_HOST, QB_WIRE_NO_SPACE, none of its runs written (ent_pos /
 *     ent_bytes stay); ent_off is monotone, so the messages that fit are a
 *     prefix, as with the encoder's cap.
 *   every other type (MsgSnap, MsgProp, the response, read, transfer and
 *     local types, values above 18): QB_FIN_HOST, QB_WIRE_TYPE.
 * Every QB_FIN_HOST record keeps group, from and term (index, aux and commit
 * are 0 unless it is a MsgApp), so the follower step stops the group there in
 * batch order.  term is Message.Term as sent (0: a local message, as Step
 * reads it).  Snapshot, Reject, RejectHint and To on these types are
 * validated and otherwise ignored, as Step ignores them.  commit is 0 for
 * every type but MsgApp; ent_pos / ent_bytes / ent_n are 0 for every other
 * type too.
 *
 * ent_off [M+1] is complete for every message (empty ranges for all but
 * QB_FIN_APP records, and for those downgraded to QB_WIRE_NO_SPACE the range
 * they would have had) and *ent_total = ent_off[M] is what the batch needs,
 * whatever ent_cap is, so a caller can size a retry.  With these columns
 * qb_follower_inbox = {M, group, flags, from, term, index, aux} and
 * qb_follower_app_inbox = {commit, ent_off, ent_term, ent_len, E = ent_cap}.
 * The host persists the entries it takes from bytes[ent_pos[i] .. ent_pos[i]
 * + ent_bytes[i]) (one 3a-keyed field each: the mirror of the encoder's
 * ent_at).  stats (nullable, QB_WIRE_FOLLOWER_STATUS_COUNT device uint64,
 * accumulated) counts each final status.
 *
 * qb_wire_follower_scratch_bytes(M) (the workspace's size, named as the
 * encoder's is) is 0 for M > 2^32 - 2 (the follower steps' bound, and M + 1
 * offsets of the 32-bit scan).  A NULL out, ent_off,
 * ent_total; with M > 0 a NULL msg_off, msg_group, required column (group,
 * flags, from, term, index, aux, commit, status), bytes with nbytes > 0,
 * ent_term / ent_len with ent_cap > 0; a short workspace, such an M, or
 * nbytes >= 2^32 (an entry takes two bytes at least, so below that the run
 * total fits the 32-bit scan and ent_bytes its column; split the batch) is
 * QB_EINVAL before any launch.  M == 0 is QB_OK with ent_off[0] = 0 and
 * *ent_total = 0 written.  No allocation inside the call (it can be
 * graph-captured); nothing outside [bytes, bytes + nbytes) is read and
 * nothing outside the caller's arrays written. */
#define QB_WIRE_ENTRIES 4  /* MsgApp whose entries the device does not take  */
#define QB_WIRE_NO_SPACE 5 /* MsgApp whose runs end past ent_cap             */
#define QB_WIRE_FOLLOWER_STATUS_COUNT 6

typedef struct qb_follower_wire_out {
  uint32_t* group;      /* [M] qb_follower_inbox's six columns                */
  uint8_t* flags;       /* [M] QB_FIN_* | QB_FREC_FORCE                       */
  uint64_t* from;       /* [M] */
  uint64_t* term;       /* [M] */
  uint64_t* index;      /* [M] */
  uint64_t* aux;        /* [M] */
  uint64_t* commit;     /* [M] qb_follower_app_inbox.commit                   */
  uint8_t* status;      /* [M] QB_WIRE_*                                      */
  uint8_t* msg_type;    /* [M] nullable: the low byte of Message.Type         */
  uint64_t* ent_pos;    /* [M] nullable                                       */
  uint32_t* ent_bytes;  /* [M] nullable                                       */
  uint32_t* ent_n;      /* [M] nullable: the entry count                      */
  uint32_t* ent_off;    /* [M+1]                                              */
  uint64_t* ent_term;   /* [ent_cap]                                          */
  uint32_t* ent_len;    /* [ent_cap]                                          */
  uint64_t ent_cap;
  uint64_t* ent_total;  /* device uint64                                      */
  uint64_t* stats;      /* nullable: [QB_WIRE_FOLLOWER_STATUS_COUNT]          */
} qb_follower_wire_out;

size_t qb_wire_follower_scratch_bytes(uint64_t M);
int qb_dev_ingest_follower(uint64_t M, const uint8_t* bytes, uint64_t nbytes,
                           const uint64_t* msg_off, const uint32_t* msg_group, uint64_t G,
                           const qb_follower_wire_out* out, void* workspace,
                           size_t workspace_bytes, void* stream);

/* The requests' ingest: raw raftpb.Message bytes -> the dense inputs of
 * qb_dev_leader_requests (qb_request_in) and qb_dev_leader_propose
 * (qb_propose_in), with no host pass between them.  These are the messages a
 * leader receives for its followers' clients — a forwarded MsgProp
 * (raft.go:1423-1433), MsgReadIndex and MsgTransferLeader (raft.go:1458-1470) —
 * and the MsgReadIndexResp a follower gets back.  bytes, nbytes, msg_off
 * [M+1], msg_group [M], off [G+1], ids and the validation (Message.Unmarshal,
 * raftpb/raft.pb.go:1739-2061, Entry.Unmarshal 1360-1500, skipRaft) are
 * qb_dev_ingest_messages'.  Classification goes by Message.Type as Go holds
 * it, an int32 (the varint's low 32 bits).
 *
 * Pass 1, per message i: kind[i], status[i], group[i] = msg_group[i], from[i],
 * term[i] (as sent) and msg_type[i] (the low byte), plus the kind's own
 * columns; every column a kind does not name is 0.
 *   does not unmarshal, or the slice is not inside the buffer:
 *     QB_WIRE_UNMARSHAL, QB_RQ_NONE; group = UINT32_MAX, every other column 0.
 *   MsgProp (2): QB_RQ_PROP.  ent_n = the number of field-7 fields, payload =
 *     the sum of len(Entry.Data) (PayloadSize, util.go:160; a nil Data counts
 *     0; Data is skipped by its length and read only where it is a conf
 *     change), ent_pos / ent_bytes = the byte range of the field-7 fields
 *     inside bytes where they are one contiguous range (the mirror of the
 *     follower ingest's; 0 / 0 otherwise).  Entry.Index and Entry.Term are
 *     validated and ignored: appendEntry overwrites them (raft.go:621-628).
 *     An entry of Type 1 (EntryConfChange) has its Data validated as
 *     ConfChange.Unmarshal, one of Type 2 (EntryConfChangeV2) as
 *     ConfChangeV2.Unmarshal (raft.pb.go:2543-2908).  cc_at = that entry's
 *     0-based position (UINT32_MAX: the message carries no conf change),
 *     cc_payload = its Data length, cc_leave = 1 iff it is a V2 without a
 *     field 2 (len(cc.AsV2().Changes) == 0, raft.go:1053; a V1 always has one
 *     change, so an empty V1 Data is not a leave).  In this order:
 *       Message.Term != 0: QB_WIRE_TERM (raft.send never puts a term on
 *         MsgProp or MsgReadIndex, raft.go:402-416; Step's term filter would
 *         act on one, so the message is the host's);
 *       no entries, or another field between two entries: QB_WIRE_ENTRIES;
 *       a conf-change Data that does not unmarshal (Go panics,
 *         raft.go:1039-1047) or a second conf-change entry:
 *         QB_WIRE_CONF_CHANGE, cc_at = UINT32_MAX, cc_payload = cc_leave = 0.
 *   MsgReadIndex (15): QB_RQ_READ.  The request's only field-7 entry must
 *     carry 8 bytes of Data that are not all zero: ctx = that id, big-endian.
 *     slot = From's slot among ids[off[g] .. off[g+1]) (at most QB_MAX_SLOTS
 *     of them): From == 0 gives 0xFF, a local request; a non-member 0xFE,
 *     which qb_dev_leader_requests answers QB_RD_HOST.  Term != 0:
 *     QB_WIRE_TERM; else no entry, two entries or another Data: QB_WIRE_CTX
 *     (ctx = 0).  Message.Context is ignored, as stepLeader ignores it.
 *   MsgTransferLeader (13): QB_RQ_TRANSFER.  slot = From's slot, 0xFE for a
 *     non-member (From == 0 included: "no Progress", ignored by the step);
 *     term is Message.Term as sent: the step has the filter.
 *   MsgReadIndexResp (16): QB_RQ_READ_RESP, decoded only: index = Index, ctx
 *     as for the read (another shape: QB_WIRE_CTX).  STEPPING IT IS THE
 *     HOST'S: the term filter on term[i] and one ReadState{index, ctx} append
 *     (raft.go:1465-1470).  It takes no part in pass 2 and no group check.
 *   every other type: QB_WIRE_TYPE, QB_RQ_NONE.
 *   a message of kinds 1-3 still QB_WIRE_OK whose msg_group[i] >= G:
 *     QB_WIRE_GROUP (the dense columns have no place for it; slot is 0xFE
 *     unless the read is local).
 *
 * Pass 2, per group: its messages of kinds 1-3 with status QB_WIRE_OK are
 * walked in batch order, whatever the skew (one group may hold the whole
 * batch).  A message is TAKEN into the dense columns unless a rule defers it:
 *   QB_RQ_READ      max_reads reads of the group are already taken, or a
 *                   proposal is;
 *   QB_RQ_TRANSFER  a transfer is already taken, or a proposal is;
 *   QB_RQ_PROP      a proposal is already taken and concat == 0; with concat
 *                   != 0: it carries a conf change and a taken one already
 *                   does, or the entry count would pass 2^32 - 1.
 * Once one message of a group is deferred every later one of that group is
 * too, which keeps arrival order across calls.  A deferred message gets
 * status QB_WIRE_DEFERRED and changes no dense column; its other columns stay,
 * and the host submits it again as it is.  concat == 0 gives one MsgProp per
 * group and call, Step's own granularity; concat != 0 the concatenation of a
 * group's proposals into one.
 *
 * THE HOST RUNS qb_dev_leader_requests FIRST AND qb_dev_leader_propose SECOND
 * on these columns.  That fixed order is what makes the two dense calls equal
 * to stepping the taken messages one by one: reads and the transfer commute
 * (see qb_dev_leader_requests), but a proposal can move `committed` in a
 * one-voter group, which a read queued behind it would see — so a read or
 * transfer behind a taken proposal waits for the next call.
 *
 * Per taken message: rd_k[i] = the read's row, ent_base[i] = the entries of
 * the group's proposal before this message's (its entries get the indexes
 * last_index - n_ents + 1 + ent_base[i] .. once QB_PFLAG_APPENDED comes back);
 * both are 0 for every other message.  Dense outputs, written for every group
 * (the caller zeroes nothing): n_reads[g]; rd_ctx / rd_from[k * G + g] for k <
 * n_reads[g] only; xf_from[g] (0xFF: none) and xf_term[g]; action[g] =
 * QB_PROP_NONE, or QB_PROP_ENTRIES with QB_PROP_CONF_CHANGE /
 * QB_PROP_CC_LEAVE_JOINT; n_ents[g] and g_payload[g], the sums; g_cc_at[g] =
 * the taken message's ent_base + its cc_at, g_cc_payload[g]; gflags[g] =
 * QB_RWFLAG_*.  These are exactly qb_request_in {n_reads, rd_ctx, rd_from,
 * xf_from, xf_term} and qb_propose_in {action, n_ents, g_payload, g_cc_at,
 * g_cc_payload}: a caller passes them on untouched.
 *
 * stats (nullable, QB_RWSTAT_COUNT device uint64, accumulated): one counter
 * per final status at its QB_WIRE_* value, then the QB_RWSTAT_* ones.
 *
 * qb_wire_requests_scratch_bytes(G, M) is 0 for G or M > 2^32 - 2.  A NULL
 * out, max_reads outside 1..QB_REQ_MAX_READS; with G > 0 a NULL off, ids or
 * dense output; with M > 0 a NULL msg_off, msg_group, message column or bytes
 * with nbytes > 0; a short workspace, such an M or G, or nbytes >= 2^32 is
 * QB_EINVAL before any launch (stats alone is nullable).  G == 0 is QB_OK and
 * writes nothing; M == 0 with G > 0 still writes the dense columns.  No
 * allocation inside the call (it can be graph-captured); nothing outside
 * [bytes, bytes + nbytes) is read and nothing outside the caller's arrays
 * written, whatever off / ids hold. */
#define QB_WIRE_TERM 6        /* MsgProp / MsgReadIndex with a Term             */
#define QB_WIRE_CONF_CHANGE 7 /* conf change that does not unmarshal, or two    */
#define QB_WIRE_GROUP 8       /* msg_group >= G                                 */
#define QB_WIRE_DEFERRED 9    /* submit again: behind what this call took       */

#define QB_RQ_NONE 0
#define QB_RQ_PROP 1
#define QB_RQ_READ 2
#define QB_RQ_TRANSFER 3
#define QB_RQ_READ_RESP 4

#define QB_RWFLAG_TAKEN 0x01u    /* a message of the group went into the dense columns */
#define QB_RWFLAG_DEFERRED 0x02u /* a message of the group was deferred                */

enum {
  /* 0 .. 9: the final statuses, at their QB_WIRE_* values (5 stays 0) */
  QB_RWSTAT_TAKEN_PROPS = 10,
  QB_RWSTAT_TAKEN_READS = 11,
  QB_RWSTAT_TAKEN_TRANSFERS = 12,
  QB_RWSTAT_READ_RESPS = 13,     /* QB_RQ_READ_RESP with QB_WIRE_OK           */
  QB_RWSTAT_ENTRIES_TAKEN = 14,  /* the sum of n_ents                         */
  QB_RWSTAT_COUNT = 15
};

typedef struct qb_request_wire_out {
  /* message-aligned, [M] */
  uint8_t* kind;          /* QB_RQ_*                                          */
  uint8_t* status;        /* QB_WIRE_*                                        */
  uint32_t* group;
  uint64_t* from;
  uint64_t* term;
  uint8_t* msg_type;      /* the low byte of Message.Type                     */
  uint8_t* slot;          /* READ / TRANSFER: From's slot, 0xFF local, 0xFE none */
  uint64_t* ctx;          /* READ / READ_RESP: the request id                 */
  uint64_t* index;        /* READ_RESP: Message.Index                         */
  uint32_t* ent_n;        /* PROP                                             */
  uint64_t* payload;      /* PROP                                             */
  uint64_t* ent_pos;      /* PROP                                             */
  uint32_t* ent_bytes;    /* PROP                                             */
  uint32_t* cc_at;        /* PROP: UINT32_MAX = no conf change                */
  uint64_t* cc_payload;   /* PROP                                             */
  uint8_t* cc_leave;      /* PROP                                             */
  uint8_t* rd_k;          /* a taken READ's row                               */
  uint32_t* ent_base;     /* a taken PROP's first entry within n_ents[g]      */
  /* dense: qb_request_in */
  uint8_t* n_reads;       /* [G] */
  uint64_t* rd_ctx;       /* [max_reads * G] k-major */
  uint8_t* rd_from;       /* [max_reads * G] k-major */
  uint8_t* xf_from;       /* [G] */
  uint64_t* xf_term;      /* [G] */
  /* dense: qb_propose_in */
  uint8_t* action;        /* [G] */
  uint32_t* n_ents;       /* [G] */
  uint64_t* g_payload;    /* [G] */
  uint32_t* g_cc_at;      /* [G] */
  uint64_t* g_cc_payload; /* [G] */
  uint8_t* gflags;        /* [G] QB_RWFLAG_* */
  uint64_t* stats;        /* nullable: [QB_RWSTAT_COUNT] */
} qb_request_wire_out;

size_t qb_wire_requests_scratch_bytes(uint64_t G, uint64_t M); /* 0: too large for one call */
int qb_dev_ingest_requests(uint64_t M, const uint8_t* bytes, uint64_t nbytes,
                           const uint64_t* msg_off, const uint32_t* msg_group, uint64_t G,
                           const uint32_t* off, const uint64_t* ids, uint32_t max_reads,
                           uint32_t concat, const qb_request_wire_out* out, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------------- */
/* Wire encode: Message.Marshal of the outboxes                            */
/* ----------------------------------------------------------------------- */

/* The sending side of the wire ingest: the messages the step calls leave as
 * records and slot-aligned columns -> gogoproto-encoded raftpb.Message bytes,
 * bit for bit Message.Marshal (raftpb/raft.pb.go: Size 1235-1263,
 * MarshalToSizedBuffer 903-972; the nested Snapshot 863-886,
 * SnapshotMetadata 824-846, ConfState 1021-1063 and Entry 785-807).  Fields go
 * in field-number order; every non-nullable field is written whatever it
 * holds (Type, To, From, Term, LogTerm, Index, Commit, Snapshot, Reject,
 * RejectHint), Context only when non-nil.  The Snapshot of every message
 * encoded here is the empty one: 4a 0a 12 08 0a 02 28 00 10 00 18 00.
 * A context is the project's 8-byte big-endian request id in a uint64, 0 =
 * nil.  For MsgReadIndex (15) and MsgReadIndexResp (16) the id travels as one
 * Entry{Data: id} in field 7 (3a 10 08 00 10 00 18 00 22 08 + the 8 bytes),
 * not as Context (responseToReadIndexReq raft.go:1737-1751 hands req.Entries
 * back; a follower forwards the request whole, raft.go:1445-1470); id 0 writes
 * neither.
 * Entry payloads and snapshots never reach the device: a message with n > 0
 * entries is written whole except field 7, and ent_at[i] is the byte offset
 * inside message i just behind the Index field, where the host splices its
 * encoded entries (one 3a-keyed field each); a MsgSnap is left to the host.
 *
 * Message i is bytes[msg_off[i] .. msg_off[i+1]).  msg_off [M+1] is always
 * complete (it is the array qb_dev_ingest_messages takes) and *nbytes =
 * msg_off[M] is what the batch needs, so a caller can size a retry.  A
 * message whose end lies past cap gets QB_ENC_NO_SPACE and none of its bytes
 * is written; those before it are intact.  Nothing outside [bytes, bytes +
 * cap) is written, and inside it only the bytes of written messages: bytes
 * may have any alignment.  ent_at (nullable) is written where status <= 1,
 * stats (nullable, QB_ENC_STATUS_COUNT device uint64, accumulated) counts
 * each status. */
#define QB_ENC_OK 0        /* the bytes are the complete message                 */
#define QB_ENC_ENTRIES 1   /* complete but for field 7 at ent_at                 */
#define QB_ENC_HOST 2      /* length 0: the host marshals it (MsgSnap, or a type
                              the front end does not form)                        */
#define QB_ENC_NONE 3      /* length 0: no message here                          */
#define QB_ENC_NO_SPACE 4  /* length counted, not written                        */
#define QB_ENC_STATUS_COUNT 5
/* The longest message the device writes, a read type with a context: Type 2
 * (the two read types are below 128), To / From / Term / LogTerm / Index 11
 * each, the read entry 18, Commit 11, Snapshot 12, Reject 2, RejectHint 11.
 * Any other type (a uint8: up to 3 bytes) carries a Context of 10 instead of
 * the entry: 104 at most. */
#define QB_ENC_MAX_BYTES 111

typedef struct qb_encode_out {
  uint8_t* bytes;     /* [cap]                                             */
  uint64_t cap;
  uint64_t* msg_off;  /* [M+1]                                             */
  uint8_t* status;    /* [M] QB_ENC_*                                      */
  uint32_t* ent_at;   /* [M] nullable                                      */
  uint64_t* nbytes;   /* device uint64                                     */
  uint64_t* stats;    /* nullable: [QB_ENC_STATUS_COUNT] accumulated       */
} qb_encode_out;

/* The general form: every field explicit, all columns [M]; a NULL column
 * reads as 0 (type is required).  Term is taken as given: raft.send's rule
 * (raft.go:386-419) is the caller's.  Type QB_MSG_SNAP gives QB_ENC_HOST and
 * type 0 QB_ENC_NONE; n_entries > 0 gives QB_ENC_ENTRIES (for the two read
 * types n_entries is not read: their entry is the context). */
typedef struct qb_encode_cols {
  const uint8_t* type;
  const uint64_t* to;
  const uint64_t* from;
  const uint64_t* term;
  const uint64_t* log_term;
  const uint64_t* index;
  const uint64_t* commit;
  const uint64_t* reject_hint;
  const uint8_t* reject;      /* 0 / non-zero                                */
  const uint64_t* context;
  const uint64_t* n_entries;
} qb_encode_cols;

/* The groups of the two front ends over the step calls' outputs: the CSR
 * every call already has plus the sender.  Both apply raft.send
 * (raft.go:386-419): From = self_id[g], Term = term[g]; To = ids[slot].  They
 * form QB_MSG_APP, QB_MSG_HEARTBEAT, QB_MSG_TIMEOUT_NOW and
 * QB_MSG_READ_INDEX_RESP; QB_MSG_SNAP and any other type give QB_ENC_HOST;
 * type 0, QB_READ_STATE, to = 0xFF, a slot outside its group (or past the
 * group's QB_MAX_SLOTS-th) and a group >= G give QB_ENC_NONE. */
typedef struct qb_encode_groups {
  uint64_t G;
  const uint32_t* off;      /* [G+1] */
  const uint64_t* ids;      /* [off[G]] slot -> raft ID */
  const uint64_t* self_id;  /* [G] */
  const uint64_t* term;     /* [G] */
} qb_encode_groups;

/* Slot-aligned messages, as the heartbeats are: message s belongs to slot s,
 * M = S = off[G] (the caller's count: slots the off table does not cover get
 * QB_ENC_NONE).  A group takes part where gflags == NULL or gflags[g] &
 * gmask; the slot whose ID is self_id[g] never gets a message.  One form for
 * the tick's broadcast (tflags & QB_TFLAG_BEAT, type_all QB_MSG_HEARTBEAT,
 * hb_commit as commit, hb_ctx as ctx_g: sendHeartbeat raft.go:495-511), the
 * requests' heartbeats (qflags & QB_QFLAG_HEARTBEATS) and the proposal's
 * bcastAppend (pflags & QB_PFLAG_BCAST, msg_type / msg_index / msg_log_term /
 * msg_n, committed as commit_g: maybeSendAppend raft.go:432-492). */
typedef struct qb_encode_slot_cols {
  uint64_t S;
  const uint8_t* gflags;     /* [G] nullable                                */
  uint32_t gmask;
  uint32_t type_all;         /* the type of every slot where type == NULL   */
  const uint8_t* type;       /* [S] nullable                                */
  const uint64_t* index;     /* [S] nullable                                */
  const uint64_t* log_term;  /* [S] nullable                                */
  const uint64_t* commit;    /* [S] nullable                                */
  const uint64_t* n_entries; /* [S] nullable                                */
  const uint64_t* commit_g;  /* [G] nullable: Commit where commit == NULL   */
  const uint64_t* ctx_g;     /* [G] nullable                                */
} qb_encode_slot_cols;

/* Workspace of a call over M messages (0: M * QB_ENC_MAX_BYTES >= 2^32, too
 * large for one call: the offsets' scan is 32-bit).  A NULL required pointer,
 * a short workspace or such an M is QB_EINVAL before any launch; M == 0 (or
 * G == 0) is QB_OK with *nbytes = 0 and msg_off[0] = 0 written.  No
 * allocation inside the calls (they can be graph-captured).
 * qb_dev_encode_msg_out takes qb_dev_leader_step's dense list (the outbox's
 * slots / chunks work too, as flat arrays: a zeroed record has type 0) with M
 * = msg_cap; records at or past *msg_total (device, nullable: all msg_cap)
 * get QB_ENC_NONE — the count is never copied back.  MsgApp: Index / LogTerm
 * / Commit from the record, aux entries; MsgReadIndexResp: Index from index,
 * the entry from aux. */
size_t qb_encode_scratch_bytes(uint64_t M);
int qb_dev_encode_messages(uint64_t M, const qb_encode_cols* c, const qb_encode_out* out,
                           void* workspace, size_t workspace_bytes, void* stream);
int qb_dev_encode_msg_out(const qb_encode_groups* eg, const qb_msg_out* msgs, uint64_t msg_cap,
                          const uint64_t* msg_total, const qb_encode_out* out, void* workspace,
                          size_t workspace_bytes, void* stream);
int qb_dev_encode_slots(const qb_encode_groups* eg, const qb_encode_slot_cols* s,
                        const qb_encode_out* out, void* workspace, size_t workspace_bytes,
                        void* stream);

/* ----------------------------------------------------------------------- */
/* Configuration changes                             */
/* ----------------------------------------------------------------------- */

/* One confchange.Changer operation per group, all groups in one call:
 * Simple / EnterJoint(autoLeave) / LeaveJoint (confchange/confchange.go:
 * 49-146) over the group's ConfChangeSingle list (apply, makeVoter,
 * makeLearner, remove, initProgress: confchange.go:151-281), with
 * checkInvariants on input and output (confchange.go:283-334).
 * A group's config is its CSR slots (ascending IDs of the ProgressMap) with
 * cfg = Voters[0] | Voters[1] << 16 and ext = LearnersNext | AutoLeave << 16;
 * a slot in none of the three masks is a learner.  The result is written to
 * a second set of arrays (double-buffered): new_off [G+1] (offsets), slot
 * IDs, masks and the Progress arrays of the leader-step layout — carried for
 * kept slots, initialised for added ones (Next = last_index[g], Match 0,
 * StateProbe, RecentActive; initProgress).  A group whose operation fails
 * keeps its config and Progress; err[g] names the reference's error and
 * err_id[g] (nullable) the offending ID where the message has one (the
 * smallest such ID).  Restore(ConfState) (confchange/restore.go:116-155) is a
 * sequence of such calls. */
#define QB_CC_NONE 0                 /* copy through                      */
#define QB_CC_SIMPLE 1
#define QB_CC_ENTER_JOINT 2
#define QB_CC_ENTER_JOINT_AUTOLEAVE 3
#define QB_CC_LEAVE_JOINT 4

/* raftpb.ConfChangeType (raft.pb.go) */
#define QB_CC_ADD_NODE 0
#define QB_CC_REMOVE_NODE 1
#define QB_CC_UPDATE_NODE 2
#define QB_CC_ADD_LEARNER 3

enum {
  QB_CCERR_OK = 0,
  QB_CCERR_ALREADY_JOINT = 1,       /* "config is already joint"                        */
  QB_CCERR_ZERO_VOTER_JOINT = 2,    /* "can't make a zero-voter config joint"           */
  QB_CCERR_NOT_JOINT = 3,           /* "can't leave a non-joint config"                 */
  QB_CCERR_SIMPLE_IN_JOINT = 4,     /* "can't apply simple config change in joint config" */
  QB_CCERR_MORE_THAN_ONE = 5,       /* "more than one voter changed without entering joint config" */
  QB_CCERR_REMOVED_ALL = 6,         /* "removed all voters"                             */
  QB_CCERR_UNKNOWN_TYPE = 7,        /* "unexpected conf type %d"                        */
  QB_CCERR_NO_PROGRESS = 8,         /* "no progress for %d"                             */
  QB_CCERR_LNEXT_NOT_OUTGOING = 9,  /* "%d is in LearnersNext, but not Voters[1]"       */
  QB_CCERR_LNEXT_IS_LEARNER = 10,   /* "%d is in LearnersNext, but is already marked as learner" */
  QB_CCERR_LEARNER_OUTGOING = 11,   /* "%d is in Learners and Voters[1]"                */
  QB_CCERR_LEARNER_INCOMING = 12,   /* "%d is in Learners and Voters[0]"                */
  QB_CCERR_LEARNER_NOT_MARKED = 13, /* "%d is in Learners, but is not marked as learner" */
  QB_CCERR_AUTOLEAVE_NOT_JOINT = 14, /* "AutoLeave must be false when not joint"        */
  QB_CCERR_TOO_MANY_SLOTS = 15,     /* engine limit: > QB_MAX_SLOTS members, or > 24 IDs alive at once within one change list
                                       (a current config of > 24 slots is kept as it is, and
                                       copied through under QB_CC_NONE) */
  QB_CCERR_BAD_OP = 16              /* op is not a QB_CC_* operation                     */
};

typedef struct qb_conf_change_in {
  uint64_t G;
  uint32_t inflight_cap;     /* ring size of infl_buf per slot */
  uint32_t reserved;
  const uint8_t* op;         /* [G] QB_CC_*                           */
  const uint32_t* cc_off;    /* [G+1] ConfChangeSingle list per group */
  const uint8_t* cc_type;    /* [cc_off[G]] QB_CC_ADD_NODE ...         */
  const uint64_t* cc_node;   /* [cc_off[G]] NodeID (0 = ignored)       */
  const uint64_t* last_index; /* [G] Changer.LastIndex                 */
  const uint32_t* off;       /* [G+1] current slots                    */
  const uint64_t* ids;       /* [off[G]] ascending per group           */
  const uint32_t* cfg;       /* [G]                                     */
  const uint32_t* ext;       /* [G] (nullable: no LearnersNext/AutoLeave) */
  const uint64_t* match;     /* Progress, leader-step layout [off[G]]  */
  const uint64_t* next;
  const uint64_t* pending_snapshot;
  const uint8_t* pstate;
  const uint32_t* infl_pos;
  const uint64_t* infl_buf;  /* [off[G] * inflight_cap]; 8-byte aligned suffices (16-byte
                                aligned in and out buffers let inflight_cap 4 move rings
                                as 16-byte words) */
} qb_conf_change_in;

typedef struct qb_conf_change_out {
  uint64_t slot_cap;         /* capacity of the per-slot output arrays */
  uint32_t* new_off;         /* [G+1]; new_off[G] = slots needed        */
  uint64_t* ids;
  uint32_t* cfg;             /* [G] */
  uint32_t* ext;             /* [G] */
  uint64_t* match;
  uint64_t* next;
  uint64_t* pending_snapshot;
  uint8_t* pstate;
  uint32_t* infl_pos;
  uint64_t* infl_buf;
  uint8_t* err;              /* [G] QB_CCERR_*   */
  uint64_t* err_id;          /* [G] (nullable)   */
} qb_conf_change_out;

size_t qb_conf_change_workspace_bytes(uint64_t G);
/* If new_off[G] > slot_cap nothing past the capacity is written: check
 * new_off[G] after the call. */
int qb_dev_conf_change(const qb_conf_change_in* in, const qb_conf_change_out* out,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------------- */
/* switchToConfig: what follows a configuration change                     */
/* ----------------------------------------------------------------------- */

/* raft.switchToConfig (raft.go:1651-1700) for G groups in one call: the tail
 * of applyConfChange (raft.go:1623-1650) behind qb_dev_conf_change, and the
 * tail of restore (raft.go:1606-1609) behind qb_dev_follower_snapshot.  Dense,
 * one action byte per group, groups independent.  The new config and Progress
 * are qb_dev_conf_change's outputs (off / ids / cfg and the Progress arrays,
 * read and written in place); old_off / old_ids are the off / ids that went
 * into that call.
 *
 * action[g]:
 *   QB_SW_NONE     nothing (swflags[g] = 0);
 *   QB_SW_SWITCH   applyConfChange's tail: steps 1-6;
 *   QB_SW_RESTORE  restore's tail: steps 1-6, then 7;
 *   any other code is treated as QB_SW_NONE and counted
 *   (QB_SWSTAT_BAD_ACTION).
 *
 * Per acting group, in this order:
 *   1. Renumber (this library's representation, not Go; whatever the role).
 *      A slot is an ID's rank, so the two ascending ID lists give the new
 *      slot of every old slot (slot_map, 0xFF: removed).  The own slot (meta
 *      bits 0-7) becomes the rank of self_id in the new IDs, or 0xFF; the
 *      transferee slot (meta bits 8-15), the ack bits and the From slot of
 *      each pending rq_meta entry (meta bits 20-24 of them, at most
 *      readq_cap) and both halves of votes go through the map.  Bits of
 *      removed slots are dropped.  A dropped voted bit raises
 *      QB_SWFLAG_VOTE_DROPPED: Go keeps Votes by ID, so this matters only if
 *      the ID comes back within the same candidacy (the host then records
 *      that vote again).
 *   2. Stops, found before anything is written: swflags[g] =
 *      QB_SWFLAG_HOST alone, nothing of the group changes and no output but
 *      swflags is written.
 *      (a) a pending read whose From slot names an ID that is not in the new
 *          config (Go keeps the message's ID; a slot cannot);
 *      (b) a leader that is removed or demoted while its transferee's ID is
 *          not in the new config (Go returns early and keeps the ID).
 *   3. isLearner: the own slot is present and in neither voter half.  Own
 *      slot absent or a learner at a leader: QB_SWFLAG_SELF_REMOVED /
 *      QB_SWFLAG_SELF_LEARNER and 4-6 are skipped (raft.go:1663-1674; the
 *      transferee is not aborted here, as in Go).
 *   4. Not a leader, or no incoming voter (cfg & 0xFFFF == 0): 5-6 are
 *      skipped (raft.go:1678).
 *   5. maybeCommit (raft.go:585-588, log.go:328-334): the joint committed
 *      index over the new match and cfg, taken iff it is > committed and its
 *      term, through the run table, equals term (term() is 0 outside
 *      [first_index - 1, last_index]).
 *        true:  QB_SWFLAG_COMMITTED and bcastAppend: maybeSendAppend(to,
 *               true) for every slot but the own, exactly as
 *               qb_dev_leader_propose sends;
 *        false: maybeSendAppend(id, false) for every slot, the own included,
 *               as Visit does.  With sendIfEmpty == false an empty entry list
 *               returns before the snapshot fallback (raft.go:442-444), so a
 *               compacted next sends nothing here.
 *      Either way QB_SWFLAG_SENT: msg_type[s] = 0 / QB_MSG_APP / QB_MSG_SNAP
 *      for every new slot of the group, with qb_propose_out's contract
 *      (Commit is committed[g] after the call).
 *   6. The transferee, if not 0xFF and in neither voter half of the new
 *      config, becomes 0xFF: QB_SWFLAG_TRANSFER_ABORTED (raft.go:1695-1697).
 *   7. QB_SW_RESTORE only, whatever 3 and 4 decided: with an own slot
 *      present, MaybeUpdate(next - 1) on it (progress.go:144-153).
 * Every acting group that is not stopped gets QB_SWFLAG_SWITCHED.
 *
 * QB_ROLE_PROMOTABLE is not touched: qb_dev_campaign tests membership itself,
 * the bit carries only !hasPendingSnapshot.  Stays the host's: the ConfState
 * returned to the application, r.isLearner beyond what meta and cfg say, a
 * stopped group, and any slot-indexed state of its own (through slot_map).
 * Index arithmetic wraps as Go's uint64 does.  A slot count above
 * QB_MAX_SLOTS is read as QB_MAX_SLOTS, a run count of 0 as 1 and above 8 as
 * 8, a request count above readq_cap as readq_cap; an old slot at or above
 * the old slot count maps to 0xFF. */
#define QB_SW_NONE 0
#define QB_SW_SWITCH 1
#define QB_SW_RESTORE 2

#define QB_SWFLAG_SWITCHED 0x01u         /* renumbered: meta / votes / rq_meta / slot_map */
#define QB_SWFLAG_COMMITTED 0x02u        /* maybeCommit returned true               */
#define QB_SWFLAG_SENT 0x04u             /* step 5 ran: msg_type of the group's slots written */
#define QB_SWFLAG_TRANSFER_ABORTED 0x08u /* the transferee was removed or demoted   */
#define QB_SWFLAG_SELF_REMOVED 0x10u     /* a leader without a Progress of its own  */
#define QB_SWFLAG_SELF_LEARNER 0x20u     /* a leader demoted to learner             */
#define QB_SWFLAG_VOTE_DROPPED 0x40u     /* a recorded vote's slot was removed      */
#define QB_SWFLAG_HOST 0x80u             /* stopped: nothing applied                */

enum {
  QB_SWSTAT_SWITCHED = 0,         /* groups renumbered (restores included)     */
  QB_SWSTAT_RESTORES = 1,         /* of them under QB_SW_RESTORE               */
  QB_SWSTAT_COMMITS = 2,
  QB_SWSTAT_BCAST = 3,            /* groups that ran bcastAppend               */
  QB_SWSTAT_PROBED = 4,           /* groups that ran maybeSendAppend(id, false) */
  QB_SWSTAT_MSG_APP = 5,
  QB_SWSTAT_MSG_SNAP = 6,
  QB_SWSTAT_TRANSFER_ABORTED = 7,
  QB_SWSTAT_SELF_REMOVED = 8,
  QB_SWSTAT_SELF_LEARNER = 9,
  QB_SWSTAT_VOTE_DROPPED = 10,
  QB_SWSTAT_HOST = 11,
  QB_SWSTAT_BAD_ACTION = 12,
  QB_SWSTAT_COUNT = 13
};

/* The per-group and Progress arrays are those of qb_leader_groups,
 * qb_campaign_groups and qb_propose_groups (same layouts: a caller passes the
 * same buffers), the Progress arrays and off / ids / cfg being
 * qb_conf_change_out's. */
typedef struct qb_switch_groups {
  uint64_t G;
  uint32_t inflight_cap;        /* 1..4096                                  */
  uint32_t readq_cap;           /* 0..QB_LEADER_MAX_READQ                   */
  const uint32_t* old_off;      /* [G+1] the config before the change       */
  const uint64_t* old_ids;      /* [old_off[G]] ascending per group         */
  const uint32_t* off;          /* [G+1] the new config                     */
  const uint64_t* ids;          /* [off[G]] ascending per group             */
  const uint32_t* cfg;          /* [G] */
  const uint64_t* self_id;      /* [G] */
  const uint8_t* role;          /* [G] QB_ROLE_* */
  const uint64_t* term;         /* [G] */
  const uint64_t* first_index;  /* [G] */
  const uint64_t* last_index;   /* [G] */
  const uint64_t* last_term;    /* [G] the term of last_index */
  const uint64_t* snap_index;   /* [G] */
  const uint64_t* snap_term;    /* [G] */
  const uint64_t* max_ents;     /* [G] */
  const uint64_t* run_start;    /* [QB_LEADER_MAX_RUNS * G] run-major */
  const uint64_t* run_term;     /* same layout */
  uint32_t* meta;               /* [G] in/out: only bits 0-15 may change */
  uint64_t* committed;          /* [G] in/out */
  uint32_t* votes;              /* [G] in/out: voted | granted << 16 (nullable) */
  uint32_t* rq_meta;            /* [G * readq_cap] in/out; NULL iff readq_cap == 0 */
  /* per new slot, S = off[G] (in/out) */
  uint64_t* match;
  uint64_t* next;
  uint64_t* pending_snapshot;
  uint8_t* pstate;
  uint32_t* infl_pos;
  uint64_t* infl_buf;           /* [S * inflight_cap] */
} qb_switch_groups;

typedef struct qb_switch_out {
  uint8_t* swflags;       /* [G] QB_SWFLAG_*, written for every group */
  uint8_t* slot_map;      /* [old_off[G]] (nullable) the new slot of each old slot, 0xFF:
                             removed; written for every old slot of a group with
                             QB_SWFLAG_SWITCHED and for no other slot */
  uint8_t* msg_type;      /* [S] written for every new slot of a group with QB_SWFLAG_SENT
                             and for no other slot */
  uint64_t* msg_index;    /* [S] written only where msg_type != 0 */
  uint64_t* msg_log_term; /* [S] same */
  uint64_t* msg_n;        /* [S] same: entries of the MsgApp (0 for a MsgSnap) */
} qb_switch_out;

/* stats: QB_SWSTAT_COUNT device uint64 (accumulated).  G == 0 is QB_OK and
 * writes nothing; every pointer but votes, slot_map (and rq_meta with
 * readq_cap 0) is required.  No workspace and no allocation inside the call
 * (it can be graph-captured); nothing outside the caller's arrays is read or
 * written. */
int qb_dev_switch_config(const qb_switch_groups* sg, const uint8_t* action,
                         const qb_switch_out* out, uint64_t* stats, void* stream);

/* ----------------------------------------------------------------------- */
/* Sharding over the GPUs of a node                        */
/* ----------------------------------------------------------------------- */

/* One process per GPU; rank r owns the contiguous global groups
 * [begin, end) = qb_shard_range(total, world, r) (sizes differ by at most
 * one; etcd_amd/shard.py shard_range).  Groups are independent, so the hot
 * path exchanges nothing; the one collective is at its edge: the node-wide
 * CommittedIndex / VoteResult vectors assembled from the shards by an RCCL
 * all-gather over xGMI.  The host distributes the 128-byte unique ID from
 * rank 0 over its own transport (the reference's peer transport is
 * rafthttp, server/etcdserver/api/rafthttp/peer.go:178). */
#define QB_COMM_ID_BYTES 128
typedef struct qb_comm qb_comm;
int qb_shard_range(uint64_t total, int world, int rank, uint64_t* begin, uint64_t* end);
int qb_comm_get_unique_id(void* id_out);
/* ncclCommInitRank on the calling thread's current device (qb_set_device);
 * collective: every rank calls it with the same id. */
int qb_comm_init(qb_comm** out, int world, int rank, const void* id);
int qb_comm_destroy(qb_comm* comm);
size_t qb_allgather_workspace_bytes(uint64_t total, int world);
/* commit_all[total] / vote_all[total] (device; either nullable) receive every
 * rank's shard in rank order (a rank whose shard is empty, total < world,
 * may pass NULL shard vectors).  Collective over the comm, enqueued on stream.
 * The workspace (device, qb_allgather_workspace_bytes) is needed only when
 * total % world != 0 (padded shards compacted by rank). */
int qb_dev_allgather_results(qb_comm* comm, uint64_t total,
                             const uint64_t* commit_shard, const uint8_t* vote_shard,
                             uint64_t* commit_all, uint8_t* vote_all,
                             void* workspace, size_t workspace_bytes, void* stream);

/* The changed-commit delta (gather only the groups whose
 * commit moved).  A group surfaces a Ready when its HardState changed
 * (raft/node.go:573 newReady, raft/rawnode.go:157 HasReady); in a tick that
 * is the groups whose maybeCommit advanced (raft.go:585-588) — the tracker
 * steps' advanced_out.  Device half: the n groups' changed flags (u8, nonzero
 * = changed) compacted in group order into (g_base + g, commit[g]) pairs in
 * out_gid / out_commit (room for n each); *out_count (device u64) = pairs
 * written (global groups must fit uint32). */
size_t qb_compact_changed_workspace_bytes(uint64_t n);
int qb_dev_compact_changed(uint64_t n, const uint8_t* changed, const uint64_t* commit,
                           uint64_t g_base, uint32_t* out_gid, uint64_t* out_commit,
                           uint64_t* out_count, void* workspace, size_t workspace_bytes,
                           void* stream);
/* commit_all[gid[i]] = commit[i] for i < m (gid UINT32_MAX or >= total:
 * skipped, the padding of the exchange below). */
int qb_dev_scatter_changed(uint64_t m, const uint32_t* gid, const uint64_t* commit, uint64_t total,
                           uint64_t* commit_all, void* stream);
size_t qb_allgather_changed_workspace_bytes(uint64_t total, int world);
/* Collective over the comm: this rank's shard's changed groups (changed_shard
 * / commit_shard: the shard's local arrays, qb_shard_range) are exchanged and
 * applied to commit_all[total] (device) on every rank — the caller keeps
 * commit_all across ticks.  Every rank pads its pairs to the largest
 * per-rank count C_max, so each rank receives 12 * world * C_max bytes (not
 * 12 per changed group): a skewed tick (one shard with many commits)
 * approaches the full gather's cost, and when 12 * C_max exceeds 8 * the
 * shard size the call is cheaper as qb_dev_allgather_results (it picks that
 * itself: see below).  *changed_total (host) = changed groups node-wide.  The
 * host waits on the stream once (the exchange size is data-dependent); a
 * rank's local failure in the compaction (NULL shard columns included)
 * reaches every rank through the gathered counts, so all return QB_EINVAL
 * together.  Every rank must pass the same total, a non-NULL commit_all and a
 * large enough workspace: a rank failing those checks returns before the
 * count all-gather and leaves the others waiting in it (as
 * qb_dev_route_records). */
int qb_dev_allgather_changed(qb_comm* comm, uint64_t total, const uint8_t* changed_shard,
                             const uint64_t* commit_shard, uint64_t* commit_all,
                             uint64_t* changed_total, void* workspace, size_t workspace_bytes,
                             void* stream);

/* Record delivery to the owning shards ("message batches are
 * bucketed by owning shard").  A node's inbound responses arrive at any rank;
 * each record goes to the rank owning its global group, with the group
 * rebased to that shard's local index (a group >= total goes to the last
 * rank as an index >= its shard size, which the steps count as a bad group).
 * Delivery is stable: the receiver gets each source rank's records in
 * source-rank order, each source's in their original order — the batch order
 * the leader step's sequential semantics need (raft.go:1099-1342 is a
 * per-message fold).  Replaces the Python etcd_amd/shard.py:route_records
 * (torch bucketize / argsort / all_to_all_single) for a cgo embedder. */
#define QB_ROUTE_MAX_WORLD 64
size_t qb_route_partition_workspace_bytes(int world, uint64_t M);
/* The device half (no communication; usable with any world for testing and
 * by callers with their own transport): the batch's records stably
 * partitioned by owner into the send_* columns (M entries each; hint /
 * log_term both-or-neither with their inputs), send_off[world + 1] (device)
 * = the first send position per destination rank, send_off[world] = M. */
int qb_dev_route_partition(uint64_t total, int world, uint64_t M, const uint32_t* rec_group,
                           const uint8_t* rec_flags, const uint64_t* rec_index,
                           const uint64_t* rec_term, const uint64_t* rec_hint,
                           const uint64_t* rec_log_term, uint32_t* send_group,
                           uint8_t* send_flags, uint64_t* send_index, uint64_t* send_term,
                           uint64_t* send_hint, uint64_t* send_log_term, uint32_t* send_off,
                           void* workspace, size_t workspace_bytes, void* stream);
size_t qb_route_workspace_bytes(int world, uint64_t M);
/* Collective over the comm: partition, an all-gather of every rank's counts
 * and output capacity (every rank refuses with QB_EINVAL if any rank's
 * receive would exceed its out_cap — one decision everywhere, no rank left in
 * a send), then RCCL point-to-point runs per column into out_* (device,
 * out_cap entries).  *out_count (host) = records received.  The host waits on
 * the stream twice (the receive sizes are data-dependent).  Every rank must
 * call it with valid arguments: a rank failing a precondition before the
 * all-gather leaves the others waiting in it. */
int qb_dev_route_records(qb_comm* comm, uint64_t total, uint64_t M, const uint32_t* rec_group,
                         const uint8_t* rec_flags, const uint64_t* rec_index,
                         const uint64_t* rec_term, const uint64_t* rec_hint,
                         const uint64_t* rec_log_term, uint32_t* out_group, uint8_t* out_flags,
                         uint64_t* out_index, uint64_t* out_term, uint64_t* out_hint,
                         uint64_t* out_log_term, uint64_t out_cap, uint64_t* out_count,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------------- */
/* Synthetic workload generators (bench/test inputs)        */
/* ----------------------------------------------------------------------- */

/* Counter-based, so every shard/device/CPU regenerates identical inputs:
 * r(g, slot, field) = splitmix64(seed ^ (g << 12 | slot << 4 | field)).
 * g_begin offsets the global group number (sharding). */
int qb_dev_synth_fixed(uint64_t seed, uint32_t n, uint64_t G, uint64_t g_begin,
                       uint64_t* match, void* voted, void* granted,
                       uint64_t* term_start, void* stream);
/* Host-side: group sizes and CSR offsets of the ragged config (s_g = n_g +
 * learners_g).  off has G+1 entries.  Returns QB_OK or QB_EINVAL if the total
 * overflows uint32. */
int qb_host_synth_csr_offsets(uint64_t seed, uint64_t G, uint64_t g_begin,
                              uint32_t* off);
/* Device fill of the ragged (kind 0) or joint 5+5 (kind 1) config given off. */
int qb_dev_synth_csr(uint64_t seed, int kind, uint64_t G, uint64_t g_begin,
                     const uint32_t* off, uint64_t* match, uint32_t* cfg,
                     uint32_t* votes, void* stream);
/* Host-side joint offsets: s_g = 10 - overlap_g. */
int qb_host_synth_joint_offsets(uint64_t seed, uint64_t G, uint64_t g_begin,
                                uint32_t* off);

#ifdef __cplusplus
}
#endif

#endif /* QUORUM_BATCH_H */
