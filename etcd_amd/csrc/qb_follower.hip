// qb_follower.hip — qb_dev_follower_step: the LOG = false instantiation of
// qb_follower_impl.h (kinds 0-4; the kernels and what they do are described there).
#include "qb_follower_impl.h"

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
  fol::Args A;
  fol::bind(A, fg, in, resp_type, resp_term, stop_at, gflags, stats, ws, cv);
  return fol::launch<false>(A, cv, ws, as_stream(stream), "qb_dev_follower_step: memset");
}
