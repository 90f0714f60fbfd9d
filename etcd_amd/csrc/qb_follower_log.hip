// qb_follower_log.hip — qb_dev_follower_log_step: the LOG = true instantiation
// of qb_follower_impl.h, the follower step plus QB_FIN_APP (pb.MsgApp).  A
// translation unit of its own, so that qb_follower.hip compiles to the code
// object it had before this call existed.
#include "qb_follower_impl.h"

using namespace qb;

// The grouping is the follower step's, so is the workspace
// (qb_follower_workspace_bytes).
extern "C" int qb_dev_follower_log_step(const qb_follower_groups* fg, const qb_follower_log* lg,
                                        const qb_follower_inbox* in, const qb_follower_app_inbox* app,
                                        uint8_t* resp_type, uint64_t* resp_term,
                                        const qb_follower_app_out* out, uint32_t* stop_at,
                                        uint8_t* gflags, uint64_t* stats, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  QB_REQUIRE(fg, "qb_dev_follower_log_step: fg is NULL");
  QB_REQUIRE(lg, "qb_dev_follower_log_step: lg is NULL");
  QB_REQUIRE(in, "qb_dev_follower_log_step: in is NULL");
  QB_REQUIRE(app, "qb_dev_follower_log_step: app is NULL");
  QB_REQUIRE(out, "qb_dev_follower_log_step: out is NULL");
  QB_REQUIRE(fg->election_timeout >= 1,
             "qb_dev_follower_log_step: election_timeout must be >= 1 (got %u)", fg->election_timeout);
  QB_REQUIRE(fg->check_quorum <= 1, "qb_dev_follower_log_step: check_quorum must be 0 or 1 (got %u)",
             fg->check_quorum);
  QB_REQUIRE(fg->pre_vote <= 1, "qb_dev_follower_log_step: pre_vote must be 0 or 1 (got %u)",
             fg->pre_vote);
  QB_REQUIRE(in->M <= fol::kMaxM, "qb_dev_follower_log_step: M %llu > 2^32 - 2",
             static_cast<unsigned long long>(in->M));
  QB_REQUIRE(fg->G <= 0xFFFFFFFFull, "qb_dev_follower_log_step: G %llu > 2^32 - 1 (groups are uint32)",
             static_cast<unsigned long long>(fg->G));
  if (fg->G == 0) return QB_OK;  // every record is a bad group; nothing to initialise
  const u64 G = fg->G, M = in->M;
  QB_REQUIRE(fg->term && fg->vote && fg->lead && fg->committed && fg->last_index && fg->last_term &&
                 fg->role && fg->election_elapsed && fg->heartbeat_elapsed,
             "qb_dev_follower_log_step: required group pointer is NULL");
  QB_REQUIRE(lg->meta && lg->first_index && lg->last_index && lg->last_term && lg->run_start &&
                 lg->run_term,
             "qb_dev_follower_log_step: required log pointer is NULL");
  QB_REQUIRE(lg->last_index == fg->last_index,
             "qb_dev_follower_log_step: lg->last_index != fg->last_index (the step reads and "
             "writes one array)");
  QB_REQUIRE(lg->last_term == fg->last_term,
             "qb_dev_follower_log_step: lg->last_term != fg->last_term (the step reads and "
             "writes one array)");
  QB_REQUIRE(M == 0 || (in->group && in->flags && in->from && in->term && in->index && in->aux),
             "qb_dev_follower_log_step: required inbox pointer is NULL");
  QB_REQUIRE(M == 0 || (app->commit && app->ent_off && (app->E == 0 || (app->ent_term && app->ent_len))),
             "qb_dev_follower_log_step: required append-inbox pointer is NULL (commit / ent_off / "
             "ent_term / ent_len)");
  QB_REQUIRE(stop_at && gflags && stats && (M == 0 || (resp_type && resp_term)),
             "qb_dev_follower_log_step: required output pointer is NULL (resp_type / resp_term / "
             "stop_at / gflags / stats)");
  QB_REQUIRE(M == 0 || (out->resp_index && out->resp_hint && out->resp_log_term && out->app_from),
             "qb_dev_follower_log_step: required append-output pointer is NULL (resp_index / "
             "resp_hint / resp_log_term / app_from)");
  const fol::Carve cv = fol::carve(G, M);
  QB_REQUIRE(workspace, "qb_dev_follower_log_step: workspace is NULL");
  QB_REQUIRE(workspace_bytes >= cv.total,
             "qb_dev_follower_log_step: workspace too small: %zu < %zu "
             "(qb_follower_workspace_bytes)",
             workspace_bytes, cv.total);
  QB_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0,
             "qb_dev_follower_log_step: workspace must be 8-byte aligned");
  char* ws = static_cast<char*>(workspace);
  fol::LogArgs A;
  fol::bind(A, fg, in, resp_type, resp_term, stop_at, gflags, stats, ws, cv);
  A.lg = *lg;
  A.app = *app;
  A.out = *out;
  return fol::launch<true>(A, cv, ws, as_stream(stream), "qb_dev_follower_log_step: memset");
}
