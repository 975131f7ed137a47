// handles.hpp -- what the units of libopenpano_hip.so use of each other's result handles and per-context state, declared once.
// The handle types themselves are declared by openpano_hip.h; op_features is laid out in features.hpp, op_matches in
// match.hip, op_ransac_result in ransac.hip.
#pragma once
#include "internal.hpp"

// features.hip
struct FeatView { int n; const int* counts; const int64_t* offsets; const float* desc; int device; };       // desc: null for a coordinates-only table
FeatView op_features_view(const op_features* f);
// total x 2 centred coordinates on the host (nullptr + error set on failure); ordered on ctx's stream
const double* op_features_coor_host(const op_features* f, op_ctx* ctx);
// the all-gather of op_sift_batch_multi and the replicas of a table on the other devices of an op_group (multi.hip)
int op_features_allgather_blocks(op_ctx* const* ctxs, int nctx, op_features* const* parts, const int* start, int n, op_features** tables);
int op_features_replicate(op_ctx* dst, const op_features* src, op_features** out);
std::vector<op_features*>& op_features_replicas(op_features* f);
int op_features_device(const op_features* f);

// match.hip
int op_matches_num_pairs(const op_matches* m);
const std::vector<int>& op_matches_counts(const op_matches* m);
const std::vector<int64_t>& op_matches_offsets(const op_matches* m);
const std::vector<int>& op_matches_limits(const op_matches* m);
const int* op_matches_host(const op_matches* m);
const int* op_matches_device(const op_matches* m, int device, hipStream_t consumer);
const std::vector<op_matches*>& op_matches_parts(const op_matches* m);
const std::vector<std::vector<int>>& op_matches_part_index(const op_matches* m);
op_matches* op_matches_merge(op_matches* const* parts, const std::vector<std::vector<int>>& index, int npairs);

// ransac.hip
op_ransac_result* op_ransac_merge(op_ransac_result* const* parts, const std::vector<std::vector<int>>& index, int npairs);

// sift_host.hip: the SIFT workspace of a context, released with it (capi.hip)
void op_ctx_release_workspace(op_ctx* c);
