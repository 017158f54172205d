// backend_launch.h — what ba.hip offers to the batched back end (backend.hip): the solve stage of Backend::OptimizeActiveMap (src/backend.cpp:208-243,
// k_ba_optimize) on device buffers, without the argument checks of the C ABI around it.  The kernel stays in its own translation unit; nothing here
// changes its arithmetic.  And what backend.hip and tracker.hip offer to the mapper (mapper.hip): their launch sequences with a per-item gate.
#pragma once
#include "common.h"

namespace myslam_hip {

// scratch doubles per window as the host-pointer entry points size them: max(max_edges x 18, the HBM form's need) — with this stride the capacity clause of
// myslam_ba_optimize_batch can never trigger
size_t ba_active_map_scratch_doubles(int max_pts, int max_edges);
// k_ba_optimize as myslam_ba_optimize_active_map_batch launches it, with `scratch_stride` doubles of d_scratch per window; d_skip: nwin i32 or NULL, a
// window whose entry is not 0 is left alone (none of its arrays, its status included, is read or written)
int ba_active_map_launch(double* d_poses, double* d_points, const int32_t* d_edge_pose, const int32_t* d_edge_pt, const double* d_obs, const uint8_t* d_fixed,
                         const int32_t* d_sizes, const int32_t* d_skip, int nwin, int max_poses, int max_pts, int max_edges, double fx, double fy, double cx,
                         double cy, double huber_delta, double chi2_th, int max_rounds, int iters_per_round, double* d_scratch, size_t scratch_stride,
                         double* d_edge_chi2, uint8_t* d_outlier, int32_t* d_rounds, int32_t* d_n_outliers, int32_t* d_status, hipStream_t s);

// What backend.hip offers to the mapper (mapper.hip): the launch sequences of myslam_backend_insert_keyframe_batch and myslam_backend_optimize_batch with
// their arguments, checks and bytes, plus a per-item gate.  d_gate: batch i32 or NULL; an item whose entry is not 0 leaves k_backend_insert /
// k_backend_flatten with MYSLAM_MAPPER_IDLE before any of its tables is read: its tables keep every byte, the solve skips it (d_skip), the
// write-back's `st != 0` branch zeroes its reports and its culled count.  The two public entry points are these with a NULL gate.
int backend_insert_launch(myslam_backend* h, int64_t* d_kf_id, double* d_kf_pose, int32_t* d_n_kf, int64_t* d_mp_id, double* d_mp_pos,
                          uint8_t* d_mp_outlier, int32_t* d_n_mp, int32_t* d_obs_mp, int32_t* d_obs_kf, uint8_t* d_obs_flags,
                          float* d_obs_uv, int32_t* d_obs_tag, int32_t* d_n_obs, const int64_t* d_new_kf_id, const double* d_new_kf_pose,
                          const int64_t* d_feat_mp_id, const double* d_feat_mp_pos, const float* d_feat_uv, const int32_t* d_feat_tag,
                          const uint8_t* d_feat_flags, const int32_t* d_n_feat, int feat_cap, const int64_t* d_prior_mp_id,
                          const int64_t* d_prior_kf_id, const float* d_prior_uv, const int32_t* d_prior_tag, const uint8_t* d_prior_flags,
                          const int32_t* d_n_prior, int prior_cap, const int64_t* d_outlier_mp_id, const int32_t* d_n_outlier_mp,
                          int outlier_cap, int batch, int window, double min_dis_th, int32_t* d_feat_row, int32_t* d_mp_new_row,
                          int64_t* d_removed_kf_id, int32_t* d_removed_kf_row, double* d_dis, int32_t* d_status, const int32_t* d_gate);
int backend_optimize_launch(myslam_backend* h, const int64_t* d_kf_id, double* d_kf_pose, const int32_t* d_n_kf, int64_t* d_mp_id, double* d_mp_pos,
                            uint8_t* d_mp_outlier, int32_t* d_n_mp, int32_t* d_obs_mp, int32_t* d_obs_kf, uint8_t* d_obs_flags, float* d_obs_uv,
                            int32_t* d_obs_tag, int32_t* d_n_obs, int batch, double fx, double fy, double cx, double cy, double huber_delta,
                            double chi2_th, int max_rounds, int iters_per_round, uint8_t* d_obs_report, uint8_t* d_mp_report,
                            int32_t* d_new_outlier_mp, int32_t* d_n_new_outlier_mp, double* d_obs_chi2, int32_t* d_rounds,
                            int32_t* d_n_outlier_edges, int32_t* d_status, const int32_t* d_gate);

// What tracker.hip offers to the mapper: the handle's stream, bank size and feature cap, and myslam_tracker_update_from_map_batch with the same gate (a
// gated stream keeps every byte: its table was not touched, and the outlier flags its steps have set since are not in the table yet).
void tracker_shape(const myslam_tracker* h, hipStream_t* stream, int* streams, int* cap);
int tracker_update_from_map_launch(myslam_tracker* h, const int64_t* d_kf_id, const double* d_kf_pose, const int32_t* d_n_kf, int kf_cap,
                                   const int64_t* d_mp_id, const double* d_mp_pos, const uint8_t* d_mp_outlier, const int32_t* d_n_mp, int mp_cap,
                                   const int32_t* d_gate);

}  // namespace myslam_hip
