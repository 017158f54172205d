// frontend_launch.h — launch helpers that lk.hip and ba.hip offer to the multi-stream tracker (tracker.hip): the per-frame operators of
// Frontend::Track (LK last -> current, pose-only optimisation) on device buffers, without the argument checks of the C ABI around them.
// The kernels stay in their own translation units (and keep their compile flags); nothing here changes their arithmetic.
#pragma once
#include "common.h"

namespace myslam_hip {

// ---- lk.hip ----
// geometry of one image size for `h` (the pyramid levels of the handle's window / max_level): bytes of one image's levels >= 1 and the top level
int lk_bank_plan(myslam_lk* h, int rows, int cols, size_t* pyr_bytes, int* levels);
// levels >= 1 of `batch` images (image b at d_img + b * stride, row pitch `step`) into d_pyr [+ d_sel[b] * pyr_sel] + b * pyr_bytes; d_sel[b] < 0
// skips image b; d_sel == NULL: no selection
int lk_bank_pyramid(myslam_lk* h, const uint8_t* d_img, int step, size_t stride, uint8_t* d_pyr, int batch, const int32_t* d_sel, size_t pyr_sel);
// k_lk_track over `batch` pairs held in two equally laid out (image, pyramid) buffers img_sel / pyr_sel bytes apart: pair b tracks FROM buffer
// 1 - d_sel[b] INTO buffer d_sel[b]; d_sel[b] < 0 skips pair b.  Points as myslam_lk_track_batch.
int lk_bank_track(myslam_lk* h, const uint8_t* d_img, int step, size_t stride, const uint8_t* d_pyr, int batch, const int32_t* d_sel, size_t img_sel,
                  size_t pyr_sel, const float* d_prev_pts, float* d_next_pts, const int32_t* d_counts, int cap, uint8_t* d_status);

// ---- ba.hip ----
// k_pose_only as myslam_pose_only_optimize_batch launches it (pre_optimize 0)
int pose_only_bank_launch(double* d_poses, const double* d_pts3d, const double* d_obs, const int32_t* d_counts, int batch, int cap, double fx, double fy,
                          double cx, double cy, double chi2_th, int rounds, int iters, uint8_t* d_outlier, int32_t* d_n_inliers, int32_t* d_status,
                          hipStream_t s);
// the same kernel with pre_optimize plain optimize() calls before the rounds, for the loop closer's chain (pnp.hip): LoopClosing::OptimizeCurrentPose
int pose_only_loop_launch(double* d_poses, const double* d_pts3d, const double* d_obs, const int32_t* d_counts, int batch, int cap, double fx, double fy,
                          double cx, double cy, double chi2_th, int rounds, int iters, int pre_optimize, uint8_t* d_outlier, int32_t* d_n_inliers,
                          int32_t* d_status, hipStream_t s);

}  // namespace myslam_hip
