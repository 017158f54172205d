// backend_launch.h — what ba.hip offers to the batched back end (backend.hip): the solve stage of Backend::OptimizeActiveMap (src/backend.cpp:208-243,
// k_ba_optimize) on device buffers, without the argument checks of the C ABI around it.  The kernel stays in its own translation unit; nothing here
// changes its arithmetic.
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

}  // namespace myslam_hip
