// orb_launch.h — what orb_kernels.hip (the extractor's kernels and their launch helpers) exports to the other units: orb_engine.hip, which
// sequences them, and calc.hip, which borrows the Gaussian.  The only declaration of each: all three units include it, so a definition
// that drifts from its declaration does not compile.
#pragma once
#include <vector>

#include "common.h"
#include "orb_plan.h"

namespace myslam_hip {

// Counters a launch clears before its own work: up to four u32 arrays of n[k] elements.  All n = 0: nothing to clear.  (The per-call
// counters are cleared by the FIRST kernel of a call instead of by hipMemsetAsync, see k_ingest.)
struct ZeroArgs { uint32_t* p[4]; int n[4]; };

// Q8 Gaussian taps (defined in orb_engine.hip).  kind 0: sigma = 2, the extractor's; kind 1: OpenCV's fixed 7-tap table (sigma <= 0)
void gauss_q8(int kind, int q[7]);

// level 0 and the per-call counters
void launch_zero_u32(const ZeroArgs& z, hipStream_t s);
void launch_ingest(const uint8_t* src, int rows, int cols, int step, size_t sstride, uint8_t* dst, int dpitch, size_t dstride, int batch,
                   const ZeroArgs& z, hipStream_t s);

// image pyramid
bool resize_uses_strips(const ResizeArgs& a);
bool resize_is_little(const ResizeArgs& a, int batch);
int resize_chain_max();
int pyr_head_levels();
void launch_resize(const ResizeArgs& a, int batch, hipStream_t s);
void launch_resize_chain(const ResizeArgs* lv, int n, int batch, hipStream_t s);
void launch_pyr_head(const ResizeArgs* lv, int n, int rows, int cols, uint8_t* dst0, int dpitch0, size_t dstride0, int b0, int batch,
                     const ZeroArgs& z, hipStream_t s);

// Gaussian pyramid
bool blur_uses_strips(const BlurArgs& a);
void launch_blur_levels(const BlurArgs* lv, int n, int batch, hipStream_t s);
bool blur_mfma_tables(int w, int h, const int q[7], std::vector<uint4>& tab, size_t& offH, size_t& offV);
void blur_mfma_ident(std::vector<uint4>& tab, size_t& offI);

// FAST, oct-tree, descriptors
void launch_fast(const OrbPlan& P, const uint8_t* pyr, size_t pyrStride, const uint8_t* maskPyr, uint32_t* cand,
                 int32_t* candCount, const uint32_t* statPrev, uint32_t* statCur, int forceMode, int batch, hipStream_t s);
size_t octree_lds_bytes(int nodeCap);
bool launch_octree(const OrbPlan& P, const uint32_t* cand, const int32_t* candCount, uint32_t* sortbuf, const uint32_t* octTab, uint32_t* selOut,
                   int32_t* selCount, int32_t* status, int batch, uint16_t* order, hipStream_t s, const BlurArgs* blurLv, int nBlur);
bool describe_uses_tile_order(bool have_order, int detectOnly, int batch);
void launch_describe(const OrbPlan& P, const uint8_t* pyr, const uint8_t* blur, size_t pyrStride, const uint32_t* selOut,
                     const int32_t* selCount, myslam_keypoint* kps, uint8_t* desc, int32_t* counts, int32_t* status,
                     int cap, int detectOnly, int batch, uint16_t* order, bool order_ready, int blocks_per_cu, hipStream_t s);
void launch_screen(const OrbPlan& P, const uint8_t* pyr, myslam_keypoint* kin, int n, myslam_keypoint* kout, uint8_t* keep,
                   hipStream_t s);
void launch_calc_desc(const OrbPlan& P, const uint8_t* blur, const myslam_keypoint* kps, int n, uint8_t* desc, hipStream_t s);

// ProcessNewKF's ORB half for a batch of key-frames (myslam_orb_process_keyframes_batch): the caller's arrays, the handle's pyramid and blurred
// blocks, and the handle's scratch — rowCap = feat_cap * nlevels screened key-points and keep flags per item
struct PkfArgs {
    const uint8_t* pyr; const uint8_t* blur; size_t pyrStride;
    const float* featXy; const int32_t* nFeat; int featCap;
    myslam_keypoint* rows; uint8_t* keep; int rowCap;
    myslam_keypoint* outKps; uint8_t* outDesc; int32_t* counts; int32_t* status; int cap;
};
// screen, compaction, descriptors: three dependent launches
void launch_process_keyframes(const OrbPlan& P, const PkfArgs& a, int batch, hipStream_t s);
void launch_unpack_cands(const uint32_t* cand, int n, int32_t* xs, int32_t* ys, int32_t* sc, hipStream_t s);

}  // namespace myslam_hip
