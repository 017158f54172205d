/*
 * myslam_hip.h — C ABI of libmyslam_hip.so: the MI355X (gfx950) implementation of the per-frame
 * dense path of "A Simple Stereo SLAM System with Deep Loop Closing".
 *
 * The reference has no FFI/plugin layer: the path sits behind C++ member functions of libmyslam.so
 * (SURVEY.md §8b).  Each entry point below names the reference interface it replaces
 * (file:line under the reference tree).  A maintainer's binding is shown in INTEGRATION.md; the
 * C++ facade with the reference's own class names lives in <pkg>/host/.
 *
 * Conventions: caller-owned buffers; plain pointers and sizes; int status (0 = ok, <0 = error);
 * no exceptions cross the ABI.  "_batch" entry points take DEVICE pointers, are asynchronous on
 * the handle's HIP stream and never synchronise; the others take HOST pointers and return when the
 * result is in the caller's buffers.  There is NO CPU fallback: every call fails with
 * MYSLAM_ERR_HIP when no gfx950 device is usable.
 *
 * Threading: a handle owns device scratch and one HIP stream, so it serves one thread at a time; handle-free functions are
 * re-entrant.  The reference shares ONE ORBextractor between the frontend and the loop-closing thread (src/system.cpp:31,54,66):
 * create one handle per thread instead.  Work of different handles on different streams runs concurrently on the device.
 */
#ifndef MYSLAM_HIP_H
#define MYSLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MYSLAM_OK 0
#define MYSLAM_ERR_INVALID (-1)     /* bad argument */
#define MYSLAM_ERR_HIP (-2)         /* HIP runtime error / no device */
#define MYSLAM_ERR_CAPACITY (-3)    /* an output or internal buffer was too small */
#define MYSLAM_ERR_UNSUPPORTED (-4) /* image too small for the 30-px FAST grid etc. */

/* cv::KeyPoint layout (28 bytes): pt.x pt.y size angle response octave class_id */
typedef struct myslam_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} myslam_keypoint;

#define MYSLAM_DESC_BYTES 32   /* 256-bit rBRIEF */
#define MYSLAM_LCD_DIM 1064    /* DeepLCD::DescrVector, include/myslam/deeplcd.h:25 */

/* ------------------------------------------------------------------------------------------
 * Library-wide
 * ------------------------------------------------------------------------------------------ */
int myslam_hip_device_count(void);
/* "myslam_hip <version> (gfx950) build <digest>": the digest covers every source file the library was built from (build.py), so a measurement
 * file can name the build it was taken on (profiles/r<NN>_pmc_*.json "build_id"; bench.py sets roofline.traffic_stale when it differs) */
const char* myslam_hip_version(void);
/* The shader clock the device runs at NOW: one wave spins for spin_us (0 < spin_us <= 1e6) on the given stream and compares the shader cycle counter
 * with the constant 100 MHz counter; synchronises the stream.  bench.py samples it around its timed regions ("clock_mhz"): box-to-box and
 * run-to-run differences of a few per cent are clock states more often than code */
int myslam_prof_shader_clock_mhz(void* hip_stream, float spin_us, float* mhz);
/* per-kernel HIP-event timing: enable, run, synchronise, then read (name, total ms, launches) */
int myslam_prof_enable(int on);
int myslam_prof_reset(void);
int myslam_prof_count(void);
int myslam_prof_get(int i, const char** name, double* total_ms, long* launches);
/* debug: device->host copy of n bytes through this library's HIP runtime */
int myslam_debug_peek(const void* d_ptr, void* out, size_t n);

/* ------------------------------------------------------------------------------------------
 * ORB extractor — replaces class ORBextractor (include/myslam/ORBextractor.h:52-110)
 * ------------------------------------------------------------------------------------------ */
typedef struct myslam_orb myslam_orb;

/* ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)  ORBextractor.h:55-56 */
int myslam_orb_create(myslam_orb** out, int nfeatures, float scale_factor, int nlevels,
                      int ini_th_fast, int min_th_fast);
int myslam_orb_destroy(myslam_orb* h);
/* all work of this handle is ordered on `hip_stream` (a hipStream_t; NULL = default stream).  The batched extractor may run its
 * Gaussian-pyramid launches on an internal stream; they are fenced by events against `hip_stream` on both sides, so for the caller
 * every call still starts after, and completes before, its neighbours on `hip_stream`. */
int myslam_orb_set_stream(myslam_orb* h, void* hip_stream);
/* pipelining aid for callers that run several extractor handles on several streams (two cameras, or the left and the right images
 * of a batch of stereo pairs): `hip_event` (a hipEvent_t, NULL = off) is
 * recorded on the handle's stream right after the grid-FAST stage of every following batched call.  FAST is the VALU-bound
 * stage, the oct-tree / descriptor stages after it are latency-bound: a second handle whose stream waits for this event runs its
 * own FAST under them instead of beside the first handle's FAST.  No reference counterpart (scheduling only). */
int myslam_orb_set_fast_event(myslam_orb* h, void* hip_event);
/* the matching gate: before the grid-FAST stage of every following batched call the handle's stream waits for `hip_event`
 * (a hipEvent_t, NULL = off) as it was last recorded when the call is made; the pyramid stages before FAST are not held back.
 * Two handles that gate each other with their fast events take turns on the VALU-bound stage. */
int myslam_orb_set_fast_gate(myslam_orb* h, void* hip_event);
/* scheduling / debugging knobs of a handle (no reference counterpart; none of them changes a result):
 *   FAST_MODE        -1 (default) = the grid-FAST kernel picks its path per pyramid level from what the handle's previous launch measured:
 *                    a compass pre-test + compaction of the surviving pixel pairs (imagery with a few % of corners: a tenth of the pixels
 *                    is scored) or full scoring of every pixel (noise-like texture where most pairs survive the pre-test);
 *                    0 / 1 force the two-phase / the dense path
 *   INTERNAL_STREAM  1 (default) = the Gaussian pyramid runs on an internal stream beside the oct-tree kernel (forked after FAST),
 *                    2 = forked right after the image pyramid (beside FAST), 0 = everything on the handle's stream
 *   COPY_INPUT       0 (default) = a *_batch call reads the full-resolution level of every image but the last IN PLACE (no copy into the
 *                    pyramid block): the input buffer must then stay unchanged until the call has completed on the handle's stream;
 *                    1 = every image is copied first, the input may be overwritten as soon as the copy kernel has run
 *   STOP_AFTER       debug: a batched call returns after stage 1 ingest / 2 pyramid / 3 oct-tree / 4 blur (0 = complete call)
 *   BLUR_MFMA        1 = the 7 x 7 Gaussian pyramid runs on the int8 matrix cores (two banded Toeplitz products per 32 x 32 tile, bit-identical
 *                    to the register-strip kernel; levels narrower than 64 columns or tap tables with a folded coefficient above 127 keep
 *                    the strip kernel), 0 = register-strip kernel on the vector units.  The step is VALU-issue bound: see DESIGN.md section 6
 *   SIDE_BLOCKS_PER_CU  n > 0: the descriptor kernel of a batched call is launched as a LIMITED grid of 256 n blocks, each walking several
 *                    (image, 64-key-point chunk) work items.  For callers that run two handles beside each other: a descriptor block lives
 *                    three times as long as a FAST block, so an unlimited grid gradually takes the CUs from the other handle's FAST launch —
 *                    the VALU-bound kernel starves under the latency-bound one (measured: 7.12 -> 7.02 ms per 512-pair step with n = 2, round 4).
 *                    Since the kernel fetches its BRIEF windows by LDS-DMA (end of round 6) its blocks are short and the unlimited grid measures
 *                    faster (6.25 -> 6.09 ms): 0 (default) = one block per work item */
#define MYSLAM_ORB_OPT_FAST_MODE 1
#define MYSLAM_ORB_OPT_INTERNAL_STREAM 2
#define MYSLAM_ORB_OPT_STOP_AFTER 3
#define MYSLAM_ORB_OPT_COPY_INPUT 4
#define MYSLAM_ORB_OPT_BLUR_MFMA 5
#define MYSLAM_ORB_OPT_SIDE_BLOCKS_PER_CU 6
int myslam_orb_set_option(myslam_orb* h, int option, int value);
/* The 7 x 7 sigma = 2 Gaussian before rBRIEF (ORBextractor.cpp:966, :1197) runs in OpenCV's 8-bit fixed-point form; how OpenCV 3.4.8
 * rounds the taps to Q8 could not be checked in the build environment (parity unpinned).  Default
 * [18,34,49,55,49,34,18]: every normalised tap rounded to nearest on its own, as getFixedpointGaussianKernel of the 3.4.8 era does —
 * the sum is 257 and the u8 result saturates as ufixedpoint32 -> uint8_t does.  A maintainer who measures another table with
 * tools/dump_opencv_goldens.py sets it here (7 ints, 0..255, sum 1..257 so that the Q8.8 row sums fit 16 bits; NULL restores the
 * default; [18,34,49,54,49,34,18] is the sum-256 table rounds 1-2 of this library used). */
int myslam_orb_set_gauss_taps(myslam_orb* h, const int32_t* q7);
/* getters ORBextractor.h:87-107 */
int myslam_orb_get_tables(const myslam_orb* h, float* scale, float* inv_scale, int* features_per_level, int* umax16);
/* upper bound of keypoints DetectAndCompute / Detect can return for one image: sum over levels of
 * max(N_level + 3, 32) — the oct-tree stops only after a split pushed it to >= N, and its first round is unconditional */
int myslam_orb_max_keypoints(const myslam_orb* h);
/* the same bound for one image size, exact for ANY aspect ratio (a level with nIni = round(width/height) root nodes can return
 * 4*nIni key-points even when its budget is smaller, ORBextractor.cpp:645-716); use it to size kps / desc for that size */
int myslam_orb_max_keypoints_for(const myslam_orb* h, int rows, int cols);

/* void DetectAndCompute(image, mask, keypoints, descriptors)   ORBextractor.h:61-63, .cpp:922-985
 * mask may be NULL (= all 255).  desc: cap x 32 bytes. */
int myslam_orb_detect_and_compute(myslam_orb* h, const uint8_t* img, int rows, int cols, int step,
                                  const uint8_t* mask, int mask_step,
                                  myslam_keypoint* kps, uint8_t* desc, int cap, int* n);
/* void Detect(image, mask, keypoints)   ORBextractor.h:70-71, .cpp:989-1074 (level 0 only) */
int myslam_orb_detect(myslam_orb* h, const uint8_t* img, int rows, int cols, int step,
                      const uint8_t* mask, int mask_step, myslam_keypoint* kps, int cap, int* n);
/* void ScreenAndComputeKPsParams(image, keypoints, out_keypoints)   ORBextractor.h:83-84, .cpp:1083-1129
 * kps_in is modified in place exactly as the reference does (pt /= scale ... pt *= scale). */
int myslam_orb_screen_and_compute_params(myslam_orb* h, const uint8_t* img, int rows, int cols, int step,
                                         myslam_keypoint* kps_in, int n_in,
                                         myslam_keypoint* kps_out, int cap, int* n_out);
/* void CalcDescriptors(image, keypoints, descriptors)   ORBextractor.h:65-67, .cpp:1180-1226 */
int myslam_orb_calc_descriptors(myslam_orb* h, const uint8_t* img, int rows, int cols, int step,
                                const myslam_keypoint* kps, int n, uint8_t* desc);

/* Batched DetectAndCompute over `batch` same-sized images resident in HBM.
 *   d_imgs : batch images, image b at d_imgs + b*img_stride, row pitch `step` bytes
 *   d_masks: NULL or same layout
 *   d_kps  : batch x cap keypoints, d_desc: batch x cap x 32, d_counts: batch
 *   d_status: batch int32 (0 ok / MYSLAM_ERR_CAPACITY), may be NULL
 * level_only0 != 0 runs Detect() semantics (level 0, N = nfeatures, no angle/descriptor). */
int myslam_orb_detect_and_compute_batch(myslam_orb* h, const uint8_t* d_imgs, int batch, int rows, int cols,
                                        int step, size_t img_stride, const uint8_t* d_masks,
                                        myslam_keypoint* d_kps, uint8_t* d_desc, int32_t* d_counts,
                                        int32_t* d_status, int cap);
int myslam_orb_detect_batch(myslam_orb* h, const uint8_t* d_imgs, int batch, int rows, int cols,
                            int step, size_t img_stride, const uint8_t* d_masks,
                            myslam_keypoint* d_kps, int32_t* d_counts, int32_t* d_status, int cap);

/* The ORB half of LoopClosing::ProcessNewKF (src/loopclosing.cpp:93-113) for `batch` key-frames of one image size on the device: what
 * myslam_expand_pyramid_keypoints -> myslam_orb_screen_and_compute_params (ORBextractor.cpp:1083-1129) -> myslam_orb_calc_descriptors
 * (ORBextractor.cpp:1180-1226) give per key-frame through the host, bit for bit, written where myslam_loop_match_batch reads it: mvPyramidKeyPoints
 * (its d_loop_pyr / d_cur_pyr), mORBDescriptors (d_loop_desc / d_cur_desc) and their count (d_n_loop / d_n_cur).  Images as in
 * myslam_orb_detect_and_compute_batch; every image is copied into the handle's pyramid block by the first launch.  Per item b:
 *   expansion    feature i < n_feat, level l < nlevels, in that order: octave = l, response = -1, class_id = i (:94-105).  Only the feature's pixel
 *                comes from the caller (d_feat_xy, the layout of myslam_loop_match_batch's d_cur_feat_xy);
 *   screening    a row is kept when pt / scale[l] passes the float border test (19 pixels) and isFastCorner(minThFAST) (:1098-1127); NaN and
 *                +-inf coordinates fail the border test, as the reference's !(...) does.  A kept row has pt = (pt / scale) * scale in float,
 *                size = 31 * scale[l], angle = IC_Angle on the level's image;
 *   order        kept rows in input order — feature-major, level-minor — as out_keypoints.push_back leaves them (:1125);
 *   descriptors  of the kept rows on the blurred pyramid (:1194-1223);
 *   d_counts[b]  the number of kept rows; all 28 bytes of a key-point and the 32 of a descriptor are written below it, slots from it on are
 *                left as they were;
 *   d_n_feat[b]  below 0 reads as 0, above feat_cap as feat_cap; slots of d_feat_xy from the count on are never read.  n_feat = 0: count 0,
 *                status 0 (the reference logs and returns);
 *   d_status[b]  0, or MYSLAM_ERR_CAPACITY when more rows are kept than `cap`: then d_counts[b] = 0 and none of the item's rows are written
 *                (nothing is truncated).  Other items are unaffected.
 * The DeepLCD half is not run here: calcDescrOriginalImg blurs the key-frame's image in place BEFORE the ORB half reads it (:91,
 * deeplcd.cpp:46), so a caller that reproduces ProcessNewKF enqueues myslam_lcd_describe_batch(..., blur_in_place = 1, ...) on the same stream
 * first and passes the same d_imgs.
 * Call level, nothing enqueued: NULL pointers, batch / rows / cols / feat_cap / cap <= 0 or step < cols -> MYSLAM_ERR_INVALID; an image size the
 * extractor's plan refuses -> MYSLAM_ERR_UNSUPPORTED; batch > 65535, feat_cap * nlevels > 2^24 or cap > 2^24 (launch grid) -> MYSLAM_ERR_CAPACITY.
 * Runs on the handle's stream; shares the handle's pyramid and blurred blocks with the other *_batch calls and leaves their results as they
 * were.  Scratch (feat_cap * nlevels screened key-points and flags per item) lives in the handle: after one call at a given (batch, shape,
 * feat_cap) a repeat allocates nothing, never synchronises and reads no device memory from the host — recordable between
 * myslam_graph_begin / _end on one stream. */
int myslam_orb_process_keyframes_batch(myslam_orb* h,
        const uint8_t* d_imgs, int batch, int rows, int cols, int step, size_t img_stride,   /* as myslam_orb_detect_and_compute_batch */
        const float* d_feat_xy,        /* batch x feat_cap x 2: mvpFeaturesLeft[i]->mkpPosition.pt (the layout of loop_match_batch's d_cur_feat_xy) */
        const int32_t* d_n_feat,       /* batch */
        int feat_cap,
        myslam_keypoint* d_pyr_kps,    /* batch x cap: mvPyramidKeyPoints, item b at + b*cap */
        uint8_t* d_desc,               /* batch x cap x 32: mORBDescriptors */
        int32_t* d_counts, int32_t* d_status /* batch each */, int cap);

/* debug/inspection taps used by the stage-level parity tests (host buffers, one image) */
int myslam_orb_debug_pyramid(myslam_orb* h, const uint8_t* img, int rows, int cols, int step,
                             int level, int blurred, uint8_t* out, int out_step, int* w, int* hgt);
int myslam_orb_debug_candidates(myslam_orb* h, const uint8_t* img, int rows, int cols, int step,
                                const uint8_t* mask, int mask_step, int level,
                                int32_t* xs, int32_t* ys, int32_t* scores, int cap, int* n);

/* raw readback of the engine's HBM buffers after a *_batch call: what = 0 pyramid plane (w*h, tight), 1 blurred
 * plane, 2 candidate count (i32), 3 candidate payloads (u32 py<<20|px<<8|score), 4 selected count, 5 selected payloads,
 * 6 the grid-FAST statistics of the last launch on `level`: 4 x u32 {pixel pairs that survived the pre-test (two-phase path) or 4-pixel
 * rows holding a corner (dense path), pixel pairs looked at — both over the sampled strips —, path used (0 two-phase, 1 dense), 0} */
int myslam_orb_debug_readback(myslam_orb* h, int what, int b, int level, void* out, size_t cap_bytes, int detect_plan);

/* ------------------------------------------------------------------------------------------
 * Hamming brute force — replaces cv::BFMatcher(NORM_HAMMING)::match as used at
 * src/loopclosing.cpp:33,172 and the filter at :175-194.  One match per query row, ties -> lowest
 * train index.  nt == 0 -> train_idx = -1, dist = -1.
 * ------------------------------------------------------------------------------------------ */
int myslam_hamming_match(const uint8_t* query, int nq, const uint8_t* train, int nt,
                         int32_t* train_idx, int32_t* dist);
/* batch: pair p uses d_q + p*cap*32 (d_nq[p] rows) vs d_t + p*cap*32 (d_nt[p] rows).  A count above cap acts as cap; a negative
 * d_nq[p] writes nothing for that pair; a negative d_nt[p] acts as 0 (train_idx = -1, dist = -1 for each of the pair's query rows).
 * Slots past a pair's query count are never written.  A train index takes 20 bits beside the distance: nt >= 2^20 (single call) and
 * cap >= 2^20 (batch) return MYSLAM_ERR_UNSUPPORTED before anything is launched; 2^20 - 1 rows are accepted. */
int myslam_hamming_match_batch(const uint8_t* d_q, const int32_t* d_nq, const uint8_t* d_t, const int32_t* d_nt,
                               int batch, int cap, int32_t* d_train_idx, int32_t* d_dist, void* hip_stream);
/* keep[i] = dist[i] <= max(2*min_dist, 30.0)   (loopclosing.cpp:175-186); host-side bookkeeping */
int myslam_hamming_filter(const int32_t* dist, int n, uint8_t* keep, int* min_dist);

/* Key-frame / feature bookkeeping of the loop closer around the two calls above (KeyFrame::mvPyramidKeyPoints,
 * cv::KeyPoint::class_id as the feature index).  Host functions, no device work.
 * expand: LoopClosing::ProcessNewKF src/loopclosing.cpp:94-105 — out[i * nlevels + l] = feats[i] with octave = l, response = -1,
 *         class_id = i (the input of myslam_orb_screen_and_compute_params).
 * pairs : LoopClosing::MatchFeatures :175-194 — matches with distance <= max(2 * min_dist, 30) mapped to (current feature id, loop
 *         feature id) through class_id, de-duplicated and ordered as the reference's std::set<std::pair<int,int>> iterates. */
int myslam_expand_pyramid_keypoints(const myslam_keypoint* feats, int n, int nlevels, myslam_keypoint* out);
int myslam_match_feature_pairs(const int32_t* train_idx, const int32_t* dist, int n_query, const myslam_keypoint* loop_pyr_kps,
                               const myslam_keypoint* cur_pyr_kps, int n_train, int32_t* pairs, int* n_pairs);

/* LoopClosing::MatchFeatures (src/loopclosing.cpp:167-203) and the point gather at the top of LoopClosing::ComputeCorrectPose (:210-253) for `batch`
 * (current key-frame, loop key-frame) candidates on the device: everything between "the database names a loop key-frame" and
 * myslam_loop_verify_batch, whose d_pts3d / d_pts2d / d_counts it writes (out_cap = that handle's cap).  Two dependent launches on hip_stream —
 * the matcher exactly as myslam_hamming_match_batch launches it (query = loop, train = current, :172), then one workgroup per item — nothing
 * allocated, nothing synchronised, no device memory read from the host: recordable between myslam_graph_begin / _end.  Per item b:
 *   d_train_idx, d_dist   the matcher's output, the bits of myslam_hamming_match_batch;
 *   kept rows             (double)dist <= max(2.0 * min_dist, 30.0) with min_dist over the item's n_loop rows (:175-183);
 *   d_pairs, d_n_pairs    every kept row as (cur_pyr[train_idx].class_id, loop_pyr[row].class_id), duplicates collapsed, ascending current id then
 *                         loop id: _msetValidFeatureMatches as the reference's std::set<std::pair<int,int>> iterates (:184-194), and its size;
 *   fewer than min_matches (10 at :198) pairs: MatchFeatures returns false — d_status[b] = MYSLAM_LOOP_MATCH_FEW_PAIRS, d_counts[b] = 0;
 *   d_valid_pairs, d_pts2d, d_pts3d, d_counts   otherwise the set is walked in order and pairs whose loop feature has no map point
 *                         (d_loop_feat_landmark = -1: mpMapPoint.lock() is null) leave it (:218-237); survivor k keeps its pair, takes the current
 *                         feature's pixel (:223-224) and (float) of the landmark's f64 position, rounded to nearest even as cv::Point3f(pos(0),
 *                         pos(1), pos(2)) does (:225-226); d_counts[b] = the number of survivors.  Fewer than min_matches (10 at :252):
 *                         MYSLAM_LOOP_MATCH_FEW_POINTS, count and arrays still written; else MYSLAM_LOOP_MATCH_OK.
 * n_loop == 0 or n_cur == 0: the reference dereferences the end of an empty range (:175-177); here that item has zero pairs (FEW_PAIRS).
 * Counts above cap are read as cap, counts below 0 as 0; slots from an item's count on are never read, and class_id is the only field read of a
 * pyramid key-point, for kept rows only.  Output slots from the written count on are left as they were.  Per-item errors, each with d_counts[b] = 0
 * and nothing else of that stage written: MYSLAM_ERR_INVALID — a class_id outside [0, feat_cap) (then d_n_pairs[b] = 0 too) or a landmark slot outside
 * [-1, landmark_cap); MYSLAM_ERR_CAPACITY — more survivors than out_cap (nothing is truncated).  Other items are unaffected.
 * Call-level, nothing enqueued: NULL pointers, batch / cap / out_cap / feat_cap <= 0, landmark_cap < 0 -> MYSLAM_ERR_INVALID; cap > 16384 (one item's keys are sorted in
 * LDS), feat_cap > 65536 (a feature id is half a 32-bit key), out_cap > 4096 (myslam_pnp_create's limit) -> MYSLAM_ERR_CAPACITY. */
#define MYSLAM_LOOP_MATCH_OK 0
#define MYSLAM_LOOP_MATCH_FEW_PAIRS 1
#define MYSLAM_LOOP_MATCH_FEW_POINTS 2
int myslam_loop_match_batch(
    const uint8_t* d_loop_desc, const int32_t* d_n_loop,      /* query: loop KF's mORBDescriptors, item b at + b*cap*32 */
    const uint8_t* d_cur_desc,  const int32_t* d_n_cur,       /* train: current KF's */
    const myslam_keypoint* d_loop_pyr, const myslam_keypoint* d_cur_pyr,   /* mvPyramidKeyPoints, item b at + b*cap; only class_id is read */
    int batch, int cap,
    const float*   d_cur_feat_xy,          /* batch x feat_cap x 2: mvpFeaturesLeft[i]->mkpPosition.pt of the current KF */
    const int32_t* d_loop_feat_landmark,   /* batch x feat_cap: slot in the item's landmark table, -1 = mpMapPoint.lock() is null */
    int feat_cap,
    const double*  d_landmark_pos, size_t landmark_stride, int landmark_cap,   /* item b's table at + b*landmark_stride*3 doubles; stride 0 = one shared table */
    int min_matches, int out_cap,
    int32_t* d_train_idx, int32_t* d_dist,         /* batch x cap: the matcher's output, as myslam_hamming_match_batch writes it */
    int32_t* d_pairs, int32_t* d_n_pairs,          /* batch x cap x 2 (current id, loop id) in std::set order; the set's size after :194 */
    int32_t* d_valid_pairs,                        /* batch x out_cap x 2: the pairs that survive :218-237, same order */
    float* d_pts3d, float* d_pts2d, int32_t* d_counts,   /* batch x out_cap x 3 / x 2 / batch: verify_batch's inputs */
    int32_t* d_status, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * Loop key-frame store and the decision of LoopClosing::DetectLoop on the device — what lies between myslam_lcddb_query_batch's three outputs and
 * myslam_loop_match_batch's loop-side inputs: `if (maxScore < 0.94 || cntSuspected > 3) return false` (src/loopclosing.cpp:147, the whole function
 * :124-161) and `_mpLoopKF = _mvDatabase.at(bestId)` (:151) with what that key-frame holds (include/myslam/keyframe.h: mvPyramidKeyPoints,
 * mORBDescriptors, and for every feature of mvpFeaturesLeft whether mpMapPoint.lock() still names a landmark).
 *
 * The store has kf_capacity slots of `cap` key-points (all 28 bytes), cap x 32 descriptor bytes, a row count, feat_cap landmark slots and a feature
 * count; slot s is the s-th key-frame put.  Nothing ever moves and nothing grows, so a recorded step that names the store stays valid.  Ids ascend, as
 * the loop database's do, and are kept on the host and in a device array.
 *
 * put_batch: `batch` key-frames as myslam_orb_process_keyframes_batch left them (d_pyr_kps, d_desc, d_counts, item b at + b*cap; d_kf_status = its
 * d_status or NULL) plus the feature -> landmark table in myslam_loop_match_batch's d_loop_feat_landmark layout (batch x feat_cap, -1 = no map point)
 * and its count.  ids (host): strictly ascending and above every id held, else MYSLAM_ERR_INVALID; size + batch > kf_capacity: MYSLAM_ERR_CAPACITY; in
 * both cases nothing is stored or enqueued and the store answers later calls as before.  Counts are read on the device: d_counts[b] below 0 reads as 0,
 * above cap as cap; d_kf_status[b] != 0 stores the key-frame with 0 rows (the reference keeps such a key-frame, and it matches nothing); d_n_feat[b] is
 * clamped to [0, feat_cap]; only rows and entries below the counts are read.  Enqueues on the handle's stream and does not wait; the caller's arrays
 * may be reused once that work is done.  Like myslam_lcddb_append_batch_async it is host bookkeeping as well and cannot be replayed:
 * MYSLAM_ERR_UNSUPPORTED, before anything is enqueued, while the handle's stream is being captured (the capture stays usable).
 *
 * set_landmarks_batch: replaces the feature -> landmark table and feature count of n key-frames already held (mpMapPoint.lock() goes null when the map
 * removes or fuses a point; that bookkeeping stays with the caller).  An id that is not held, or named twice: MYSLAM_ERR_INVALID, nothing enqueued.
 * Same stream, capture and clamping rules as put_batch.
 *
 * detect_batch: ONE launch on the handle's stream; allocates nothing, never synchronises, reads no device memory from the host: recordable between
 * myslam_graph_begin / _end.  Ids, counts and the number of key-frames held are read on the device, so a replay sees key-frames put after the
 * recording.  d_best_id / d_max_score / d_cnt are myslam_lcddb_query_batch's outputs (nq each).  Per item b:
 *   1. d_max_score[b] < thr_high || d_cnt[b] > max_suspected, f32 and i32 compares, the reference's expression literally (0.94f and 3 at :147):
 *      d_status[b] = MYSLAM_LOOP_DETECT_NO_LOOP, d_n_loop[b] = 0, d_loop_slot[b] = -1, no other byte of the item is written.  A NaN score is not
 *      "less", exactly as in the reference, so it goes on to step 2; thr_high = +inf rejects every item with a finite score, which is how a recorded
 *      step is switched off while the database is below the reference's size gate;
 *   2. d_best_id[b] is looked up among the ids held; not held: d_status[b] = MYSLAM_ERR_INVALID, d_n_loop[b] = 0, d_loop_slot[b] = -1, no other byte
 *      of the item is written;
 *   3. d_status[b] = MYSLAM_LOOP_DETECT_CANDIDATE, d_loop_slot[b] = the slot, d_n_loop[b] = the stored row count; that many key-points (item b at
 *      d_loop_pyr + b*cap) and descriptors (d_loop_desc + b*cap*32) and the stored number of landmark entries (d_loop_feat_landmark + b*feat_cap) are
 *      copied.  Output slots from the counts on are left as they were.
 * A rejected item carries n_loop = 0: myslam_loop_match_batch answers MYSLAM_LOOP_MATCH_FEW_PAIRS for it, myslam_loop_verify_batch
 * MYSLAM_VERIFY_FEW_MATCHES and myslam_loop_correct_batch MYSLAM_LOOP_CORRECT_SKIPPED, so the chain needs no compaction between its stages.
 * The gate `_mvDatabase.size() > _mnDatabaseMinSize` (:62) and AddToDatabase for the items that end unconfirmed are on the device for a bank of
 * streams: myslam_lcdbank_query_batch gates each stream by its own row count (a gated or idle item carries a score of 0 and ends NO_LOOP here) and
 * myslam_lcdbank_append_batch adds the rows the caller selects.  With the single myslam_lcddb both stay with the caller (see thr_high = +inf above).
 *
 * Call level, nothing enqueued: NULL pointers (d_kf_status excepted), nq / batch / n / kf_capacity / cap / feat_cap <= 0 -> MYSLAM_ERR_INVALID;
 * cap > 16384, feat_cap > 65536 (myslam_loop_match_batch's limits) or nq > 65535 -> MYSLAM_ERR_CAPACITY; create out of device memory ->
 * MYSLAM_ERR_CAPACITY, any other allocation failure -> MYSLAM_ERR_HIP.
 * ------------------------------------------------------------------------------------------ */
typedef struct myslam_loop_store myslam_loop_store;
int myslam_loop_store_create(myslam_loop_store** out, int kf_capacity, int cap, int feat_cap);
int myslam_loop_store_destroy(myslam_loop_store* h);
int myslam_loop_store_set_stream(myslam_loop_store* h, void* hip_stream);
int myslam_loop_store_size(const myslam_loop_store* h);        /* key-frames held */
int myslam_loop_store_capacity(const myslam_loop_store* h);
int myslam_loop_store_put_batch(myslam_loop_store* h, const uint64_t* ids /*host*/, int batch,
        const myslam_keypoint* d_pyr_kps, const uint8_t* d_desc, const int32_t* d_counts,   /* process_keyframes_batch's outputs, item b at + b*cap */
        const int32_t* d_kf_status,            /* its d_status, may be NULL */
        const int32_t* d_feat_landmark,        /* batch x feat_cap, the layout of loop_match_batch's d_loop_feat_landmark */
        const int32_t* d_n_feat);              /* batch */
int myslam_loop_store_set_landmarks_batch(myslam_loop_store* h, const uint64_t* ids /*host*/, int n,
        const int32_t* d_feat_landmark, const int32_t* d_n_feat);
#define MYSLAM_LOOP_DETECT_CANDIDATE 0
#define MYSLAM_LOOP_DETECT_NO_LOOP   1
int myslam_loop_detect_batch(myslam_loop_store* h,
        const uint64_t* d_best_id, const float* d_max_score, const int32_t* d_cnt, int nq,   /* myslam_lcddb_query_batch's outputs */
        float thr_high, int max_suspected,                                                   /* 0.94f and 3 at loopclosing.cpp:147 */
        uint8_t* d_loop_desc, int32_t* d_n_loop, myslam_keypoint* d_loop_pyr, int32_t* d_loop_feat_landmark,   /* loop_match_batch's inputs, item b at + b*cap (+ b*feat_cap) */
        int32_t* d_loop_slot, int32_t* d_status);                                            /* nq each */

/* ------------------------------------------------------------------------------------------
 * Triangulation — replaces triangulation() include/myslam/algorithm.h:16-33 with the stereo rig
 * of src/system.cpp:108-116,141-145 and Camera::pixel2camera src/camera.cpp:22-26.
 * ok[i] = (sigma3/sigma2 < 1e-2) && z > 0   (frontend.cpp:400, 471).
 * ------------------------------------------------------------------------------------------ */
int myslam_triangulate_stereo(const float* xl, const float* yl, const float* xr, const float* yr, int n,
                              double fx, double fy, double cx, double cy, double baseline,
                              double* xyz, uint8_t* ok);
/* batch: left keypoint i of pair p is matched to right keypoint d_match[p*cap+i].  An index below 0 or at or above cap means "no
 * match": ok = 0, xyz = 0.  An index in [number of right key-points, cap) is NOT an error: that slot of d_kps_r is read as it is, so
 * the caller keeps every slot readable.  Only x and y of a record are read.  d_nl[p] above cap acts as cap, a negative one writes
 * nothing; slots past it are never written.  A non-finite coordinate gives ok = 0 (xyz unspecified). */
int myslam_triangulate_stereo_batch(const myslam_keypoint* d_kps_l, const myslam_keypoint* d_kps_r,
                                    const int32_t* d_match, const int32_t* d_nl, int batch, int cap,
                                    double fx, double fy, double cx, double cy, double baseline,
                                    double* d_xyz, uint8_t* d_ok, void* hip_stream);

/* cv::BFMatcher::match (src/loopclosing.cpp:172-173) followed by triangulation() (include/myslam/algorithm.h:16-33) of every matched left
 * key-point, as Frontend::FindFeaturesInRight + TriangulateNewPoints do in sequence (src/frontend.cpp:344-420): exactly
 * myslam_hamming_match_batch(d_q = left descriptors, d_t = right descriptors, ...) and then myslam_triangulate_stereo_batch(d_kps_l, d_kps_r,
 * d_train_idx, d_nq, ...) — same outputs, bit for bit.  For fewer than 16 pairs per call it is ONE launch (each matcher block triangulates
 * its 128 queries once their matches are known): a live stream's step is bound by the number of its dependent launches. */
int myslam_hamming_match_triangulate_batch(const uint8_t* d_q, const int32_t* d_nq, const uint8_t* d_t, const int32_t* d_nt,
                                           const myslam_keypoint* d_kps_l, const myslam_keypoint* d_kps_r, int batch, int cap,
                                           double fx, double fy, double cx, double cy, double baseline,
                                           int32_t* d_train_idx, int32_t* d_dist, double* d_xyz, uint8_t* d_ok, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * DeepLCD — replaces class DeepLCD (include/myslam/deeplcd.h:21-48, src/deeplcd.cpp:10-91)
 *
 * The model is DATA: a list of layer records (what calc_model/deploy.prototxt says) + the convolution weights (what
 * calc_model/calc.caffemodel holds).  Three sources:
 *   myslam_lcd_create_from_caffe  the reference's two files, read by a dependency-free parser (host/myslam_caffe.hpp)
 *   myslam_lcd_create_from_layers records + flat weights from the caller
 *   myslam_lcd_create / _from_file the SURVEY A.6 layer list (myslam_lcd_default_layers) + a flat blob / the CALCW1 / CALCW2 files
 * weights: flat f32, per Convolution layer in order: w[OC][IC][K][K] then b[OC] (Caffe's blob order).  For the default list:
 *          conv1.w[64][1][5][5] conv1.b[64] conv2.w[128][64][4][4] conv2.b[128] conv3.w[4][128][3][3] conv3.b[4] (137476 floats).
 * Supported layers: Convolution (square kernel, group 1, with bias), ReLU, Pooling MAX (Caffe ceil mode, pad 0), LRN ACROSS_CHANNELS;
 * input 1 x 120 x 160 (the reference resizes every frame to that, deeplcd.cpp:50); 1064 outputs (deeplcd.cpp:80 asserts it).
 * Anything else: MYSLAM_ERR_UNSUPPORTED.  A list with the SURVEY A.6 geometry (any LRN alpha / beta / k, ReLUs present or not) runs
 * on fused kernels; other lists run layer by layer on generic kernels (myslam_lcd_uses_fused_kernels tells which).
 * ------------------------------------------------------------------------------------------ */
#define MYSLAM_CALC_CONV 1
#define MYSLAM_CALC_RELU 2
#define MYSLAM_CALC_POOL_MAX 3
#define MYSLAM_CALC_LRN 4
typedef struct myslam_calc_layer {
    int32_t type;                              /* MYSLAM_CALC_* */
    int32_t num_output, kernel, stride, pad;   /* Convolution (convolution_param); Pooling uses kernel / stride / pad (pooling_param) */
    int32_t local_size;                        /* LRN (lrn_param): y = x * (k + alpha / local_size * sum x^2)^-beta */
    float alpha, beta, k;
} myslam_calc_layer;
typedef struct myslam_lcd myslam_lcd;
/* the SURVEY A.6 list (10 records); layers == NULL returns the count only */
int myslam_lcd_default_layers(myslam_calc_layer* layers, int cap);
int myslam_lcd_create(myslam_lcd** out, const float* weights, size_t nweights);
int myslam_lcd_create_from_layers(myslam_lcd** out, const myslam_calc_layer* layers, int nlayers, const float* weights, size_t nweights);
/* DeepLCD::DeepLCD(prototxt_path, caffemodel_path, gpu_id)  deeplcd.h:33, deeplcd.cpp:10-31 */
int myslam_lcd_create_from_caffe(myslam_lcd** out, const char* prototxt_path, const char* caffemodel_path);
/* host only (no device needed): parse + validate the two Caffe files into records and the flat weight blob; NULL outputs are skipped */
int myslam_calc_parse_caffe(const char* prototxt_path, const char* caffemodel_path, myslam_calc_layer* layers, int cap, int* nlayers,
                            float* weights, size_t wcap, size_t* nweights);
/* own files: "CALCW1" (weights of the default list) or "CALCW2" (records + weights), see csrc/calc.hip */
int myslam_lcd_create_from_file(myslam_lcd** out, const char* path);
/* 1 = the layer list runs on the fused kernels, 0 = on the generic layer kernels */
int myslam_lcd_uses_fused_kernels(const myslam_lcd* h);
/* partial products per multiply-add of the fused path's conv2: 3 = f16 x 3 (k_conv2_f16x3: the model's ranges fit f16 — |conv2 weight| < 31 and
 * sum |conv1 weights| + |bias| < 60000 with an LRN that cannot amplify), 6 = bf16 x 6 (k_conv2_bf16x6), 0 = generic kernels.  Both matrix-core forms
 * reach f32-level accuracy (max-normalised error against f64: 1.1e-6 / 1.5e-6). */
int myslam_lcd_conv2_products(const myslam_lcd* h);
#define MYSLAM_LCD_OPT_GENERIC_KERNELS 1       /* value != 0: run even a fusable list on the generic kernels (tests, diagnosis) */
#define MYSLAM_LCD_OPT_CONV2_BF16X6 2          /* value != 0: conv2 of the fused path on the six-product bf16 kernel and conv1 on its f32 vector kernel even when
                                                * the model's ranges allow the three-product f16 matrix-core kernels (all reach f32-level accuracy; tests and
                                                * tools/gpu_fuzz_lcd.py compare the two families) */
#define MYSLAM_LCD_OPT_SKIP_KERNELS 3          /* DIAGNOSIS, timing only (results are garbage): bit mask of fused-path kernels that are not launched —
                                                * 1 input, 2 conv1, 4 conv2, 8 pool2, 16 conv3 + norm: what each costs a step that runs beside the extractor */
int myslam_lcd_set_option(myslam_lcd* h, int option, int value);
int myslam_lcd_destroy(myslam_lcd* h);
int myslam_lcd_set_stream(myslam_lcd* h, void* hip_stream);
size_t myslam_lcd_nweights(void);
/* DescrVector calcDescrOriginalImg(const cv::Mat&)  deeplcd.cpp:43-52.  blur_in_place != 0 reproduces
 * the reference's side effect (the caller's image is Gaussian-blurred). */
int myslam_lcd_calc_descr_original_img(myslam_lcd* h, uint8_t* img, int rows, int cols, int step,
                                       int blur_in_place, float* descr1064);
/* const DescrVector calcDescr(const cv::Mat& im)  deeplcd.cpp:55-91; im = 160x120 u8 */
int myslam_lcd_calc_descr(myslam_lcd* h, const uint8_t* img160x120, int step, float* descr1064);
/* const float score(d1, d2)  deeplcd.cpp:35-39 */
float myslam_lcd_score(const float* d1, const float* d2);
int myslam_lcd_describe_batch(myslam_lcd* h, uint8_t* d_imgs, int batch, int rows, int cols, int step,
                              size_t img_stride, int blur_in_place, float* d_descr /* batch x 1064 */);
/* stage taps for parity tests (host buffers, one image) */
int myslam_lcd_debug_forward(myslam_lcd* h, const float* in120x160, float* out_stage, int stage, size_t cap_floats);

/* ------------------------------------------------------------------------------------------
 * Loop database — replaces LoopClosing::_mvDatabase + DetectLoop()/AddToDatabase()
 * (include/myslam/loopclosing.h:67,120; src/loopclosing.cpp:124-161, 651-659).
 * ids must be appended in ascending order (std::map iteration order).
 * query: scan ascending, stop at the first id with cur_id - id < 20, max score (strict >, init 0),
 *        cnt = #{score > thr_low}.  The caller applies maxScore >= thr_high && cnt <= 3.
 * ------------------------------------------------------------------------------------------ */
typedef struct myslam_lcddb myslam_lcddb;
int myslam_lcddb_create(myslam_lcddb** out, int capacity);
int myslam_lcddb_destroy(myslam_lcddb* h);
int myslam_lcddb_set_stream(myslam_lcddb* h, void* hip_stream);
int myslam_lcddb_size(const myslam_lcddb* h);
/* `capacity` of myslam_lcddb_create is the first allocation only: _mvDatabase is an unbounded std::map (loopclosing.h:120), so append
 * grows the device matrix geometrically (x2, one device-to-device copy of the rows held so far; the handle's stream is synchronised
 * while it moves) and fails with MYSLAM_ERR_CAPACITY only when the device has no memory left.  myslam_lcddb_reserve makes room for
 * `rows` key-frames ahead of time (never shrinks); myslam_lcddb_capacity = rows the current allocation holds. */
int myslam_lcddb_capacity(const myslam_lcddb* h);
int myslam_lcddb_reserve(myslam_lcddb* h, int rows);
int myslam_lcddb_append(myslam_lcddb* h, uint64_t id, const float* descr1064);
int myslam_lcddb_append_batch(myslam_lcddb* h, const uint64_t* ids /*host*/, const float* d_descr, int n);
/* AddToDatabase inside a pipelined step (round 6): as myslam_lcddb_append_batch, but the device copies are enqueued on `hip_stream` and the call does NOT wait for them — the
 * caller orders later scans of those rows behind the copy (same stream, or an event).  Ids and row count are updated before the call returns (the next query's row limits
 * cover the new rows).  Never moves the matrix: MYSLAM_ERR_CAPACITY when the rows do not fit the allocation (myslam_lcddb_reserve ahead of the run). */
int myslam_lcddb_append_batch_async(myslam_lcddb* h, const uint64_t* ids /*host*/, const float* d_descr, int n, void* hip_stream);
int myslam_lcddb_query(myslam_lcddb* h, const float* descr1064, uint64_t cur_id, float thr_low,
                       uint64_t* best_id, float* max_score, int* cnt);
/* nq queries at once: d_q nq x 1064 (device), cur_ids nq (HOST); outputs nq each (device).  nq <= 65536; no host synchronisation. */
int myslam_lcddb_query_batch(myslam_lcddb* h, const float* d_q, const uint64_t* cur_ids /*host*/, int nq, float thr_low,
                             uint64_t* d_best_id, float* d_max_score, int32_t* d_cnt);

/* For a query recorded into a HIP graph (myslam_graph_begin / _end below): the per-query row limits (the `cur - id < 20` cut-off of
 * loopclosing.cpp:133 for each cur_id) sit in a pinned host buffer that the recorded copy reads at EVERY replay.  This call rewrites them
 * for new cur_ids or after appends; it waits for the handle's stream first.  MYSLAM_ERR_CAPACITY = the database moved (it grew beyond its
 * allocation) or holds more rows than the recorded launch covers: record the step again.  nq <= the recorded query count. */
int myslam_lcddb_update_query_limits(myslam_lcddb* h, const uint64_t* cur_ids /*host*/, int nq);

/* Query contexts: ONE database, several concurrent streams of queries.  LoopClosing::_mvDatabase is a single std::map that every
 * key-frame of the process goes into (include/myslam/loopclosing.h:120, src/loopclosing.cpp:651-659); with L cameras on one GPU the
 * L loop-closing streams must scan the SAME matrix, not L copies of it.  A myslam_lcddb owns the descriptor matrix and the ids
 * (append / reserve); a myslam_lcddb_query_ctx owns what one stream of scans needs (row-limit staging, partial results, shard
 * scratch, recorded-step state) and is bound to one HIP stream.  The handle's own entry points above use a built-in context on the
 * handle's stream.  Rules:
 *   - appends return when the new rows are in HBM; scans in flight on any context only read rows below the limits they were
 *     issued with, so appends and scans need no ordering between them;
 *   - growth beyond the allocation moves the matrix: append / reserve wait for every context's stream and for every replay of a
 *     recorded step that scans through a context, then bump myslam_lcddb_generation();
 *   - a scan recorded into a step graph covers the whole ALLOCATION (blocks behind the row limits return at once): appends inside the
 *     capacity only need myslam_lcddb_ctx_update_query_limits before the next replay.  After a move, myslam_graph_launch of a step
 *     that captured a scan returns MYSLAM_ERR_CAPACITY (record it again); the old matrix stays allocated until the database is
 *     destroyed, so even an unchecked replay reads valid memory;
 *   - a recorded scan also names the CONTEXT's scratch (row limits, partial results): an eager call on the same context that needs more of it
 *     (more queries than any call before) replaces that scratch after waiting for the step's replays, and the step is refused from then on
 *     (MYSLAM_ERR_CAPACITY: record it again) — round 6;
 *   - while a step that scans through a context is being RECORDED (myslam_graph_begin .. _end, on any thread), nothing may synchronise that
 *     context's stream: an append / reserve that would have to move the matrix, and myslam_lcddb_set_stream, return MYSLAM_ERR_UNSUPPORTED until
 *     the recording has ended.  Appends inside the allocation are unaffected, except that myslam_lcddb_append / _append_batch wait for their
 *     copies on the handle's stream: while THAT stream is being captured they return MYSLAM_ERR_UNSUPPORTED before they enqueue anything — round 6;
 *   - a query holds the database's host lock until its launches are enqueued, so a growing append from another thread waits for them (its stream
 *     synchronisation then covers the scan) instead of freeing the matrix under a launch that is about to be issued — round 6;
 *   - contexts are destroyed before their database (myslam_lcddb_destroy frees any that are left: their pointers die with it).
 * One thread per context; append / reserve may come from any thread. */
typedef struct myslam_lcddb_query_ctx myslam_lcddb_query_ctx;
int myslam_lcddb_query_ctx_create(myslam_lcddb_query_ctx** out, myslam_lcddb* db, void* hip_stream);
int myslam_lcddb_query_ctx_destroy(myslam_lcddb_query_ctx* c);
int myslam_lcddb_ctx_query_batch(myslam_lcddb_query_ctx* c, const float* d_q, const uint64_t* cur_ids /*host*/, int nq, float thr_low,
                                 uint64_t* d_best_id, float* d_max_score, int32_t* d_cnt);
int myslam_lcddb_ctx_update_query_limits(myslam_lcddb_query_ctx* c, const uint64_t* cur_ids /*host*/, int nq);
/* number of times the descriptor matrix has moved (growth): a recorded step is valid for the generation it was recorded in */
int myslam_lcddb_generation(const myslam_lcddb* h);

/* Multi-GPU form: the database is sharded by contiguous key-frame id range, shard r on rank r, every shard scores
 * every query.  A shard's answer travels as one 16-byte record; the records of all shards (rank order = id order) are reduced to what
 * ONE scan of src/loopclosing.cpp:124-161 over the whole std::map returns: strict '>' keeps the first (lowest-id) maximum, counts
 * add up, and the first shard whose own scan hit the `cur - id < 20` break (:133) ends the scan for all shards behind it.
 * The all-gather between the two calls is the caller's (RCCL ncclAllGather on the raw bytes). */
typedef struct myslam_lcd_candidate {
    uint64_t best_id;      /* 0 when nothing scored above 0 (loopclosing.cpp:129) */
    float max_score;
    int32_t cnt;           /* bits 0..30: #{score > thr_low} in this shard; bit 31: this shard's scan stopped at the break */
} myslam_lcd_candidate;
/* as myslam_lcddb_query_batch, one record per query (device memory, asynchronous on the handle's stream) */
int myslam_lcddb_query_batch_sharded(myslam_lcddb* h, const float* d_q, const uint64_t* cur_ids /*host*/, int nq, float thr_low,
                                     myslam_lcd_candidate* d_cand);
int myslam_lcddb_ctx_query_batch_sharded(myslam_lcddb_query_ctx* c, const float* d_q, const uint64_t* cur_ids /*host*/, int nq, float thr_low,
                                     myslam_lcd_candidate* d_cand);
/* gathered: [nshards][nq] records, shard-major in ascending id-range order.  Host pointers (plain C++, no device needed). */
int myslam_lcd_merge_candidates(const myslam_lcd_candidate* gathered, int nshards, int nq, uint64_t* best_id, float* max_score, int32_t* cnt);
/* the same reduce on device pointers, asynchronous on hip_stream */
int myslam_lcd_merge_candidates_device(const myslam_lcd_candidate* d_gathered, int nshards, int nq, uint64_t* d_best_id,
                                       float* d_max_score, int32_t* d_cnt, void* hip_stream);

/* A sharded database that GROWS (round 6).  With contiguous id ranges every new key-frame belongs to the last rank; a job that appends (the reference
 * does, per key-frame: LoopClosing::AddToDatabase, src/loopclosing.cpp:651-659) spreads the rows instead — e.g. the k-th key-frame of the job goes to rank
 * k mod N (sharded_db.py GrowingShardedDatabase; app/sharded_db_rccl.cpp) — and a shard's ids then INTERLEAVE with the others'.  Any rule works that puts
 * every id into exactly one shard and keeps each shard's own ids ascending.  The reference's one ascending scan (:124-161) looks at every id below the
 * cut-off window {id : cur - id < 20}, stops if the map holds an id inside it, and otherwise goes on with the ids above cur; so a shard reports BOTH parts
 * and whether it holds an id inside the window (32 bytes per query), and the merge — highest score, LOWEST ID among equal scores (shard order is not id
 * order here), counts added — takes the parts above cur only when no shard reported the break.  Bit-identical to one scan of the whole map. */
typedef struct myslam_lcd_owned_candidate {
    uint64_t pre_best_id;  /* over this shard's ids below the window: 0 when nothing scored above 0 */
    float pre_max_score;
    int32_t pre_cnt;       /* bits 0..30: #{score > thr_low}; bit 31: this shard holds an id with cur - id < 20 */
    uint64_t suf_best_id;  /* over this shard's ids above cur */
    float suf_max_score;
    int32_t suf_cnt;
} myslam_lcd_owned_candidate;
/* one record per query (device memory, asynchronous on the stream; not recordable into a step graph) */
int myslam_lcddb_query_batch_owned(myslam_lcddb* h, const float* d_q, const uint64_t* cur_ids /*host*/, int nq, float thr_low,
                                   myslam_lcd_owned_candidate* d_cand);
int myslam_lcddb_ctx_query_batch_owned(myslam_lcddb_query_ctx* c, const float* d_q, const uint64_t* cur_ids /*host*/, int nq, float thr_low,
                                       myslam_lcd_owned_candidate* d_cand);
/* gathered: [nshards][nq] records, shard-major, ANY shard order.  Host pointers / device pointers (asynchronous on hip_stream). */
int myslam_lcd_merge_owned_candidates(const myslam_lcd_owned_candidate* gathered, int nshards, int nq, uint64_t* best_id, float* max_score, int32_t* cnt);
int myslam_lcd_merge_owned_candidates_device(const myslam_lcd_owned_candidate* d_gathered, int nshards, int nq, uint64_t* d_best_id,
                                             float* d_max_score, int32_t* d_cnt, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * Loop database bank — S loop databases in one device allocation, item s = stream s as in the tracker, the back end and the archives.  A bank of S
 * streams is S reference Systems, so S LoopClosing::_mvDatabase maps (include/myslam/loopclosing.h:120) whose key-frame ids all start at 0
 * (myslam_tracker's new_kf_id).  Per stream it replaces the gate of LoopClosingRun (src/loopclosing.cpp:62), the scan of DetectLoop (:126-143) and
 * AddToDatabase (:651-659).
 *
 * Layout, fixed at create: rows [S][rows_per_stream][1064] f32, ids [S][rows_per_stream] u64 ascending per stream, count [S] i32 — all in device
 * memory; nothing grows and nothing moves, so a recorded step (myslam_graph_begin / _end) that names the bank stays valid for ever and a replay sees
 * the rows appended since the recording.  After create no call changes host state but set_stream.  query / append / clear enqueue on the handle's
 * stream and return: they read no device memory from the host, allocate nothing, never synchronise and use no global atomics.  One stream of calls per
 * bank (the query's scratch is the handle's).  load / get / sizes are the synchronous test and resume path: host pointers, they wait for the
 * handle's stream (MYSLAM_ERR_UNSUPPORTED while it is being recorded).
 *
 * query_batch (d_q S x 1064, 16-byte aligned; d_cur_id S; d_active S or NULL = every item; outputs S each), per item s —
 * LoopClosing::DetectLoop's loop, src/loopclosing.cpp:126-143, behind the gate at :62:
 *   1. d_active[s] == 0: d_status[s] = MYSLAM_LCDBANK_IDLE, (d_best_id, d_max_score, d_cnt)[s] = (0, 0.0f, 0), d_best_row[s] = -1; d_q and
 *      d_cur_id of the item are not read;
 *   2. n[s] <= min_size: MYSLAM_LCDBANK_GATED with the same outputs (`_mvDatabase.size() > _mnDatabaseMinSize`, :62);
 *   3. else MYSLAM_LCDBANK_SCANNED: rows 0 .. n[s]-1 of the stream in ascending order, ending at the first row with (cur - id) mod 2^64 < 20 (:133;
 *      the window wraps for cur < 19); the maximum starts at 0 with best id 0 (:128-129), '>' is strict for the maximum (the lowest row wins ties)
 *      and for cnt = #{score > thr_low}; NaN never wins and is never counted.  d_best_row[s] = the winning row's index inside its stream, -1 when
 *      nothing scored above 0.
 * The three outputs are myslam_loop_detect_batch's inputs: an idle or gated item carries a score of 0 and ends MYSLAM_LOOP_DETECT_NO_LOOP there.
 * A score is an f32 sum whose order depends on the entry's place in its row only: the same row and query give the same bits in every stream and slot.
 * At most myslam_lcdbank_launches_per_query() = 3 launches; a workgroup scans MYSLAM_LCDBANK_ROW_TILE rows of one stream (myslam_lcdbank_row_tile()).
 *
 * append_batch (d_descr S x 1064, d_id S, d_add S or NULL = every item), one launch, one workgroup per stream — AddToDatabase, :651-659:
 *   d_add[s] == 0                               MYSLAM_LCDBANK_IDLE, nothing read or written but the status
 *   the stream holds rows_per_stream rows       MYSLAM_ERR_CAPACITY, nothing stored
 *   n[s] > 0 and d_id[s] <= the last id held    MYSLAM_ERR_INVALID, nothing stored (std::map order, as myslam_lcddb_append_batch's rule on the host)
 *   otherwise                                   MYSLAM_LCDBANK_ADDED: row and id written at n[s], then n[s] incremented
 * A query enqueued behind it on the same stream sees the row.
 *
 * clear_batch: n[s] = 0 where d_clear[s] != 0 (a stream that starts again, myslam_tracker_reset_stream, has an empty database).
 * load replaces stream s: rows and ids below n and the count are written, bytes behind n are kept; ids must ascend strictly (MYSLAM_ERR_INVALID),
 * n > rows_per_stream: MYSLAM_ERR_CAPACITY; the stream keeps every byte then.  get: *n = the count; more than cap: MYSLAM_ERR_CAPACITY, nothing copied
 * (ids / rows may be NULL).
 *
 * Call level, nothing enqueued: NULL required pointers, a d_q that is not 16-byte aligned, sizes <= 0, a stream index out of range ->
 * MYSLAM_ERR_INVALID; streams > 65535 or rows_per_stream > 2^24 -> MYSLAM_ERR_CAPACITY; create out of device memory -> MYSLAM_ERR_CAPACITY, any
 * other HIP failure -> MYSLAM_ERR_HIP.
 *
 * The per-stream key-frame store (d_best_row is its key), the decision of which items end unconfirmed (d_add) and the five-key-frames rule of
 * LoopClosing::InsertNewKeyFrame (d_active) are myslam_loop_bank's, below.  Out of scope: the wiring into a bank of trackers, and sharding a bank over
 * several GPUs.
 * ------------------------------------------------------------------------------------------ */
typedef struct myslam_lcdbank myslam_lcdbank;
#define MYSLAM_LCDBANK_SCANNED 0
#define MYSLAM_LCDBANK_GATED   1
#define MYSLAM_LCDBANK_IDLE    2
#define MYSLAM_LCDBANK_ADDED   3
#define MYSLAM_LCDBANK_ROW_TILE 32
int myslam_lcdbank_create(myslam_lcdbank** out, int streams, int rows_per_stream);
int myslam_lcdbank_destroy(myslam_lcdbank* h);
int myslam_lcdbank_set_stream(myslam_lcdbank* h, void* hip_stream);
int myslam_lcdbank_row_tile(void);
int myslam_lcdbank_launches_per_query(void);
int myslam_lcdbank_query_batch(myslam_lcdbank* h, const float* d_q /*S x 1064*/, const uint64_t* d_cur_id /*S*/, const int32_t* d_active /*S, NULL = all*/,
        float thr_low, int min_size,
        uint64_t* d_best_id, float* d_max_score, int32_t* d_cnt,     /* S each: myslam_loop_detect_batch's inputs */
        int32_t* d_best_row, int32_t* d_status);                     /* S each */
int myslam_lcdbank_append_batch(myslam_lcdbank* h, const float* d_descr /*S x 1064*/, const uint64_t* d_id /*S*/, const int32_t* d_add /*S, NULL = all*/,
        int32_t* d_status);
int myslam_lcdbank_clear_batch(myslam_lcdbank* h, const int32_t* d_clear /*S*/);
int myslam_lcdbank_view(const myslam_lcdbank* h, const float** d_rows, const uint64_t** d_ids, const int32_t** d_n);
int myslam_lcdbank_load(myslam_lcdbank* h, int s, const uint64_t* ids, const float* rows, int n);   /* host pointers, synchronous, replaces stream s */
int myslam_lcdbank_get(myslam_lcdbank* h, int s, uint64_t* ids, float* rows, int cap, int* n);      /* host pointers, synchronous */
int myslam_lcdbank_sizes(myslam_lcdbank* h, int32_t* n /*S, host*/);

/* ------------------------------------------------------------------------------------------
 * Loop key-frame store BANK: S per-stream key-frame stores in device memory, with the three decisions of LoopClosingRun that sit between the batched
 * units — which key-frames the loop closer takes at all (LoopClosing::InsertNewKeyFrame, src/loopclosing.cpp:671-681), which ones end unconfirmed and
 * are kept (`if(!bConfirmedLoopKF) AddToDatabase()`, :73-75, the store half of :651-659) and `_mpLastClosedKF = _mpCurrentKF` (:331) — taken on the
 * device.  Stream s is one reference System: its own _mvDatabase (include/myslam/loopclosing.h:120) as far as key-frames go, its own _mpLastClosedKF,
 * ids that start at 0.  myslam_lcdbank holds the same streams' image descriptors; a bank and an lcdbank created with the same number of rows per stream
 * and fed the same ids and the same d_add make the same refusals, so row r of stream s names the same key-frame in both, and the scan's d_best_row is
 * the slot detect reads.  If the two are driven apart (different ids, different d_add, one of them cleared alone), detect answers MYSLAM_ERR_INVALID
 * for that stream: the id at the row is compared with d_best_id.
 *
 * Layout, fixed at create (K = kfs_per_stream; strides cap_st / feat_st = cap / feat_cap rounded up to 4, as in myslam_loop_store): key-points
 * [S][K][cap_st] (28 bytes each), descriptors [S][K][cap_st x 32], landmark tables [S][K][feat_st] i32, rows [S][K] i32, n_feat [S][K] i32, ids [S][K] u64
 * ascending per stream, n [S] i32, last_closed [S] i64 (-1 = no loop closed yet), put_slot [S] i32 (finish's plan, below).  Nothing grows and nothing
 * moves, so a recorded step (myslam_graph_begin / _end) that names the bank stays valid and a replay sees the key-frames stored since the recording.
 * After create no call changes host state but set_stream.  gate / detect / finish / links / clear take DEVICE pointers, enqueue on the handle's
 * stream and return: they read no device memory from the host, allocate nothing, never synchronise and use no global atomics.  One stream of calls per
 * bank.  Key-frame ids are below 2^63 (the gate's id is the tracker's signed new_kf_id).
 *
 * gate_batch — InsertNewKeyFrame, :671-681 — one launch.  Stream s is a candidate iff d_new_kf_id[s] >= 0 and (d_item_status == NULL or
 * d_item_status[s * status_stride] == 0): pass myslam_mapper_keyframe_batch's d_status with stride MYSLAM_MAPPER_STATUS_WORDS, whose word 0 is 0 for a
 * mapped stream.  A candidate is taken iff last_closed[s] < 0 || (uint64)(id - last_closed[s]) > 5, the reference's unsigned expression as written
 * (:674-675).  d_active[s] = 1 / 0 (what myslam_lcdbank_query_batch takes as d_active); d_status[s] = MYSLAM_LOOP_BANK_TURN, _SKIPPED (one of the
 * five key-frames behind a closed loop: neither processed nor stored) or _IDLE (no candidate).
 *
 * detect_batch — :147 and `_mpLoopKF = _mvDatabase.at(bestId)` (:151) — one launch, grid (chunks, S).  d_best_id / d_best_row / d_max_score / d_cnt are
 * myslam_lcdbank_query_batch's outputs.  The decision is myslam_loop_detect_batch's, literally (`d_max_score[s] < thr_high || d_cnt[s] >
 * max_suspected` -> MYSLAM_LOOP_DETECT_NO_LOOP; a NaN score is not "less"; thr_high = +inf rejects every finite score).  The lookup is the row the scan
 * found: slot = d_best_row[s], valid iff 0 <= slot < n[s] and ids[s][slot] == d_best_id[s] — one load, no search; otherwise MYSLAM_ERR_INVALID with
 * d_n_loop[s] = 0, d_loop_slot[s] = -1.  Status values, the output layout (item s at + s*cap / + s*feat_cap) and "no other byte of a rejected item is
 * written" are myslam_loop_detect_batch's.
 *
 * finish_batch — :73-75 with :331 and AddToDatabase's store half (:651-659) — myslam_loop_bank_launches_per_finish() = 2 launches.
 *   a. the decision, one workgroup, per stream s:
 *        d_active[s] == 0                                      MYSLAM_LOOP_BANK_IDLE, d_add[s] = 0
 *        d_verify_status[s] == MYSLAM_VERIFY_CONFIRMED         last_closed[s] = d_cur_kf_id[s], d_add[s] = 0, MYSLAM_LOOP_BANK_CLOSED: the key-frame is
 *                                                              not stored, as in the reference
 *        n[s] == K                                             MYSLAM_ERR_CAPACITY, d_add[s] = 0, every byte of the stream kept
 *        n[s] > 0 and d_cur_kf_id[s] <= the last id held       MYSLAM_ERR_INVALID, d_add[s] = 0, every byte of the stream kept (std::map order)
 *        otherwise                                             put_slot[s] = n[s], d_add[s] = 1, MYSLAM_LOOP_BANK_STORED
 *      put_slot[s] = -1 in every case but the last.
 *   b. the copy, grid (chunks, S): a workgroup reads put_slot[s], which nothing writes during this launch, and returns when it is -1; otherwise it moves
 *      its share of the stream's item (d_pyr_kps / d_desc / d_counts / d_kf_status / d_feat_landmark / d_n_feat: item s of
 *      myslam_orb_process_keyframes_batch's outputs and the landmark table, in myslam_loop_store_put_batch's layout and with its clamping rules: counts
 *      clamped to [0, cap] / [0, feat_cap], d_kf_status[s] != 0 stores 0 rows) into slot put_slot[s]; chunk 0 writes rows, n_feat, the id and
 *      n[s] = put_slot[s] + 1.  No workgroup reads n[s] in this launch: the count changes at a launch boundary, with no flag, atomic or fence inside a
 *      launch.
 *   d_add is myslam_lcdbank_append_batch's d_add.
 *
 * links_batch — myslam_loop_store_clear_links_batch / _set_links_batch per stream, entry for entry (LINK UPKEEP below; d_value NULL = -1
 * for every entry: clear_links): item s walks its list against stream s's ids only; the pending key-frame's table and the skipping of ids that are not held
 * included.  One launch of S workgroups.
 *
 * clear_batch: n[s] = 0 and last_closed[s] = -1 where d_reset[s] != 0 (a stream that starts again, myslam_tracker_reset_stream).  One launch.
 *
 * load / get / sizes are the synchronous resume and test path: HOST pointers, they wait for the handle's stream (MYSLAM_ERR_UNSUPPORTED while it is being
 * recorded).  load replaces stream s: n key-frames, kps n x cap, desc n x cap x 32, feat_landmark n x feat_cap, whole slots; ids ascend strictly,
 * rows in [0, cap], n_feat in [0, feat_cap], last_closed >= -1, else MYSLAM_ERR_INVALID; n > K: MYSLAM_ERR_CAPACITY; the stream keeps every byte then.
 * get: *n = the count, *last_closed; more than kf_room key-frames: MYSLAM_ERR_CAPACITY, nothing copied; array pointers may be NULL.
 *
 * Call level, nothing enqueued: NULL required pointers (d_item_status, d_kf_status, d_value, d_n_set and both pending pointers may be NULL; the
 * pending pointers both or neither), sizes <= 0, a stream index out of range -> MYSLAM_ERR_INVALID; cap > 16384, feat_cap > 65536
 * (myslam_loop_match_batch's limits) or streams > 65535 -> MYSLAM_ERR_CAPACITY; create out of device memory -> MYSLAM_ERR_CAPACITY, any other HIP
 * failure -> MYSLAM_ERR_HIP.
 *
 * Out of scope: the wiring into a bank of trackers, skipping ProcessNewKF's work for the streams the gate rejects, DeepLCD's in-place blur hand-back,
 * sharding a bank over several GPUs.
 * ------------------------------------------------------------------------------------------ */
typedef struct myslam_loop_bank myslam_loop_bank;
#define MYSLAM_LOOP_BANK_TURN    0
#define MYSLAM_LOOP_BANK_SKIPPED 1
#define MYSLAM_LOOP_BANK_IDLE    2
#define MYSLAM_LOOP_BANK_CLOSED  3
#define MYSLAM_LOOP_BANK_STORED  4
typedef struct myslam_loop_bank_arrays {      /* device pointers and shapes, as laid out above */
    myslam_keypoint* kps; uint8_t* desc; int32_t* feat_landmark;
    int32_t* rows; int32_t* n_feat; uint64_t* ids; int32_t* n; int64_t* last_closed; int32_t* put_slot;
    int32_t streams, kfs_per_stream, cap, feat_cap;
    int64_t cap_stride, feat_stride;          /* key-points / landmark entries per slot */
} myslam_loop_bank_arrays;
int myslam_loop_bank_create(myslam_loop_bank** out, int streams, int kfs_per_stream, int cap, int feat_cap);
int myslam_loop_bank_destroy(myslam_loop_bank* h);
int myslam_loop_bank_set_stream(myslam_loop_bank* h, void* hip_stream);
int myslam_loop_bank_view(const myslam_loop_bank* h, myslam_loop_bank_arrays* out);
int myslam_loop_bank_launches_per_finish(void);
int myslam_loop_bank_gate_batch(myslam_loop_bank* h, const int64_t* d_new_kf_id /*S*/, const int32_t* d_item_status /*may be NULL*/, int status_stride,
        int32_t* d_active /*out S*/, int32_t* d_status /*out S*/);
int myslam_loop_bank_detect_batch(myslam_loop_bank* h,
        const uint64_t* d_best_id, const int32_t* d_best_row, const float* d_max_score, const int32_t* d_cnt,   /* myslam_lcdbank_query_batch's outputs, S each */
        float thr_high, int max_suspected,                                                                      /* 0.94f and 3 at loopclosing.cpp:147 */
        uint8_t* d_loop_desc, int32_t* d_n_loop, myslam_keypoint* d_loop_pyr, int32_t* d_loop_feat_landmark,    /* loop_match_batch's inputs, item s at + s*cap (+ s*feat_cap) */
        int32_t* d_loop_slot, int32_t* d_status);                                                               /* S each */
int myslam_loop_bank_finish_batch(myslam_loop_bank* h, const uint64_t* d_cur_kf_id /*S*/, const int32_t* d_active /*S*/, const int32_t* d_verify_status /*S*/,
        const myslam_keypoint* d_pyr_kps, const uint8_t* d_desc, const int32_t* d_counts, const int32_t* d_kf_status /*may be NULL*/,
        const int32_t* d_feat_landmark, const int32_t* d_n_feat,
        int32_t* d_add /*out S*/, int32_t* d_status /*out S*/);
int myslam_loop_bank_links_batch(myslam_loop_bank* h, const int64_t* d_kf_id, const int32_t* d_tag, const int32_t* d_value /*NULL = -1 for all*/,
        const int32_t* d_n, int list_cap, const int64_t* d_pending_kf_id, int32_t* d_pending_feat_landmark, int32_t* d_n_set);
int myslam_loop_bank_clear_batch(myslam_loop_bank* h, const int32_t* d_reset /*S*/);
int myslam_loop_bank_load(myslam_loop_bank* h, int s, const uint64_t* ids, const myslam_keypoint* kps, const uint8_t* desc, const int32_t* rows,
        const int32_t* feat_landmark, const int32_t* n_feat, int n, int64_t last_closed);      /* host pointers, synchronous, replaces stream s */
int myslam_loop_bank_get(myslam_loop_bank* h, int s, uint64_t* ids, myslam_keypoint* kps, uint8_t* desc, int32_t* rows, int32_t* feat_landmark,
        int32_t* n_feat, int kf_room, int* n, int64_t* last_closed);                           /* host pointers, synchronous */
int myslam_loop_bank_sizes(myslam_loop_bank* h, int32_t* n /*S, host*/);

/* ------------------------------------------------------------------------------------------
 * Local BA linear-system build — replaces the per-edge work g2o does for
 * Backend::OptimizeActiveMap (src/backend.cpp:126-232): EdgeProjection::computeError /
 * linearizeOplus (include/myslam/g2o_types.h:115-144), Huber(delta) and the block quadratic form.
 * poses  nposes x 7  (qx qy qz qw tx ty tz), Tcw;  points npts x 3;  obs nedges x 2
 * Hpp nposes x 36, Hll npts x 9, Hpl nedges x 18 (6x3 row-major), bp nposes x 6, bl npts x 3,
 * chi2 nedges (un-robustified e^T e, what edge->chi2() returns at backend.cpp:219,238)
 * ------------------------------------------------------------------------------------------ */
int myslam_ba_build(const double* poses, int nposes, const double* points, int npts,
                    const int32_t* edge_pose, const int32_t* edge_pt, const double* obs, int nedges,
                    const uint8_t* fixed_pt, double fx, double fy, double cx, double cy, double huber_delta,
                    double* Hpp, double* Hll, double* Hpl, double* bp, double* bl, double* chi2);
/* batch of `nwin` windows with identical capacities (max_poses, max_pts, max_edges); window w's arrays
 * start at base + w*capacity*elemsize; d_sizes = nwin x 3 (nposes, npts, nedges).  A window whose sizes exceed the capacities is
 * skipped: its blocks are zero and its chi2[0] = -1. */
int myslam_ba_build_batch(const double* d_poses, const double* d_points, const int32_t* d_edge_pose,
                          const int32_t* d_edge_pt, const double* d_obs, const uint8_t* d_fixed,
                          const int32_t* d_sizes, int nwin, int max_poses, int max_pts, int max_edges,
                          double fx, double fy, double cx, double cy, double huber_delta,
                          double* d_Hpp, double* d_Hll, double* d_Hpl, double* d_bp, double* d_bl, double* d_chi2,
                          void* hip_stream);

/* Map -> flat arrays: the graph-build rules of Backend::OptimizeActiveMap (src/backend.cpp:139-206) as a host function (plain C++,
 * no device needed), so that a maintainer's OptimizeActiveMap body is { copy the Map's tables; flatten; optimize_active_map; write back }.
 * Inputs (host pointers), one row per object of the reference's containers:
 *   active_kf_ids[n_kf]                 Map::GetActiveKeyFrames() keys (any order; :136,139-150)
 *   mp_ids / mp_outlier / mp_first_observer_kf [n_mp]   Map::GetActiveMapPoints(): mnId, mbIsOutlier, and the key-frame id of
 *                                       GetObservations().front() (:163-177)
 *   obs_mp_id / obs_kf_id / obs_uv / obs_feat_outlier [n_obs]   every MapPoint::GetActiveObservations() entry (list order within a map
 *                                       point): the map point's id, feature->mpKF->mnKFId, feature->mkpPosition.pt, feature->mbIsOutlier (:181-189)
 * Rules reproduced: outlier map points get no vertex and no edges (:163); outlier features get no edge (:189); a map point whose FIRST
 * observer is not an active key-frame is fixed (:175-177); an observation from a key-frame outside the active set is the reference's
 * assert (:187) -> MYSLAM_ERR_INVALID, as is an observation of an unknown map point.  Orders (the reference iterates unordered_maps, g2o
 * then sorts vertices by id): pose slots by ascending key-frame id, landmark slots by ascending map-point id, edges grouped by landmark
 * (what myslam_ba_optimize* need) in observation-list order.  Map points left without an edge are dropped (g2o never activates them).
 * Outputs: pose_src[n_kf] / pt_src[*n_pts] = index of the INPUT row each slot was taken from (to gather poses / positions and to write
 * results back: :252-258), edge_pose / edge_pt / edge_obs (double, as toVec2) / edge_src (index of the observation row, for the outlier
 * write-back :234-250) [*n_edges <= n_obs], fixed_pt[*n_pts]. */
int myslam_ba_flatten_window(const uint64_t* active_kf_ids, int n_kf, const uint64_t* mp_ids, const uint8_t* mp_outlier,
                             const uint64_t* mp_first_observer_kf, int n_mp, const uint64_t* obs_mp_id, const uint64_t* obs_kf_id,
                             const float* obs_uv, const uint8_t* obs_feat_outlier, int n_obs, int32_t* pose_src, int32_t* pt_src,
                             int32_t* n_pts, int32_t* edge_pose, int32_t* edge_pt, double* edge_obs, int32_t* edge_src, int32_t* n_edges,
                             uint8_t* fixed_pt);

/* The solve kernels keep a window's pose system on one wavefront: at most MYSLAM_BA_MAX_WINDOW_POSES key-frames per window
 * (Map.activeMap.size is 7 in every config the reference ships, config/stereo/gray/KITTI00-02.yaml:73); a larger window returns
 * MYSLAM_ERR_UNSUPPORTED from myslam_ba_optimize* (myslam_ba_build* has no such limit). */
#define MYSLAM_BA_MAX_WINDOW_POSES 10

/* Levenberg-Marquardt with Schur complement on device — replaces optimizer.optimize(n) of
 * Backend::OptimizeActiveMap (src/backend.cpp:212-214: g2o OptimizationAlgorithmLevenberg + BlockSolver_6_3 +
 * CSparse).  poses/points are updated in place.  Edges must be grouped by landmark
 * (backend.cpp:161-205 builds them that way; myslam_ba_flatten_window does); max_poses <= MYSLAM_BA_MAX_WINDOW_POSES.  d_scratch: nwin x max_edges x 18 doubles.
 * Windows too large for the all-in-LDS solver (more than ~470 landmarks at 10 key-frames) keep 22 doubles per landmark behind the edge list in
 * that scratch: the batch entry points return MYSLAM_ERR_CAPACITY when max_edges x 18 < max_edges / 2 + 22 max_pts + 10 — windows of many
 * short-lived landmarks with one or two observations each; max_edges is only a capacity, raise it.  The host-pointer entry points size
 * their scratch themselves and have no such limit. */
int myslam_ba_optimize(double* poses, int nposes, double* points, int npts, const int32_t* edge_pose, const int32_t* edge_pt,
                       const double* obs, int nedges, const uint8_t* fixed_pt, double fx, double fy, double cx, double cy,
                       double huber_delta, int max_iters, double* final_chi2, int* iters);
int myslam_ba_optimize_batch(double* d_poses, double* d_points, const int32_t* d_edge_pose, const int32_t* d_edge_pt,
                             const double* d_obs, const uint8_t* d_fixed, const int32_t* d_sizes, int nwin, int max_poses,
                             int max_pts, int max_edges, double fx, double fy, double cx, double cy, double huber_delta,
                             int max_iters, double* d_scratch, double* d_final_chi2, int32_t* d_iters, int32_t* d_status,
                             void* hip_stream);

/* The whole solve stage of Backend::OptimizeActiveMap (src/backend.cpp:208-243): up to max_rounds (5) times
 * { initializeOptimization(); optimize(iters_per_round = 10) }, stopping as soon as more than half of the edges have
 * chi2() <= chi2_th (5.991); then the outlier flags of :232-249.  edge_chi2[k] is what edge->chi2() returns there: e^T e of
 * the last error evaluation (the last Levenberg trial, accepted or not — a g2o property the reference inherits).
 * *rounds = the reference's `iteration` counter (rounds that failed the inlier test).  *rounds == max_rounds means EVERY round failed:
 * the window did NOT converge to a majority-inlier solution (the reference carries on with the result regardless, backend.cpp:232-266;
 * on such windows the Levenberg iteration is chaotic — one ulp in an observation moves the final poses by decimetres in the reference
 * arithmetic itself — so poses / flags agree with another implementation only in distribution: tests/golden/ba_chaotic_window.npz).
 * MYSLAM_BA_CONVERGED(rounds, max_rounds) spells the test.  Edges grouped by landmark, max_poses <= MYSLAM_BA_MAX_WINDOW_POSES. */
#define MYSLAM_BA_CONVERGED(rounds, max_rounds) ((rounds) < (max_rounds))
int myslam_ba_optimize_active_map(double* poses, int nposes, double* points, int npts, const int32_t* edge_pose, const int32_t* edge_pt,
                                  const double* obs, int nedges, const uint8_t* fixed_pt, double fx, double fy, double cx, double cy,
                                  double huber_delta, double chi2_th, int max_rounds, int iters_per_round,
                                  double* edge_chi2, uint8_t* outlier, int* rounds, int* n_outliers);
/* batched / device-resident form; d_edge_chi2, d_outlier: nwin x max_edges; d_rounds, d_n_outliers, d_status: nwin */
int myslam_ba_optimize_active_map_batch(double* d_poses, double* d_points, const int32_t* d_edge_pose, const int32_t* d_edge_pt,
                                        const double* d_obs, const uint8_t* d_fixed, const int32_t* d_sizes, int nwin, int max_poses,
                                        int max_pts, int max_edges, double fx, double fy, double cx, double cy, double huber_delta,
                                        double chi2_th, int max_rounds, int iters_per_round, double* d_scratch, double* d_edge_chi2,
                                        uint8_t* d_outlier, int32_t* d_rounds, int32_t* d_n_outliers, int32_t* d_status, void* hip_stream);

/* Scheduling knob of the solve kernel (process-wide, no reference counterpart; results do not depend on it beyond f64 rounding of
 * nothing: the arithmetic and its order are the same).  MYSLAM_BA_OPT_LANDMARKS_IN_HBM: 0 (default) = a window's per-landmark state lives
 * in LDS whenever it fits (133 KB for 10 key-frames x 300 landmarks: one window per CU and almost nothing beside it); 1 = always in the
 * window's HBM scratch (81 KB of LDS: the form for a solve that runs BESIDE other kernels, e.g. on the Backend's stream under the
 * extractor — its CU keeps room for their blocks).  d_scratch sizes are the same in both forms. */
#define MYSLAM_BA_OPT_LANDMARKS_IN_HBM 1
/* MYSLAM_BA_OPT_BUILD_POSE_ATOMICS (block build, myslam_ba_build[_batch]): 0 (default) = calls of fewer than 32 windows stage a window's arrays in
 * LDS and sum the pose blocks by one wave per pose over a counting-sorted edge list whenever that fits (33 bytes of LDS per edge slot + 24 per
 * landmark slot); 1 = always the form batches use (every edge's 27 pose terms added into per-wave LDS copies with ds_add_f64).  Both forms are
 * bit-reproducible; they differ from each other in the last bits of Hpp / bp (another summation order), in nothing else. */
#define MYSLAM_BA_OPT_BUILD_POSE_ATOMICS 2
int myslam_ba_set_option(int option, int value);

/* ------------------------------------------------------------------------------------------
 * Pose-only optimisation of the current frame — replaces the g2o part of Frontend::EstimateCurrentPose
 * (src/frontend.cpp:176-276): one VertexPose, one EdgeProjectionPoseOnly (include/myslam/g2o_types.h:62-100) per tracked
 * feature with a map point, Huber(1), Levenberg; `rounds` (4) x { optimize(iters = 10) over the admitted edges; classify every
 * edge by chi2 > chi2_th (5.991), exclude / re-admit }; the robust kernel is dropped after round rounds-2.   [§8(f) rank 1]
 * pose7 = (qx qy qz qw tx ty tz) Tcw in/out; pts3d n x 3 (MapPoint::Pos()); obs n x 2 (feature pixel); outlier[i] = the
 * feature's mbIsOutlier at :231-241; *n_inliers = features.size() - cntOutliers (:275).  n <= 4096.
 * pre_optimize = number of plain optimize(iters) calls before the rounds: 0 for the frontend; 1 reproduces
 * LoopClosing::OptimizeCurrentPose (src/loopclosing.cpp:339-433, extra optimize at :395-396; outlier[i] = vEdgeIsOutlier[i]).
 * ------------------------------------------------------------------------------------------ */
int myslam_pose_only_optimize(double* pose7, const double* pts3d, const double* obs, int n, double fx, double fy, double cx, double cy,
                              double chi2_th, int rounds, int iters, int pre_optimize, uint8_t* outlier, int* n_inliers);
/* `batch` frames: d_poses batch x 7, d_pts3d batch x cap x 3, d_obs batch x cap x 2, d_counts batch, d_outlier batch x cap.  A count below 0 is
 * read as 0, one above cap as cap; slots from a frame's count on are neither read nor written; a frame of 0 matches reports 0 inliers and status OK
 * and keeps its pose (the unit quaternion of the one it had), as myslam_pose_only_optimize does for n = 0. */
int myslam_pose_only_optimize_batch(double* d_poses, const double* d_pts3d, const double* d_obs, const int32_t* d_counts, int batch, int cap,
                                    double fx, double fy, double cx, double cy, double chi2_th, int rounds, int iters, int pre_optimize,
                                    uint8_t* d_outlier, int32_t* d_n_inliers, int32_t* d_status, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * Pyramidal Lucas-Kanade tracker — replaces
 *   cv::calcOpticalFlowPyrLK(prev, next, prevPts, nextPts, status, err, Size(win,win), max_level,
 *                            TermCriteria(COUNT+EPS, max_iters, eps), OPTFLOW_USE_INITIAL_FLOW)
 * as called by Frontend::TrackLastFrame (src/frontend.cpp:150-153) and Frontend::FindFeaturesInRight (:358-361) with
 * win 11, max_level 3, max_iters 30, eps 0.01 (minEigThreshold = OpenCV's default 1e-4).   [SURVEY.md §8(f) rank 1]
 * next_pts is in/out: the initial flow on entry (the reference always passes one), the tracked positions on return;
 * status[i] = 1 where the flow was found; err[i] (optional) = mean absolute patch difference / 32 at level 0.
 * ------------------------------------------------------------------------------------------ */
typedef struct myslam_lk myslam_lk;
int myslam_lk_create(myslam_lk** out, int win, int max_level, int max_iters, float eps, float min_eig_threshold);
int myslam_lk_destroy(myslam_lk* h);
int myslam_lk_set_stream(myslam_lk* h, void* hip_stream);
/* host pointers (uploads, runs, downloads, synchronises); pts = n x (x, y) float.  A point with a non-finite coordinate (NaN, +-inf, in
 * prev_pts or in the initial flow) is reported lost: status 0, err 0, its position unspecified; so is one whose window origin does not fit
 * an int.  Rows may be padded (prev_step, next_step >= cols, each image with its own); the last row need only reach its last pixel. */
int myslam_lk_track(myslam_lk* h, const uint8_t* prev, const uint8_t* next, int rows, int cols, int prev_step, int next_step,
                    const float* prev_pts, float* next_pts, int n, uint8_t* status, float* err);
/* The same call for a TRACKER that sees one new image per frame (Frontend::TrackLastFrame, src/frontend.cpp:129-172: the `next` image of frame
 * t is the `prev` image of frame t + 1): the handle keeps the device copy and the pyramid of the two images it saw last, named by caller
 * tokens.  A non-zero token promises "the bytes behind this token never change" — an image found under its token is neither uploaded nor
 * down-sampled again; 0 = do not look up, do not remember.  A caller that modifies an image in place (DeepLCD blurs a key-frame's image,
 * src/deeplcd.cpp:46, and cv::Mat copies share pixels) gives it a new token.  Results are bit-identical to myslam_lk_track.
 * myslam_lk_prefetch uploads an image and builds its pyramid asynchronously on the handle's stream into the slot the next
 * myslam_lk_track_cached call does not track FROM (the image must stay valid and unchanged until that call returns): the upload of frame
 * t + 1 then runs beside whatever the caller does with frame t (its pose optimisation). */
int myslam_lk_track_cached(myslam_lk* h, const uint8_t* prev, uint64_t prev_token, const uint8_t* next, uint64_t next_token, int rows, int cols,
                           int prev_step, int next_step, const float* prev_pts, float* next_pts, int n, uint8_t* status, float* err);
int myslam_lk_prefetch(myslam_lk* h, const uint8_t* img, uint64_t token, int rows, int cols, int step);
/* device pointers, asynchronous on the handle's stream: `batch` image pairs (image b at base + b*stride), points of pair b at
 * pts + b*cap*2, d_counts[b] of them valid (counts above cap are read as cap; slots past the count are neither read nor written);
 * d_status batch x cap, d_err batch x cap or NULL */
int myslam_lk_track_batch(myslam_lk* h, const uint8_t* d_prev, const uint8_t* d_next, int batch, int rows, int cols, int step, size_t stride,
                          const float* d_prev_pts, float* d_next_pts, const int32_t* d_counts, int cap, uint8_t* d_status, float* d_err);

/* ------------------------------------------------------------------------------------------
 * Multi-stream tracker — the work the reference does on EVERY frame, Frontend::Track() (src/frontend.cpp:86-122: constant-velocity
 * prediction, TrackLastFrame :127-171, EstimateCurrentPose :176-276, the GOOD / BAD / LOST decision), for `streams` independent cameras
 * of one image size and one calibration, advanced one frame per call with all tracker state in device memory and no host synchronisation.
 * Per stream the handle holds: the last frame's feature table (<= cap features, cap <= 4096: pixel f32 x, y and a slot of the stream's landmark
 * table or -1 = no live map point), the landmark table (<= landmark_cap: MapPoint::Pos() 3 x f64, mbIsOutlier), the reference key-frame's
 * pose7 and frame id, last.rel = RelativePose() of the last frame and _mseRelativeMotion (4 x 4 f64, row-major), the next frame id, the
 * status (0 INITING 1 TRACKING_GOOD 2 TRACKING_BAD 3 LOST, FrontendStatus), a frozen flag, and the previous left image with its LK pyramid
 * (two buffers per stream that swap roles at every step: only the new image is down-sampled).
 *
 * myslam_tracker_step_batch (device pointers: image s at d_left + s * stride, row pitch `step`; asynchronous on the handle's stream, never
 * synchronises, allocation-free, recordable between myslam_graph_begin / _end) does for every stream that is not frozen:
 *   1. cur.rel = rel_motion * last.rel, Tcw = cur.rel * T(ref pose) (:90-93); LK start point of a feature = (float)world2pixel(pos, Tcw) when
 *      its landmark is not an outlier, else its own pixel (:136-147).  f64, every product and sum rounded on its own in the order the hosts write
 *      them (chain.py mm / mv / q_to_R / world2pixel = host/myslam_system.hpp): the start points are the hosts' bits;
 *   2. LK last -> current, the arithmetic of myslam_lk_track (:150-153);
 *   3. ordered compaction: features with status && landmark form the current frame's table in their old order (:156-170); those whose landmark is
 *      not an outlier form the pose-only problem in that order, observations widened to f64 (:183-205);
 *   4. the pose-only optimisation of myslam_pose_only_optimize (chi2 5.991, 4 rounds x 10 iterations, pre_optimize 0) from
 *      pose7(cur.rel * T(ref)) (:176-260);
 *   5. outlier features lose their landmark; the landmark is marked outlier and appended to the stream's outlier list (Map::AddOutlierMapPoint,
 *      feature order) when frame id - ref frame id <= 2 (:261-270); cur.rel = T(pose) * T(ref)^-1; status from the inlier count (> tracking_good:
 *      GOOD, > tracking_bad: BAD, else LOST, :97-110); rel_motion = cur.rel * last.rel^-1 (:122); last <- cur;
 *   6. one myslam_tracker_result at d_results[s]: pose7(cur.rel * T(ref)), counts, status, frame id, and needs_host = the key-frame rule
 *      (status == TRACKING_BAD, :112; or with kf_every > 0: status != LOST && frame id % kf_every == 0) or LOST.
 * A stream with needs_host set is FROZEN: later steps leave its state, its stored image and d_results[s] untouched until myslam_tracker_set_frame.
 * A stream that was never set is frozen.  status = MYSLAM_ERR_CAPACITY (needs_host 1, frozen) reports a stream whose tables did not fit
 * (set_frame beyond cap / landmark_cap, an outlier list beyond 2 x cap); nothing is ever truncated.  (As the rules stand the list cannot
 * overflow: every entry is a feature of the table set_frame uploaded that loses its landmark in the same step and is therefore never kept again,
 * steps add no features and set_frame empties the list, so it never holds more than n_feat <= cap entries; the clause guards the buffer.)
 * A step is 5 + (pyramid levels above 0) dependent launches (8 with the reference's max_level 3): head (image copy + rule 1), one per pyramid
 * level, LK, compaction, pose-only, tail (rules 5 + 6).
 * ------------------------------------------------------------------------------------------ */
typedef struct myslam_tracker myslam_tracker;
typedef struct myslam_tracker_result {
    double pose7[7];            /* Tcw of the frame, (qx qy qz qw tx ty tz) */
    int32_t n_inliers;          /* features.size() - cntOutliers (:275) */
    int32_t n_features;         /* current frame's feature table */
    int32_t status;             /* FrontendStatus after the frame, or MYSLAM_ERR_CAPACITY */
    int32_t frame_id;
    int32_t needs_host;         /* 1: key-frame work or LOST; the stream is frozen */
    int32_t reserved;
} myslam_tracker_result;
/* win .. min_eig_threshold as myslam_lk_create; tracking_good / tracking_bad = numFeatures.trackingGood / trackingBad */
int myslam_tracker_create(myslam_tracker** out, int streams, int rows, int cols, int cap, int landmark_cap, double fx, double fy, double cx, double cy,
                          int tracking_good, int tracking_bad, int win, int max_level, int max_iters, float eps, float min_eig_threshold);
int myslam_tracker_destroy(myslam_tracker* h);
int myslam_tracker_set_stream(myslam_tracker* h, void* hip_stream);
/* Key-frame hand-off, host pointers, synchronous: uploads one stream's state (after StereoInit / InsertKeyFrame: the frame that becomes `last`)
 * and unfreezes it; the outlier list is emptied.  feat_landmark[i] in [-1, n_landmarks).  prev_image (rows x cols, row pitch image_step) replaces
 * the stored previous image and its pyramid — the reference's DeepLCD blurs a key-frame's image in place and the tracker then tracks FROM the
 * blurred pixels (src/deeplcd.cpp:46); NULL keeps the image of the last step (MYSLAM_ERR_INVALID when the stream never saw one).
 * n_feat > cap or n_landmarks > landmark_cap: MYSLAM_ERR_CAPACITY, and the stream's next result record says so (see above). */
int myslam_tracker_set_frame(myslam_tracker* h, int stream, const float* feat_xy, const int32_t* feat_landmark, int n_feat, const double* landmark_pos,
                             const uint8_t* landmark_outlier, int n_landmarks, const double* ref_pose7, int ref_frame_id, const double* last_rel16,
                             const double* rel_motion16, int next_frame_id, int status, int kf_every, const uint8_t* prev_image, int image_step);
/* downloads the same (arrays sized cap / landmark_cap by the caller; any pointer may be NULL) plus the frozen flag and the landmark slots the
 * steps since set_frame marked outlier, in Map::AddOutlierMapPoint order (outlier_landmarks: 2 x cap entries) */
int myslam_tracker_get_frame(myslam_tracker* h, int stream, float* feat_xy, int32_t* feat_landmark, int* n_feat, double* landmark_pos,
                             uint8_t* landmark_outlier, int* n_landmarks, double* ref_pose7, int* ref_frame_id, double* last_rel16, double* rel_motion16,
                             int* next_frame_id, int* status, int* kf_every, int* frozen, int32_t* outlier_landmarks, int* n_outlier_landmarks,
                             uint8_t* prev_image, int image_step);
int myslam_tracker_step_batch(myslam_tracker* h, const uint8_t* d_left, int step, size_t stride, myslam_tracker_result* d_results);
/* kernel launches one myslam_tracker_step_batch enqueues */
int myslam_tracker_launches_per_step(const myslam_tracker* h);
/* the last step's LK problem of one stream (host pointers, cap entries each, synchronises): p0 = last frame's pixels, p1 = start points (rule 1),
 * tracked / lk_status = LK's output; *n = 0 when the stream was frozen during that step */
int myslam_tracker_debug_last_step(myslam_tracker* h, int stream, float* p0, float* p1, float* tracked, uint8_t* lk_status, int* n);

/* ------------------------------------------------------------------------------------------
 * Key-frame turns on the device — what a frozen stream needed the host for when the key-frame rule fired: Frontend::DetectFeatures' mask
 * (src/frontend.cpp:302-328), FindFeaturesInRight (:335-379), TriangulateNewPoints (:451-488) and the frontend's half of InsertKeyFrame
 * (:422-446), for every eligible stream of the bank at once, written where myslam_backend_insert_keyframe_batch reads a new key-frame.
 * Detection itself stays myslam_orb_detect_batch: masks -> detect_batch (the caller's extractor, same stream) -> turn -> next step.
 *
 * Ids.  Per stream the handle also holds MapPoint::mnId by landmark slot (i64), ref_kf_id = the reference key-frame's mnKFId, next_kf_id and
 * next_mp_id (the id factories, keyframe.cpp:14 / mappoint.cpp:8, per stream) and an "ids valid" flag that myslam_tracker_set_frame CLEARS
 * (a new landmark table has no ids yet).  set_ids / get_ids: host pointers, synchronous, as set_frame / get_frame.  set_ids returns
 * MYSLAM_ERR_INVALID when n_landmarks is not the stream's landmark count, when an id (ref_kf_id and the counters included) is negative or when
 * next_mp_id is not above every landmark id; otherwise it stores the ids and sets the flag.  Each step also records WHY it froze a stream:
 * the key-frame rule, LOST, or capacity (one word of the state, one store in the step's tail; nothing else of a step changes).
 * A stream is ELIGIBLE for a turn when it is frozen, the freezing step recorded "key-frame rule" (not LOST, not capacity, not "never set")
 * and its ids are valid.
 *
 * myslam_tracker_keyframe_masks — 1 launch on the handle's stream, asynchronous: writes every stream's whole mask (rows x cols bytes, mask s at
 * d_masks + s * stride, row pitch `step`: the d_masks layout of myslam_orb_detect_batch).  Eligible stream: 255, then 0 in
 * [cvRound(x - 20), cvRound(x + 20)] x [cvRound(y - 20), cvRound(y + 20)] around every feature of its table, both ends included, clipped to the
 * image; x -+ 20 in f32, cvRound = round to nearest, ties to even (cv::rectangle(pt - (20, 20), pt + (20, 20), 0, CV_FILLED), :305-309).
 * Rectangles overlap freely.  A feature with a non-finite coordinate draws NOTHING (a choice: the hosts cannot reach it, LK never keeps such a
 * point).  Stream not eligible: all 0 (the extractor then finds nothing).  step < cols, a stride that does not hold the image or NULL:
 * MYSLAM_ERR_INVALID; cols > 8192 (8 mask rows of one block live in LDS): MYSLAM_ERR_UNSUPPORTED.
 *
 * myslam_tracker_keyframe_batch — device pointers, asynchronous on the handle's stream, never synchronises, allocates nothing (its scratch
 * is the handle's from create on), recordable between myslam_graph_begin / _end; myslam_tracker_keyframe_launches = 3 + (pyramid levels
 * above 0) dependent launches: head, one per level, LK, tail.  d_right (image s at d_right + s * stride, pitch step) = the right images of the
 * step that froze the streams; d_new_kps S x kp_cap (only x, y are read), d_n_new S (below 0 reads as 0, above kp_cap as kp_cap).
 * For an eligible stream, everything is decided before a byte of its state is written:
 *   a. the detected key-points follow the table's features in order, landmark -1 (:319-323);
 *   b. right start point of a feature whose landmark is not marked outlier = (float)world2pixel_right(pos, Tcw), Tcw = last.rel * T(ref pose):
 *      pc = mv(R, pw) + t, then pc + (-baseline, 0, 0) — f64, each product and sum rounded on its own as in rule 1 of the step; every other
 *      feature starts at its own pixel (:342-353);
 *   c. the right image goes into the stream's FREE image buffer (where the next step's image goes anyway) with its pyramid levels, and LK tracks
 *      left -> right with the arithmetic of myslam_lk_track (:358-361): mvpFeaturesRight[i] = (point, status);
 *   d. every feature with landmark -1 and right status set, in feature order (:456-485), is triangulated with match_tri's solve
 *      (myslam_triangulate_stereo's bits: one device function, csrc/tri_solve.h); where sigma3 / sigma2 < 1e-2 && z > 0 a map point is created:
 *      id = next_mp_id + its rank among the successes, pos = mv(Twc.R, p) + Twc.t with Twc = T_inv(Tcw) (:474-476);
 *   e. the landmark table is rebuilt: slots in order of FIRST reference by the features of the final table, two features on one landmark share
 *      a slot, landmarks nobody names are dropped; outlier flags and ids move with their landmarks;
 *   f. InsertKeyFrame (:422-446): kf_id = next_kf_id++, pose = p7(last.rel * T(ref pose)); ref pose = pose, ref_kf_id = kf_id, ref frame id =
 *      next frame id - 1, last.rel = I; rel_motion and status are kept; the outlier list is emptied, frozen = 0 (ids stay valid);
 *   g. outputs, feature stride = the tracker's cap (the layout myslam_backend_insert_keyframe_batch reads with feat_cap = cap, outlier_cap = 2 cap):
 *      d_new_kf_id S i64 (-1: no turn), d_new_kf_pose S x 7, d_feat_mp_id (-1: none) / d_feat_mp_pos (0 without a map point) / d_feat_uv /
 *      d_feat_tag (= the feature's index) / d_feat_flags (0), d_n_feat (0: no turn); d_outlier_mp_id S x 2 cap = the ids of the stream's outlier
 *      list in its order, read BEFORE the rebuild, d_n_outlier_mp; d_right_xy / d_right_ok S x cap; d_report S x 8 i32 = (turn status, frame id of
 *      the stream's last frame, detected features, right matches, new map points, final feature count, final landmark count, 0).  d_feat_uv with
 *      d_n_feat is also myslam_orb_process_keyframes_batch's d_feat_xy.  Rows from a count on, and the feature rows of a refused turn, are
 *      unspecified.
 * Turn status: 0 taken; MYSLAM_TRACKER_NO_TURN the stream was not eligible — its state, stored images and pyramids keep every byte;
 * MYSLAM_ERR_CAPACITY when n_feat + n_new > cap or the rebuilt table has more than landmark_cap landmarks — the stream stays frozen with every
 * byte of its state as before (get_frame and a host turn still work; only its free image buffer may hold the right image).
 * Call level, nothing enqueued: NULL pointers, step < cols, a stride that does not hold the image or kp_cap < 1 -> MYSLAM_ERR_INVALID.
 * What myslam_backend_insert_keyframe_batch does with a no-turn item (d_new_kf_id = -1, d_n_feat = 0): on a table that holds a key-frame the id
 * is not above the last one -> that item is refused with MYSLAM_ERR_INVALID and keeps every byte.  On an EMPTY key-frame table there is no last
 * id to compare with and the row (-1, pose) WOULD BE APPENDED: a stream's table holds its StereoInit key-frame before any turn can happen, and a
 * caller that batches other tables must take such items out itself (myslam_mapper_keyframe_batch, MAPPER below, does so on the device: its gate
 * idles every item without a key-frame before the insert reads a table).
 *
 * myslam_tracker_update_from_map_batch — 1 launch.  In the reference the frontend holds the MapPoint / KeyFrame objects the back end and the loop
 * closer move.  Item s = stream s: d_kf_id S x kf_cap ascending / d_kf_pose x 7 / d_n_kf, d_mp_id S x mp_cap ascending / d_mp_pos x 3 /
 * d_mp_outlier / d_n_mp (the tables of myslam_backend_optimize_batch; counts are clamped to [0, cap]).  For every stream that is NOT frozen and whose
 * ids are valid: each landmark whose id is found (binary search) takes that row's position and outlier flag; ref pose takes the pose of the row whose
 * id is ref_kf_id.  Absent ids keep their values.  NULL pointers or a cap < 1: MYSLAM_ERR_INVALID.
 *
 * myslam_tracker_set_image_batch — 1 + levels launches: for every stream with d_select[s] != 0 the stored previous left image becomes d_imgs[s] and
 * its pyramid levels are rebuilt: the device form of set_frame's prev_image (DeepLCD blurs the key-frame's image in place and the tracker then
 * tracks FROM the blurred pixels, src/deeplcd.cpp:46).  Frozen or not.  NULL pointers, step < cols or a short stride: MYSLAM_ERR_INVALID.
 * (The selection lives on the device, so the host-side "this stream has an image" mark of set_frame / get_frame is not touched: a stream that was
 * never given an image through set_frame still reports none to them.)
 * ------------------------------------------------------------------------------------------ */
#define MYSLAM_TRACKER_NO_TURN 1    /* d_report[s][0]: the stream was not eligible, nothing of it was touched */
int myslam_tracker_set_ids(myslam_tracker* h, int stream, const int64_t* landmark_id, int n_landmarks, int64_t ref_kf_id, int64_t next_kf_id,
                           int64_t next_mp_id);
/* landmark_id sized landmark_cap by the caller; any pointer may be NULL */
int myslam_tracker_get_ids(myslam_tracker* h, int stream, int64_t* landmark_id, int* n_landmarks, int64_t* ref_kf_id, int64_t* next_kf_id,
                           int64_t* next_mp_id, int* valid);
int myslam_tracker_keyframe_masks(myslam_tracker* h, uint8_t* d_masks, int step, size_t stride);
int myslam_tracker_keyframe_batch(myslam_tracker* h, const uint8_t* d_right, int step, size_t stride, const myslam_keypoint* d_new_kps,
                                  const int32_t* d_n_new, int kp_cap, double baseline, int64_t* d_new_kf_id, double* d_new_kf_pose, int64_t* d_feat_mp_id,
                                  double* d_feat_mp_pos, float* d_feat_uv, int32_t* d_feat_tag, uint8_t* d_feat_flags, int32_t* d_n_feat,
                                  int64_t* d_outlier_mp_id, int32_t* d_n_outlier_mp, float* d_right_xy, uint8_t* d_right_ok, int32_t* d_report);
/* kernel launches one myslam_tracker_keyframe_batch enqueues */
int myslam_tracker_keyframe_launches(const myslam_tracker* h);
/* the last turn's problem of one stream (host pointers, cap entries each, synchronises): left pixels of the final table, LK's right points and
 * status, the triangulation in the camera frame and its ok (0 where none was attempted); *n = 0 when the stream took no turn in that call */
int myslam_tracker_debug_last_turn(myslam_tracker* h, int stream, float* left_xy, float* right_xy, uint8_t* right_ok, double* tri_xyz, uint8_t* tri_ok,
                                   int* n);
/* test seam (host call, synchronous): freezes a stream as a step would and records `why` = 1 key-frame rule, 2 LOST, 3 capacity — so that a
 * hand-made table (set_frame, any coordinates and counts) can meet the masks and the turn without a step's LK in between */
int myslam_tracker_debug_freeze(myslam_tracker* h, int stream, int why);
int myslam_tracker_update_from_map_batch(myslam_tracker* h, const int64_t* d_kf_id, const double* d_kf_pose, const int32_t* d_n_kf, int kf_cap,
                                         const int64_t* d_mp_id, const double* d_mp_pos, const uint8_t* d_mp_outlier, const int32_t* d_n_mp, int mp_cap);
int myslam_tracker_set_image_batch(myslam_tracker* h, const uint8_t* d_imgs, int step, size_t stride, const uint8_t* d_select);

/* ------------------------------------------------------------------------------------------
 * StereoInit on the device — how a stream STARTS: Frontend::StereoInit (src/frontend.cpp:282-295) with DetectFeatures over an empty feature
 * table (:305-309, :312-313 the init extractor, :319-323), FindFeaturesInRight (:335-379; every start point is the feature's own pixel,
 * :350-352, :358-361), BuildInitMap (:385-417) and InsertKeyFrame's INITING branch (:427-428, :441-443), for every init-eligible stream of
 * the bank at once: masks -> detect_batch (the caller's INIT extractor, same stream) -> init -> first step.
 *
 * A stream is INIT-ELIGIBLE when it is frozen, its status is INITING (0), no step recorded why it froze and set_frame left no overflow: a
 * stream as myslam_tracker_create leaves it (every counter 0, kf_every 0: the reference's id factories at program start) or as
 * myslam_tracker_reset_stream leaves it.  No stream is eligible for an init and for a turn at once.
 *
 * myslam_tracker_reset_stream — host call, synchronous as set_frame / set_ids: puts the stream back into the created state (no features, no
 * landmarks, empty outlier list, last.rel = rel_motion = I, ref pose = (0, 0, 0, 1, 0, 0, 0), ref frame id 0, frozen, nothing recorded, no
 * overflow, ids not valid, ref_kf_id 0) with the given counters: a restart after LOST, or streams that share an id space.  A negative value:
 * MYSLAM_ERR_INVALID.  The stream's image buffers keep their roles and the host-side "this stream has an image" mark is left alone.
 *
 * myslam_tracker_init_masks — 1 launch on the handle's stream, asynchronous, the layout of myslam_tracker_keyframe_masks: mask s is all 255 for
 * an init-eligible stream (no feature draws a rectangle) and all 0 otherwise.  NULL, step < cols or a stride that does not hold the image:
 * MYSLAM_ERR_INVALID.  No LDS, so no limit on cols.
 *
 * myslam_tracker_init_batch — device pointers, asynchronous on the handle's stream, never synchronises, allocates nothing (its scratch is the
 * turn's plus one selector array, the handle's from create on), recordable between myslam_graph_begin / _end; myslam_tracker_init_launches =
 * 3 + 2 x (pyramid levels above 0) dependent launches: head, the left image's levels, the right image's levels, LK, tail.  d_left / d_right share
 * step and stride; d_new_kps, d_n_new, kp_cap, baseline and the thirteen outputs are those of myslam_tracker_keyframe_batch, same layout.
 * For an init-eligible stream, everything is decided before a byte of its state is written:
 *   a. m = clamp(d_n_new[s], 0, kp_cap) features = the detected key-points in order, landmark -1 (:319-323);
 *   b. the left image goes into the stream's image buffer `slot` (where a step looks for the previous image) and the right image into the other
 *      one, each with its pyramid levels; LK tracks left -> right from every feature's own pixel with the arithmetic of myslam_lk_track;
 *      nRight = the number of set statuses;
 *   c. nRight < init_good (:285-287): MYSLAM_TRACKER_INIT_RETRY.  next frame id += 1 (the Frame was constructed) and nothing else of the
 *      state changes: the stream stays init-eligible.  d_new_kf_id = -1, d_n_feat = 0, d_n_outlier_mp = 0;
 *   d. otherwise BuildInitMap: every feature with right status set, in feature order, is triangulated with match_tri's solve (the P and point
 *      expressions of the turn's rule d: myslam_triangulate_stereo's bits); where sigma3 / sigma2 < 1e-2 && z > 0 a map point is created:
 *      id = next_mp_id + its rank among the successes, pos = the solve's X itself (the key-frame's pose is the identity and the hosts do not
 *      multiply by it);
 *   e. landmark table: a success's slot = its rank, outlier flags 0; every other feature keeps landmark -1; all m features stay in the table;
 *   f. InsertKeyFrame, INITING branch: kf_id = next_kf_id++, pose = (0, 0, 0, 1, 0, 0, 0) = ref pose, ref_kf_id = kf_id, ref frame id = next
 *      frame id, then next frame id += 1; last.rel = rel_motion = I; status = TRACKING_GOOD (:291), frozen = 0, nothing recorded, the outlier
 *      list empty, next_mp_id += successes, ids valid.  `slot` is unchanged: the left image is the stream's previous image for the next step.
 *      Zero successes still insert the key-frame (BuildInitMap returns true);
 *   g. outputs as the turn's rule g with d_n_outlier_mp = 0; d_report[s] = (status, frame id, m, nRight, successes, m, successes, 0).  The
 *      turn's scratch is filled, so myslam_tracker_debug_last_turn reads an init like a turn.
 * Report of an item without a key-frame: (status, frame id, m, nRight or 0, 0, the state's feature count, its landmark count, 0), frame id =
 * the id the constructed Frame took (retry, capacity) or the stream's last frame (not eligible).
 * Not eligible: MYSLAM_TRACKER_NO_TURN — state, stored images and pyramids keep every byte; a turn-eligible stream of the same bank is not
 * touched by this call, nor an init-eligible one by myslam_tracker_keyframe_batch.  MYSLAM_ERR_CAPACITY when m > cap or successes >
 * landmark_cap: the state keeps every byte, frame id included; only the two image buffers may have been written.
 * Call level, nothing enqueued: NULL pointers, step < cols, a stride that does not hold the image or kp_cap < 1 -> MYSLAM_ERR_INVALID;
 * init_good may be any int.
 * The outputs feed myslam_backend_insert_keyframe_batch on an EMPTY table: the first id has nothing to be above, so the row is appended and
 * every success becomes a map-point row (take retry / no-turn items out first, see above).
 * As after myslam_tracker_set_image_batch, set_frame(..., prev_image = NULL) still reports "no image" after a device init: the images arrived
 * on the device and the host-side mark was not touched.
 * ------------------------------------------------------------------------------------------ */
#define MYSLAM_TRACKER_INIT_RETRY 2 /* d_report[s][0]: fewer than init_good right matches, only the frame id advanced */
int myslam_tracker_reset_stream(myslam_tracker* h, int stream, int next_frame_id, int64_t next_kf_id, int64_t next_mp_id, int kf_every);
int myslam_tracker_init_masks(myslam_tracker* h, uint8_t* d_masks, int step, size_t stride);
int myslam_tracker_init_batch(myslam_tracker* h, const uint8_t* d_left, const uint8_t* d_right, int step, size_t stride, const myslam_keypoint* d_new_kps,
                              const int32_t* d_n_new, int kp_cap, double baseline, int init_good, int64_t* d_new_kf_id, double* d_new_kf_pose,
                              int64_t* d_feat_mp_id, double* d_feat_mp_pos, float* d_feat_uv, int32_t* d_feat_tag, uint8_t* d_feat_flags, int32_t* d_n_feat,
                              int64_t* d_outlier_mp_id, int32_t* d_n_outlier_mp, float* d_right_xy, uint8_t* d_right_ok, int32_t* d_report);
/* kernel launches one myslam_tracker_init_batch enqueues */
int myslam_tracker_init_launches(const myslam_tracker* h);

/* ------------------------------------------------------------------------------------------
 * Lens undistortion — replaces Camera::UndistortImage (src/camera.cpp:36-48), which Frontend::GrabStereoImage runs on the left and the
 * right image before anything else when Camera.bNeedUndistortion is 1 (src/frontend.cpp:47-51): cv::undistort(src, dst, K, D) with
 * K = (fx, fy, cx, cy) widened from the camera's float members and D = (k1, k2, p1, p2) (read in src/system.cpp:118-138).
 * The handle holds the map of one camera at one image size: built at create time on the host in f64 the way OpenCV 3.4 builds it (stripes
 * of min(max(1, 4096 / cols), rows) rows, initUndistortRectifyMap(..., CV_16SC2)), then bilinear remap in fixed point with border 0.
 * Results are OpenCV's integers (tests/undistort_ref.py restates them; parity against OpenCV itself is unpinned, tests/test_opencv_pin_undistort.py).
 * MYSLAM_ERR_UNSUPPORTED: the source band of a single 128-pixel tile row exceeds 64 KiB (a map far from the identity).
 * ------------------------------------------------------------------------------------------ */
typedef struct myslam_undistort myslam_undistort;
/* camera.cpp:36-48: K = fx fy cx cy, D = k1 k2 p1 p2 (float, as the reference holds them) */
int myslam_undistort_create(myslam_undistort** out, int rows, int cols, const float* K, const float* D);
int myslam_undistort_destroy(myslam_undistort* h);
int myslam_undistort_set_stream(myslam_undistort* h, void* hip_stream);
/* frontend.cpp:47-51, one image: host pointers (uploads, runs, downloads, synchronises); src == dst is allowed (the reference's in-place call) */
int myslam_undistort_image(myslam_undistort* h, const uint8_t* src, int src_step, uint8_t* dst, int dst_step);
/* frontend.cpp:47-51 for `batch` images (image b at base + b * stride): device pointers, asynchronous on the handle's stream, allocation-free
 * (recordable between myslam_graph_begin / _end).  Source and destination may not overlap (MYSLAM_ERR_INVALID): the remap is a gather. */
int myslam_undistort_batch(myslam_undistort* h, const uint8_t* d_src, int batch, int src_step, size_t src_stride, uint8_t* d_dst, int dst_step,
                           size_t dst_stride);
/* camera.cpp:36-48's two maps as OpenCV's initUndistortRectifyMap gives them, host function: xy = rows x cols x 2 int16 (CV_16SC2),
 * frac = rows x cols uint16 (CV_16UC1: (v & 31) * 32 + (u & 31) in 1/32 px); either may be NULL */
int myslam_undistort_get_map(const myslam_undistort* h, int16_t* xy, uint16_t* frac);

/* ------------------------------------------------------------------------------------------
 * Loop correction — replaces the g2o part of LoopClosing::PoseGraphOptimization (src/loopclosing.cpp:537-610) and the map-point
 * write-back that follows it (:612-640).   [SURVEY.md §8(f) rank 3]
 * poses: n x 7 (qx qy qz qw tx ty tz) Tcw of every key-frame, in/out (VertexPose, :548-565); fixed[i] != 0 for the key-frames the
 * reference fixes (:557-562: active window, loop key-frame, key-frame 0); edge k = EdgePoseGraph between poses edge_v0[k] and
 * edge_v1[k] with measurement meas[k] (7 doubles, = T[v0] * T[v1]^-1 when the edge is satisfied: mRelativePoseToLastKF :577-588,
 * mRelativePoseToLoopKF :590-601), information I6, error log(meas^-1 * T[v0] * T[v1]^-1) (include/myslam/g2o_types.h:157-167),
 * Jacobians by g2o's central differences (delta 1e-9; the analytic linearizeOplus is commented out at g2o_types.h:168-182).
 * Runs g2o's Levenberg for max_iters (20, :606) iterations.  *final_chi2 = sum of e^T e at the returned poses, *iters = iterations
 * done.  Host pointers; uploads, runs and downloads synchronously on the calling thread's own non-blocking stream (never the
 * legacy null stream).
 * Solver structure: key-frames in index order form the chain; every edge that does not join neighbouring free key-frames adds
 * one separator key-frame to a dense Schur block; long chain runs are cut by further separators so that the serial
 * block-tridiagonal sweeps run in parallel.  Up to 96 separators in all, the fast path keeps the Schur pivots in LDS; graphs
 * whose natural separators fit 96 stay on it (their cuts are coarsened until they fit).  Beyond that the general path takes up
 * to 1024 separators, cuts included (MYSLAM_ERR_UNSUPPORTED beyond), with pivots and right-hand side in device memory: about
 * (32 ntile 256 + 2 ldz^2 + 2 rowsPad ldz) * 8 bytes for the call, ldz = 6 |S| + 1 rounded up to 16, ntile = (ldz/16)(ldz/16 + 1)/2,
 * rowsPad = 6 (chain key-frames) rounded up to 4 — ~6 GB near the limit (1012 separators), where one Levenberg iteration takes ~7.3 s on an MI355X.
 * ------------------------------------------------------------------------------------------ */
int myslam_pose_graph_optimize(double* poses, int n, const uint8_t* fixed, const int32_t* edge_v0, const int32_t* edge_v1,
                               const double* meas, int n_edges, int max_iters, double* final_chi2, int* iters);
/* src/loopclosing.cpp:621-633: points[i] <- T_new[first_kf[i]]^-1 * (T_old[first_kf[i]] * points[i]) — each map point outside the
 * active window keeps its camera-frame position in the key-frame that first observed it; first_kf[i] < 0 leaves the point alone
 * (the :625-629 skip).  old_poses / new_poses: n_poses x 7 as above; points n_points x 3 in/out. */
int myslam_correct_map_points(const double* old_poses, const double* new_poses, int n_poses, const int32_t* first_kf, double* points, int n_points);
/* LoopClosing::LoopLocalFusion, src/loopclosing.cpp:466-507 — the arithmetic of it (re-linking the current key-frame's observations to the
 * loop key-frame's map points, :509-532, is Map bookkeeping and stays with the caller).  active_poses: n_active x 7 Tcw of the active
 * key-frames, in/out; cur = index of the current key-frame among them; corrected_cur_pose7 = _mseCorrectedCurrentPose.
 * Every active key-frame moves rigidly with the current one (Ta' = Ta * Tc^-1 * Tc'); every map point i keeps its camera-frame position
 * in the active key-frame first_active_kf[i] that first observes it (< 0: left alone).  Host pointers. */
int myslam_loop_local_fusion(double* active_poses, int n_active, int cur, const double* corrected_cur_pose7, const int32_t* first_active_kf,
                             double* points, int n_points);
/* device pointers, asynchronous on hip_stream; *d_status (zeroed by the caller) receives MYSLAM_ERR_INVALID for an index >= n_poses */
int myslam_correct_map_points_device(const double* d_old_poses, const double* d_new_poses, int n_poses, const int32_t* d_first_kf,
                                     double* d_points, int n_points, int32_t* d_status, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * Loop verification — replaces cv::solvePnPRansac(vLoopPoints3d, vCurrentPoints2d, K, cv::Mat(), rvec, tvec, false, 100, 5.991, 0.99)
 * followed by cv::Rodrigues in LoopClosing::ComputeCorrectPose (src/loopclosing.cpp:262-272).   [SURVEY.md §8(f) rank 3]
 * pts3d n x 3 / pts2d n x 2 floats (cv::Point3f / cv::Point2f arrays as the reference builds them, :215-231); iterations = 100,
 * reproj_error = 5.991 (pixels), confidence = 0.99 at the call site.  pose7 = (qx qy qz qw tx ty tz): Sophus::SE3d(R, t) of :270-272.
 * inlier (optional, n flags) / *n_inliers: the RANSAC consensus set (the reference does not ask OpenCV for it).
 * OpenCV 3.4 semantics kept: cv::RNG((uint64)-1) drives 5-point samples, EPnP per sample, squared reprojection error against
 * threshold^2 in float, best-count bookkeeping with the shrinking iteration budget, then a least-squares refinement on the
 * consensus set (Levenberg-Marquardt from the RANSAC model instead of OpenCV's DLT restart: the same minimiser).
 * Returns MYSLAM_ERR_UNSUPPORTED when n < 5 or no model was found (OpenCV returns false there).  Host pointers, synchronous.
 * ------------------------------------------------------------------------------------------ */
int myslam_solve_pnp_ransac(const float* pts3d, const float* pts2d, int n, double fx, double fy, double cx, double cy, int iterations,
                            double reproj_error, double confidence, double* pose7, uint8_t* inlier, int* n_inliers);

/* The same for a BATCH of loop candidates on the device (several streams of cameras against one loop database verify several candidates per
 * step): a handle owns every buffer the calls need — samples max_batch x max_iterations x 5 int32, models x 12 doubles, counts, the f64 copies of the
 * chain below — so the two batch calls allocate nothing, never synchronise, never read device memory from the host and can be recorded between
 * myslam_graph_begin / _end.  cap = match slots per item, <= 4096 (the pose-only kernel's limit); max_iterations <= 100000; beyond: MYSLAM_ERR_CAPACITY. */
typedef struct myslam_pnp myslam_pnp;
int myslam_pnp_create(myslam_pnp** out, int max_batch, int cap, int max_iterations);
int myslam_pnp_destroy(myslam_pnp* h);
int myslam_pnp_set_stream(myslam_pnp* h, void* hip_stream);
/* cv::solvePnPRansac + cv::Rodrigues of src/loopclosing.cpp:262-272 for `batch` items, per item the semantics (and the bits of mask, count and
 * winner) of myslam_solve_pnp_ransac; RANSACPointSetRegistrator::getSubset runs on the device, one lane per item, because the counts live there.
 * Device pointers, asynchronous on the handle's stream.  d_pts3d batch x cap x 3, d_pts2d batch x cap x 2 (cap = the handle's), d_counts batch: a count
 * below 0 is read as 0, one above cap as cap; slots from an item's count on are never read.  d_status[b] = 0: a model was found; 1: none (fewer than
 * 5 points, or no hypothesis won) — then d_pose7[b] is left as it was (OpenCV leaves rvec / tvec alone), d_n_inliers[b] = 0.  d_inlier batch x cap:
 * slots from the count on, and the row of an item without a model, are 0.  batch / iterations beyond the handle's: MYSLAM_ERR_CAPACITY, nothing enqueued. */
int myslam_solve_pnp_ransac_batch(myslam_pnp* h, const float* d_pts3d /* batch x cap x 3 */, const float* d_pts2d /* batch x cap x 2 */,
                                  const int32_t* d_counts, int batch, double fx, double fy, double cx, double cy,
                                  int iterations, double reproj_error, double confidence,
                                  double* d_pose7 /* batch x 7 */, uint8_t* d_inlier /* batch x cap */,
                                  int32_t* d_n_inliers, int32_t* d_status);
/* The arithmetic of LoopClosing::ComputeCorrectPose (src/loopclosing.cpp:208-335) for `batch` candidates in one enqueue: fewer than min_matches (10)
 * matches -> give up (:252); PnP-RANSAC as above (:262-272); OptimizeCurrentPose (:275, :339-433) = myslam_pose_only_optimize_batch with
 * pre_optimize 1 over ALL the item's matches, points and pixels widened (double)float, started from PnP's pose (chi2_th 5.991, rounds 4, iters 10 at the
 * call site); fewer than min_matches inliers after it -> give up (:279).  d_status[b] = MYSLAM_VERIFY_*.  CONFIRMED and FEW_INLIERS write the
 * optimised d_pose7[b], the item's d_outlier flags (vEdgeIsOutlier) and d_n_inliers[b]; NO_MODEL and FEW_MATCHES leave d_pose7[b] alone and report 0 inliers.
 * d_outlier batch x cap: slots from the count on, and the rows of items that did not reach the optimisation, are 0.  d_pnp_pose7 (batch x 7) /
 * d_pnp_inlier (batch x cap), either may be NULL: PnP's own pose (items with a model only) and consensus mask. */
#define MYSLAM_VERIFY_CONFIRMED 0
#define MYSLAM_VERIFY_NO_MODEL 1
#define MYSLAM_VERIFY_FEW_MATCHES 2
#define MYSLAM_VERIFY_FEW_INLIERS 3
int myslam_loop_verify_batch(myslam_pnp* h, const float* d_pts3d, const float* d_pts2d, const int32_t* d_counts, int batch,
                             double fx, double fy, double cx, double cy, int iterations, double reproj_error, double confidence,
                             int min_matches, double chi2_th, int rounds, int iters,
                             double* d_pose7, uint8_t* d_outlier, int32_t* d_n_inliers, int32_t* d_status,
                             double* d_pnp_pose7, uint8_t* d_pnp_inlier);

/* ------------------------------------------------------------------------------------------
 * Loop correction for a BATCH of confirmed loops on the device — the arithmetic of LoopClosing::LoopCorrect (src/loopclosing.cpp:437-463) for
 * `batch` independent maps in one enqueue, reading myslam_loop_verify_batch's d_pose7 / d_status where that call left them: the loop edge of
 * :328-330, the need-correct test of :284-289, LoopLocalFusion (:470-507), PoseGraphOptimization (:537-610) and its write-back (:612-641).
 * The one-map, host-pointer forms stay: myslam_loop_local_fusion, myslam_pose_graph_optimize, myslam_correct_map_points.
 * A handle owns every scratch buffer (per item: the working poses, Jacobians, the block-tridiagonal chain, the dense separator system), so
 * myslam_loop_correct_batch allocates nothing, never synchronises, never reads device memory from the host and can be recorded between
 * myslam_graph_begin / _end.  One workgroup solves one map from start to finish (csrc/loop_correct.hip): Levenberg's control flow runs on the device.
 * Item b is one map; tables are strided by the handle's caps, slots from an item's count on are never read or written:
 *   d_poses            batch x kf_cap x 7 f64, in/out   GetAllKeyFrames() as Tcw (qx qy qz qw tx ty tz), ascending id; row 0 is key-frame 0
 *   d_n_kf             batch i32                        key-frames of the map
 *   d_active           batch x active_cap i32           rows of d_poses that form the active window, strictly ascending;  d_n_active batch i32
 *   d_cur, d_loop      batch i32                        rows of the current and the loop key-frame; cur is in the active list, loop != cur
 *   d_corrected_pose7  batch x 7 f64                    _mseCorrectedCurrentPose: myslam_loop_verify_batch's d_pose7
 *   d_verify_status    batch i32 or NULL                myslam_loop_verify_batch's d_status; NULL = every item is confirmed
 *   d_edge_v0 / _v1    batch x edge_cap i32, in/out     the edges of :568-602 as they stand BEFORE this loop (v0 != v1);  d_meas batch x edge_cap x 7 f64,
 *                                                       in/out: T[v0] * T[v1]^-1 as measured;  d_n_edges batch i32, in/out
 *   d_points           batch x point_cap x 3 f64, in/out   map points;  d_n_points batch i32
 *   d_first_active     batch x point_cap i32            slot IN THE ITEM'S ACTIVE LIST of the active key-frame that first observes the point; < 0: not an active map point
 *   d_first_kf         batch x point_cap i32            row of the key-frame that first observed the point; < 0: the skip of :627-631.  A stream that
 *                                                       re-links (RE-LINK, below) passes myslam_relink_first_kf_batch's array here: GetObservations().front()
 *                                                       in LIST order, which myslam_map_loop_inputs_batch's d_first_kf is not for a merged target
 * correct_threshold = 1.0 (:285), max_iters = 20 (:606) at the call site.  Per item, in this order:
 *   1. d_verify_status[b] != MYSLAM_VERIFY_CONFIRMED -> MYSLAM_LOOP_CORRECT_SKIPPED, nothing of the item's tables is touched;
 *   2. the edge (cur, loop) with the measurement Tcc * Tloop^-1 (:328-330; Tloop = the loop key-frame's pose as given) is appended at slot d_n_edges[b]
 *      and the count incremented; a full table -> MYSLAM_ERR_CAPACITY, the item untouched;
 *   3. |log(Tcur * Tcc^-1)| <= correct_threshold (:284-289) -> MYSLAM_LOOP_CORRECT_NOT_NEEDED: the edge stays, poses and points keep their bits;
 *   4. LoopLocalFusion (:470-507): every active key-frame becomes Ta * Tcur^-1 * Tcc (cur itself Tcc), renormalised per product as
 *      myslam_loop_local_fusion does; every point with first_active >= 0 keeps its camera-frame position in that key-frame;
 *   5. PoseGraphOptimization (:537-610) over the fixed set {active rows, loop row, row 0}: edge error, numeric Jacobian (delta 1e-9) and Levenberg rules
 *      (lambda init, rho, accept / reject, ten rejected trials, rho == 0, non-finite lambda, a failed pivot = a rejected trial) of
 *      myslam_pose_graph_optimize; d_chi2[b] / d_iters[b] have the meaning of its *final_chi2 / *iters;
 *   6. write-back (:612-641): points with first_active < 0 and first_kf >= 0 move from the pose after step 4 to the optimised pose of that key-frame
 *      (active points are left out, :616-619), the optimised poses of the free key-frames are stored (fixed rows outside the active window keep their bits);
 *   7. MYSLAM_LOOP_CORRECT_DONE.
 * An index out of range (an active row, cur, loop, an edge endpoint >= n_kf, first_active >= n_active, first_kf >= n_kf), a count beyond its cap, an active
 * list that is not strictly ascending, cur outside the active list or cur == loop -> MYSLAM_ERR_INVALID, the item untouched.  Every status but DONE
 * reports d_chi2[b] = 0 and d_iters[b] = 0.  One item's fault never changes another item's result, and an item's bytes depend neither on its position in
 * the batch nor on what else is in it (all sums run in a fixed order).
 * Solver structure: the free key-frames in row order form a block-tridiagonal chain; every edge whose two free endpoints are not neighbours in that
 * order makes its LATER endpoint a separator of a dense Schur system (chosen on the device, no greedy pass).  A map that needs more than
 * MYSLAM_LOOP_CORRECT_MAX_SEPARATORS of them (one per closed loop, 17 over KITTI 00) gets MYSLAM_LOOP_CORRECT_FUSED_ONLY: steps 2 to 4 are done, poses
 * outside the active window and non-active points are untouched, d_iters[b] = 0 — the caller finishes that map with myslam_pose_graph_optimize +
 * myslam_correct_map_points.  Re-linking observations (:509-532) is not part of this call: for tables that live on the device it is RE-LINK, below,
 * which runs after this call and myslam_map_write_backend_batch on this call's d_status (DONE and FUSED_ONLY re-link, every other status skips); for
 * host maps it is the caller's, as for myslam_loop_local_fusion.
 * batch beyond the handle's -> MYSLAM_ERR_CAPACITY, nothing enqueued.
 * ------------------------------------------------------------------------------------------ */
#define MYSLAM_LOOP_CORRECT_DONE 0
#define MYSLAM_LOOP_CORRECT_NOT_NEEDED 1
#define MYSLAM_LOOP_CORRECT_SKIPPED 2
#define MYSLAM_LOOP_CORRECT_FUSED_ONLY 3
#define MYSLAM_LOOP_CORRECT_MAX_SEPARATORS 32
typedef struct myslam_loop_corrector myslam_loop_corrector;
/* LoopClosing::LoopCorrect's workspace (src/loopclosing.cpp:437-463) for max_batch maps of up to kf_cap key-frames, edge_cap edges (the appended one
 * included), active_cap active key-frames and point_cap map points each */
int myslam_loop_corrector_create(myslam_loop_corrector** out, int max_batch, int kf_cap, int edge_cap, int active_cap, int point_cap);
int myslam_loop_corrector_destroy(myslam_loop_corrector* h);
int myslam_loop_corrector_set_stream(myslam_loop_corrector* h, void* hip_stream);
/* src/loopclosing.cpp:284-289, :328-330, :437-463, :470-507, :537-641 as described above.  Device pointers, asynchronous on the handle's stream. */
int myslam_loop_correct_batch(myslam_loop_corrector* h, double* d_poses, const int32_t* d_n_kf, const int32_t* d_active, const int32_t* d_n_active,
                              const int32_t* d_cur, const int32_t* d_loop, const double* d_corrected_pose7, const int32_t* d_verify_status,
                              int32_t* d_edge_v0, int32_t* d_edge_v1, double* d_meas, int32_t* d_n_edges, double* d_points, const int32_t* d_n_points,
                              const int32_t* d_first_active, const int32_t* d_first_kf, int batch, double correct_threshold, int max_iters,
                              double* d_chi2, int32_t* d_iters, int32_t* d_status);
/* The separator rule of myslam_loop_correct_batch for one map, on the host (host arrays, no device needed): the fixed set of :560-562
 * {active rows, loop row, row 0}, then the rule above over the edges given (the appended edge joins two fixed rows and changes nothing).
 * *n_separators, *chain_length (free key-frames left in the chain), *supported = n_separators <= MYSLAM_LOOP_CORRECT_MAX_SEPARATORS. */
int myslam_loop_correct_structure(int n_kf, const int32_t* active, int n_active, int loop, const int32_t* edge_v0, const int32_t* edge_v1, int n_edges,
                                  int* n_separators, int* chain_length, int* supported);

/* ------------------------------------------------------------------------------------------
 * Backend::OptimizeActiveMap (src/backend.cpp:126-266) for a BATCH of active maps that live in device tables — one enqueue takes every map
 * through the graph build (:139-206, the rules of myslam_ba_flatten_window), the solve (:208-243, the kernel of
 * myslam_ba_optimize_active_map_batch) and the write-back (:234-266 with Map::RemoveAllOutlierMapPoints / RemoveOldActiveMapPoints,
 * src/map.cpp:126-175), and leaves each map's tables ready to be the next call's input.  The one-map host forms stay:
 * myslam_ba_flatten_window + myslam_ba_optimize_active_map[_batch] + the caller's own container surgery.
 * A handle owns every buffer (the flat windows, the solve's scratch sized as the host-pointer calls size it, per-edge chi2 and flags), so
 * myslam_backend_optimize_batch allocates nothing, never synchronises, never reads device memory from the host and can be recorded between
 * myslam_graph_begin / _end.  It is three dependent launches on the handle's stream (csrc/backend.hip, one workgroup per map in each).
 * Item b is one map; tables are strided by the handle's caps, slots from an item's count on are never read or written:
 *   d_kf_id        batch x kf_cap i64          Map::GetActiveKeyFrames(): mnKFId, strictly ascending (:135)
 *   d_kf_pose      batch x kf_cap x 7 f64, in/out   Tcw (qx qy qz qw tx ty tz) (:145, :256-258);   d_n_kf  batch i32
 *   d_mp_id        batch x mp_cap i64, in/out  Map::GetActiveMapPoints(): mnId, strictly ascending (:136)
 *   d_mp_pos       batch x mp_cap x 3 f64, in/out   (:169, :259-261)
 *   d_mp_outlier   batch x mp_cap u8, in/out   mbIsOutlier; an input row with the flag set is on the map's outlier list (both places where the
 *                                              reference sets the flag also list the point: src/frontend.cpp:263-264, src/backend.cpp:244-245)
 *   d_n_mp         batch i32, in/out
 *   Observations: EVERY entry of GetObservations() of every active map point is one row (not only the active ones), grouped by map point, in
 *   list order within a map point:
 *   d_obs_mp       batch x obs_cap i32, in/out row of the map point in the item's table, non-decreasing
 *   d_obs_kf       batch x obs_cap i32, in/out row of the observing key-frame in the item's key-frame table, -1 = that key-frame has left the window
 *   d_obs_flags    batch x obs_cap u8, in/out  MYSLAM_BACKEND_OBS_ACTIVE: the feature is in GetActiveObservations(); MYSLAM_BACKEND_OBS_OUTLIER:
 *                                              feature->mbIsOutlier
 *   d_obs_uv       batch x obs_cap x 2 f32, in/out   mkpPosition.pt (:196)
 *   d_obs_tag      batch x obs_cap i32, in/out the caller's own handle of the feature: carried along, never interpreted
 *   d_n_obs        batch i32, in/out
 * The caller's obligation: the reference appends to both observation lists in key-frame order (src/keyframe.cpp:45, src/map.cpp:38), so the ACTIVE
 * rows of a map point in this order are its GetActiveObservations() order, and the first row of a segment is GetObservations().front() (:175).
 * LoopLocalFusion appends observations that are not active (src/loopclosing.cpp:521-525): those rows carry ACTIVE = 0 although their key-frame is
 * in the window.  Nothing has to be refreshed by the host after a removal.
 * Per item:
 *   1. flatten (:139-206): pose slot = key-frame row, landmark slots in map-point row order, edges grouped by landmark in row order.  An edge is an
 *      ACTIVE && !OUTLIER row of a map point that is no outlier (:163, :189); a map point left without an edge gets no slot; a landmark is fixed when
 *      the first row of its segment has d_obs_kf < 0 (:175-177); observations are widened f32 -> f64 (toVec2), poses and positions gathered bit for bit.
 *      MYSLAM_ERR_INVALID: a count negative or beyond its cap, ids not strictly ascending, d_obs_mp decreasing or >= n_mp, d_obs_kf >= n_kf or
 *      < -1, an ACTIVE row with d_obs_kf < 0 (the assert of :187), a map point that is no outlier and has no row.  An item without a single edge:
 *      MYSLAM_BACKEND_EMPTY.  In both cases the item's tables keep every byte, its rows of d_obs_report / d_mp_report / d_obs_chi2 are zero and
 *      d_rounds[b] = d_n_outlier_edges[b] = d_n_new_outlier_mp[b] = 0; the solve does not run for it.
 *   2. solve (:208-243): as myslam_ba_optimize_active_map_batch (huber_delta = chi2_th = 5.991, max_rounds = 5, iters_per_round = 10 at the call site).
 *      d_rounds[b] == max_rounds is reported as it is, not as an error: see MYSLAM_BA_CONVERGED.
 *   3. write-back (:234-266): an edge with chi2 > chi2_th removes its row (RemoveActiveObservation and RemoveObservation, :240-241), every other
 *      edge row gets OUTLIER cleared (:249); a map point whose segment becomes empty is an outlier (:243-246) and its INPUT row is appended to
 *      d_new_outlier_mp[b] (batch x mp_cap i32) in edge order; optimised poses go to d_kf_pose, optimised positions to d_mp_pos of the map points
 *      that had a slot (:256-261); every map point with the outlier flag, old or new, leaves the table with all its rows
 *      (RemoveAllOutlierMapPoints, src/map.cpp:166-175), then every map point without an ACTIVE row (RemoveOldActiveMapPoints, src/map.cpp:126-140);
 *      the map-point and observation tables are compacted in place in their old order, d_obs_mp is renumbered, d_mp_outlier of a kept row is 0 and
 *      the counts are stored.  Rows between a new count and the old one keep their bytes.
 * Reports, indexed by INPUT row:
 *   d_obs_report  batch x obs_cap u8   0 kept, 1 removed as an outlier edge (the feature loses its map point, :247), 2 gone with its map point
 *   d_mp_report   batch x mp_cap u8    0 kept, 1 left the active set, 2 erased as an outlier
 *   d_obs_chi2    batch x obs_cap f64  the edge's chi2 (edge->chi2(), :237), -1 for a row that was not an edge
 *   d_rounds / d_n_outlier_edges  batch i32   the *rounds / *n_outliers of myslam_ba_optimize_active_map;   d_status  batch i32
 * An item's bytes depend neither on its slot in the batch nor on its neighbours.  Map::InsertKeyFrame / RemoveOldActiveKeyframe on
 * the same tables is myslam_backend_insert_keyframe_batch, below (it sets d_obs_kf = -1 and clears ACTIVE on the rows of a key-frame that leaves).
 * Call level, nothing enqueued: NULL pointers, batch < 0, max_rounds / iters_per_round < 1 -> MYSLAM_ERR_INVALID; batch beyond the handle's ->
 * MYSLAM_ERR_CAPACITY.
 * ------------------------------------------------------------------------------------------ */
#define MYSLAM_BACKEND_DONE 0
#define MYSLAM_BACKEND_EMPTY 1
#define MYSLAM_BACKEND_OBS_ACTIVE 1
#define MYSLAM_BACKEND_OBS_OUTLIER 2
typedef struct myslam_backend myslam_backend;
/* Backend::OptimizeActiveMap's workspace (src/backend.cpp:126-266) for max_batch maps of up to kf_cap active key-frames, mp_cap active map points
 * and obs_cap observation rows each.  kf_cap > MYSLAM_BA_MAX_WINDOW_POSES -> MYSLAM_ERR_UNSUPPORTED; out of device memory -> MYSLAM_ERR_CAPACITY. */
int myslam_backend_create(myslam_backend** out, int max_batch, int kf_cap, int mp_cap, int obs_cap);
int myslam_backend_destroy(myslam_backend* h);
int myslam_backend_set_stream(myslam_backend* h, void* hip_stream);
/* src/backend.cpp:126-266 and src/map.cpp:126-175 as described above.  Device pointers, asynchronous on the handle's stream. */
int myslam_backend_optimize_batch(myslam_backend* h, const int64_t* d_kf_id, double* d_kf_pose, const int32_t* d_n_kf, int64_t* d_mp_id, double* d_mp_pos,
                                  uint8_t* d_mp_outlier, int32_t* d_n_mp, int32_t* d_obs_mp, int32_t* d_obs_kf, uint8_t* d_obs_flags, float* d_obs_uv,
                                  int32_t* d_obs_tag, int32_t* d_n_obs, int batch, double fx, double fy, double cx, double cy, double huber_delta,
                                  double chi2_th, int max_rounds, int iters_per_round, uint8_t* d_obs_report, uint8_t* d_mp_report,
                                  int32_t* d_new_outlier_mp, int32_t* d_n_new_outlier_mp, double* d_obs_chi2, int32_t* d_rounds,
                                  int32_t* d_n_outlier_edges, int32_t* d_status);
/* launches one myslam_backend_optimize_batch enqueues (3: flatten, solve, write-back) */
int myslam_backend_launches_per_call(const myslam_backend* h);
/* What the last optimise's solve left, as device pointers that stay valid until destroy: *d_points max_batch x mp_cap x 3 f64 by landmark slot,
 * *d_mp_slot max_batch x mp_cap i32 = the landmark slot of every INPUT map-point row, -1 = it had no vertex.  For myslam_map_attach_solve. */
int myslam_backend_solve_view(const myslam_backend* h, const double** d_points, const int32_t** d_mp_slot);
/* The flat window (src/backend.cpp:139-206) of one item as the last call built it, in myslam_ba_flatten_window's outputs: host pointers (any but sizes3
 * may be NULL) of kf_cap / mp_cap / obs_cap elements, sizes3 = (poses, landmarks, edges), all 0 for an item that was refused or empty.  Synchronises. */
int myslam_backend_debug_flat(myslam_backend* h, int item, int32_t* pose_src, int32_t* pt_src, int32_t* edge_pose, int32_t* edge_pt, double* edge_obs,
                              int32_t* edge_src, uint8_t* fixed, int32_t* sizes3);
/* What the solve (src/backend.cpp:208-243) left for that flat window: poses, landmark positions, per-edge chi2 and outlier flags in slot / edge order,
 * rounds_outliers2 = (*rounds, *n_outliers).  Host pointers, any may be NULL.  Synchronises. */
int myslam_backend_debug_solved(myslam_backend* h, int item, double* poses, double* points, double* edge_chi2, uint8_t* edge_outlier,
                                int32_t* rounds_outliers2);
/* Map::InsertKeyFrame (src/map.cpp:17-48) with KeyFrame::CreateKF's observation loop (src/keyframe.cpp:34-50), RemoveOldActiveKeyframe (:78-120),
 * RemoveOldActiveMapPoints (:126-140), Map::AddOutlierMapPoint (:159-164) and MapPoint::AddObservation / AddActiveObservation /
 * RemoveActiveObservation (src/mappoint.cpp:19-44) for a batch of maps held in the tables of myslam_backend_optimize_batch: the call that adds a
 * key-frame to them, so that insert -> optimise -> insert ... runs without the host touching a table.  Same handle, caps and stream (ordered with
 * optimize_batch); the handle holds a copy of the map-point and observation tables and the index arrays, so the call allocates nothing, never
 * synchronises, never reads device memory from the host and can be recorded between myslam_graph_begin / _end.  One launch, one workgroup per item
 * (k_backend_insert), block scans and binary searches, no global atomics; an item's bytes depend neither on its slot nor on its neighbours.  The
 * features are ranked by (id, index) with a count over all pairs: quadratic in the features of one key-frame (hundreds).
 * All thirteen tables are in/out here, d_kf_id and d_n_kf included.  The new key-frame of item b:
 *   d_new_kf_id   batch i64;   d_new_kf_pose  batch x 7 f64 (Tcw)
 *   d_feat_mp_id  batch x feat_cap i64      mvpFeaturesLeft order; -1 = mpMapPoint.lock() == nullptr
 *   d_feat_mp_pos batch x feat_cap x 3 f64  read for the first feature naming an id that is not in the table
 *   d_feat_uv / d_feat_tag / d_feat_flags   batch x feat_cap (x 2 f32 / i32 / u8: only MYSLAM_BACKEND_OBS_OUTLIER may be set);   d_n_feat  batch i32
 *   optional, d_n_prior == NULL = none: GetObservations() of map points that had left the active set (LoopLocalFusion, src/loopclosing.cpp:521-525),
 *   d_prior_mp_id non-decreasing, d_prior_kf_id the observer's mnKFId, flags without ACTIVE; batch x prior_cap rows
 *   optional, d_n_outlier_mp == NULL = none: ids passed to Map::AddOutlierMapPoint since the last call (src/frontend.cpp:263-264); batch x outlier_cap
 * feat_cap, prior_cap, outlier_cap are strides.  Per item, everything is decided before anything is written:
 *   0. every id of d_outlier_mp_id that is in the map-point table gets d_mp_outlier = 1; other ids are ignored.
 *   1. d_new_kf_id must be above the table's last id (mnKFId comes from a counter); the row is appended with its pose.
 *   2. every feature with an id, in feature order: an id in the table gets one row at the END of its segment (both lists push_back), an outlier map
 *      point included (the reference does not look at mbIsOutlier here); an id that is not in the table enters it at its sorted position with the
 *      position of the first feature naming it and d_mp_outlier = 0, its segment starts with that id's prior rows in prior order (d_obs_kf resolved
 *      against the FINAL key-frame table, -1 if absent, ACTIVE never set), the new key-frame's rows follow.  A new row is d_obs_kf = the new
 *      key-frame's row, flags = ACTIVE | (d_feat_flags & OUTLIER), the feature's uv and tag.  Prior rows of ids that are in the table or that no
 *      feature names are ignored.  Two features naming one id give two rows.
 *   3. if the key-frame count does not exceed `window` (Map.activeMap.size, :44) the call is done: nothing leaves, not even a map point without an
 *      ACTIVE row.
 *   4. otherwise (:78-120), for each OTHER key-frame in id order dis = |log(T_kf * T_new^-1)| (d_dis, batch x kf_cap f64 by INPUT row, -1 elsewhere)
 *      goes through the reference's scan as written: maxDis = 0, minDis = 9999, both ids 0; `if (dis > maxDis) .. else if (dis < minDis) ..`, so a
 *      distance that raises the maximum is never a candidate for the minimum and ties keep the earlier key-frame.  minDis < min_dis_th (0.2, :101)
 *      ? minKFId : maxKFId leaves; an id that is none of the other key-frames' (every distance NaN and no key-frame 0: .at() throws) is
 *      MYSLAM_ERR_INVALID.  The row leaves both key-frame arrays; rows with its d_obs_kf get -1 and ACTIVE cleared (RemoveActiveObservation: the row
 *      stays in GetObservations()), larger d_obs_kf are renumbered.
 *   5. then every map point without an ACTIVE row leaves with all its rows (:126-140); both tables are compacted in their order, d_obs_mp is
 *      renumbered, the counts are stored.  Rows between a new count and the old one keep their bytes.
 * Reports: d_feat_row (batch x feat_cap i32) the FINAL row of each feature's observation, -1 without a map point: the caller's handle of the feature;
 * d_mp_new_row (batch x mp_cap i32, by INPUT row) the row after the call, -1 if it left; d_removed_kf_id / d_removed_kf_row (batch i64 / i32, INPUT
 * row) -1 when none; d_status 0 or an error.  A refused item keeps every byte of its tables; its report rows (as far as its counts reach, d_dis whole)
 * are -1.  MYSLAM_ERR_INVALID: a count negative or beyond its cap, window < 1, the table checks of myslam_backend_optimize_batch (ids strictly
 * ascending, d_obs_mp / d_obs_kf in range and d_obs_mp non-decreasing, no ACTIVE row with d_obs_kf < 0), the new id not above the last, a feature id
 * below -1, prior ids decreasing, a feature or prior flag with a bit other than OUTLIER (so a prior row with ACTIVE).  MYSLAM_ERR_CAPACITY: the
 * key-frame, merged map-point or merged observation count BEFORE the removal exceeds its cap.
 * Call level, nothing enqueued: NULL required pointers, batch < 0, a negative stride -> MYSLAM_ERR_INVALID; batch beyond the handle's, feat_cap or
 * prior_cap beyond obs_cap -> MYSLAM_ERR_CAPACITY. */
int myslam_backend_insert_keyframe_batch(myslam_backend* h, int64_t* d_kf_id, double* d_kf_pose, int32_t* d_n_kf, int64_t* d_mp_id, double* d_mp_pos,
                                         uint8_t* d_mp_outlier, int32_t* d_n_mp, int32_t* d_obs_mp, int32_t* d_obs_kf, uint8_t* d_obs_flags,
                                         float* d_obs_uv, int32_t* d_obs_tag, int32_t* d_n_obs, const int64_t* d_new_kf_id, const double* d_new_kf_pose,
                                         const int64_t* d_feat_mp_id, const double* d_feat_mp_pos, const float* d_feat_uv, const int32_t* d_feat_tag,
                                         const uint8_t* d_feat_flags, const int32_t* d_n_feat, int feat_cap, const int64_t* d_prior_mp_id,
                                         const int64_t* d_prior_kf_id, const float* d_prior_uv, const int32_t* d_prior_tag, const uint8_t* d_prior_flags,
                                         const int32_t* d_n_prior, int prior_cap, const int64_t* d_outlier_mp_id, const int32_t* d_n_outlier_mp,
                                         int outlier_cap, int batch, int window, double min_dis_th, int32_t* d_feat_row, int32_t* d_mp_new_row,
                                         int64_t* d_removed_kf_id, int32_t* d_removed_kf_row, double* d_dis, int32_t* d_status);
/* launches one myslam_backend_insert_keyframe_batch enqueues (1) */
int myslam_backend_insert_launches_per_call(const myslam_backend* h);

/* ------------------------------------------------------------------------------------------
 * The whole map of every stream on the device — Map::mmAllKeyFrames / mmAllMapPoints (src/map.cpp: InsertKeyFrame, InsertMapPoint, RemoveMapPoint,
 * AddOutlierMapPoint, RemoveAllOutlierMapPoints) and the link fields KeyFrame::mpLastKF / mRelativePoseToLastKF (include/myslam/keyframe.h, set in
 * src/frontend.cpp:424-447), kept up to date from the back end's ACTIVE tables after every insert and optimise and laid out so that they ARE the
 * tables of myslam_loop_correct_batch: the fixed set of src/loopclosing.cpp:560-562, the edges of :568-602 and the map points of :612-641.
 * Order of one key-frame:  insert -> update(AFTER_INSERT) -> optimise -> update(AFTER_OPTIMIZE) -> ... -> detect / match / verify -> loop_inputs ->
 * myslam_loop_correct_batch on the archive's own tables -> write_backend -> myslam_tracker_update_from_map_batch.
 * The handle owns every buffer and nothing moves after create, so a recorded step that names the tables stays valid.  Item b is one stream's map;
 * tables are strided by the caps, slots from a count on are never read or written (myslam_map_view gives the device pointers):
 *   kf_id        max_batch x kf_cap i64, ascending, append-only      mnKFId of every key-frame; row 0 is the stream's first key-frame
 *   kf_pose      max_batch x kf_cap x 7 f64                          Tcw: myslam_loop_correct_batch's d_poses;   n_kf  max_batch i32
 *   edge_v0 / edge_v1 / meas / n_edges   i32, i32, f64 x 7, i32      myslam_loop_correct_batch's d_edge_*, which appends its loop edge here in place
 *   mp_id        max_batch x point_cap i64, ascending, append-only   mnId of every map point
 *   mp_pos       max_batch x point_cap x 3 f64                       d_points, and myslam_loop_match_batch's d_landmark_pos with landmark_stride = point_cap
 *   mp_first_kf  max_batch x point_cap i32                           row in kf_id of GetObservations().front()->mpKF, -1 = never seen with an observer
 *   mp_state     max_batch x point_cap u8                            0 alive; 1 on the map's outlier list (AddOutlierMapPoint) but not yet erased; 2 erased
 *   n_mp         max_batch i32
 * and, internal, the SNAPSHOT: per item the archive slot of every row of the back end's map-point table as of the last update, with its count; and the
 * WINDOW RECORD that keeps mp_first_kf exact (a back-end row with d_obs_kf = -1 no longer says whose it is): win_kf = the archive row of every row of the
 * back end's key-frame table at the last update (up to MYSLAM_BA_MAX_WINDOW_POSES), mp_win_mask (u16 per point) = bit k: the point had a row on row k
 * of that table, mp_gone_kf (i32 per point) = the lowest archive row among the point's observers that have left the window, -1 = none.
 * CONTRACT: exactly one back-end call on an item lies between two updates of it.  myslam_backend_optimize_batch's d_mp_report is indexed by INPUT row,
 * and after its compaction only the snapshot says which point that row was.
 *
 * myslam_map_load / myslam_map_get — host pointers, synchronous (they wait for the handle's stream; MYSLAM_ERR_UNSUPPORTED while it is recorded): one
 * item from / to the host, for streams that move over from a host map and for hand-made states.  load validates: ids strictly ascending, counts
 * within the caps (MYSLAM_ERR_CAPACITY beyond), edge endpoints in [0, n_kf) and distinct, mp_first_kf and mp_gone_kf in [-1, n_kf), states in {0, 1, 2},
 * snapshot entries in [0, n_mp), win_kf entries in [0, n_kf), no mask bit from n_win on — else MYSLAM_ERR_INVALID and the item keeps every byte.
 * snapshot / win_kf may be NULL with a count of 0; mp_gone_kf NULL = all -1, mp_win_mask NULL = all 0 (a map whose window is empty).  get: arrays sized
 * by the caps (snapshot: backend_mp_cap, win_kf: MYSLAM_BA_MAX_WINDOW_POSES), any pointer may be NULL.
 *
 * myslam_map_update_batch — device pointers, ONE launch (k_map_update, one workgroup per item), after EACH back-end call on the same stream.  It reads
 * the back end's tables as they stand after that call (be_kf_cap / be_mp_cap / be_obs_cap = that handle's caps; be_mp_cap must be the archive's
 * backend_mp_cap), d_backend_status = that call's d_status, and
 *   mode MYSLAM_MAP_AFTER_INSERT:   d_outlier_mp_id (batch x outlier_cap) / d_n_outlier_mp of the turn or init, NULL count = none;
 *   mode MYSLAM_MAP_AFTER_OPTIMIZE: d_mp_report of myslam_backend_optimize_batch.
 * Per item everything is decided before anything is written.  After insert:
 *   1. d_backend_status[b] != 0: the item is untouched, MYSLAM_MAP_SKIPPED.
 *   2. every back-end key-frame id above the archive's last is appended with its pose, in order (Map::InsertKeyFrame); every appended row except the
 *      archive's first gets the edge (new row, previous row, meas), meas = p7_of(mm(T_of(new), T_inv(T_of(prev)))) with prev = the archive's pose of
 *      the previous row: mRelativePoseToLastKF as T[v0] * T[v1]^-1, in chain.py's arithmetic and operation order, every f64 operation rounded alone.
 *   3. every back-end map-point id that is not in the archive is appended (Map::InsertMapPoint) with state 0; it must be above the archive's last id,
 *      otherwise MYSLAM_ERR_INVALID.  An id that is archived (a point that comes back) is just found.
 *   4. every listed outlier id that is archived with state 0 gets state 1 (Map::AddOutlierMapPoint); other ids are ignored.
 *   5. refresh: every back-end key-frame row's pose and map-point row's position goes to its archive row.  First observers: a key-frame row of the
 *      window record that is no longer in the table has left the window; every point of the OLD snapshot whose mask names it lowers its mp_gone_kf to
 *      that row.  Both observation lists are in key-frame order (src/keyframe.cpp:45, src/map.cpp:38), so GetObservations().front()->mpKF is the
 *      lowest archive row among the point's rows with d_obs_kf >= 0 (the first of them) and mp_gone_kf: a point of the table takes that minimum, a
 *      point that left the table takes mp_gone_kf (all its rows are of key-frames that left; such rows are never ACTIVE, the optimiser cannot remove
 *      them).  "The record stays when the front row has d_obs_kf < 0" alone is NOT exact: when the optimiser removes a front observation whose
 *      key-frame is in the window and the next row is one of a key-frame that left, the front becomes that key-frame (tests/test_map_archive_ref.py
 *      holds such a point).  Rows LoopLocalFusion appended out of key-frame order are out of scope, below.
 *   6. the snapshot, the masks and the window record are rebuilt from the table.  MYSLAM_MAP_UPDATED.
 * After optimise: MYSLAM_BACKEND_DONE -> every snapshot row whose d_mp_report is 2 gets state 2, then every archive point with state 1 gets state 2
 * (Map::RemoveAllOutlierMapPoints empties the whole list, points that are not active included), then 5 and 6.  A snapshot row whose d_mp_report is 1
 * (the point left the active set alive) takes the solve's position if the solve is attached: myslam_map_attach_solve, below.  MYSLAM_BACKEND_EMPTY or an error: the
 * reference returns before the removal — nothing changes, state 1 stays, MYSLAM_MAP_SKIPPED.  A table that holds an id the archive lacks, or more rows
 * than the snapshot: MYSLAM_ERR_INVALID.
 * A key-frame, edge or point count that would exceed its cap: MYSLAM_ERR_CAPACITY.  A count out of range, a key-frame id at or below the archive's
 * last that it does not hold: MYSLAM_ERR_INVALID.  An item with an error keeps every byte.
 *
 * myslam_map_loop_inputs_batch — one launch: myslam_loop_correct_batch's per-loop index inputs.  d_active (batch x active_cap, active_cap >= be_kf_cap)
 * / d_n_active = archive rows of the back end's key-frame ids in table order (ascending by construction; :560); d_cur = row of d_cur_kf_id[b] (i64,
 * the turn's d_new_kf_id); d_loop = row of d_loop_kf_id[b] (u64, the scan's d_best_id), -1 when absent or d_detect_status[b] !=
 * MYSLAM_LOOP_DETECT_CANDIDATE; d_first_active (batch x point_cap): for a point in the back end's table the d_obs_kf of its first ACTIVE row
 * (GetActiveObservations().front(); the active list is the table's order), else -1; d_first_kf: mp_first_kf for states 0 and 1, -1 for state 2 (:625-629);
 * d_n_points = n_mp.  d_cur_kf_id[b] < 0: d_cur = d_loop = -1 and empty lists; the corrector skips the item on its verify status.
 *
 * myslam_map_write_backend_batch — one launch, after myslam_loop_correct_batch ran on the archive's tables: for items with d_select[b] != 0 (NULL = all)
 * every back-end key-frame row takes its archive pose and every map-point row its archive position, found by id (:612-641 reach the active map through
 * the shared objects).  For an item the corrector skipped this is a copy of equal bits.
 *
 * myslam_map_feature_slots_batch — one launch: d_feat_mp_id (batch x feat_cap) / d_n_feat of the turn -> the archive slot per feature (binary search),
 * -1 for no id, an absent id or a point with state 2: myslam_loop_store_put_batch's d_feat_landmark.
 *
 * All batch calls allocate nothing, never synchronise, read no device memory from the host, are recordable between myslam_graph_begin / _end and use no
 * global atomics; an item's bytes depend neither on its slot nor on its neighbours.  Call level, nothing enqueued: NULL pointers, an unknown mode, a
 * back-end cap that does not match (be_kf_cap beyond MYSLAM_BA_MAX_WINDOW_POSES included) -> MYSLAM_ERR_INVALID; batch beyond the handle's -> MYSLAM_ERR_CAPACITY.
 * OUT OF SCOPE for the modes above: LoopLocalFusion's re-linking of observations (src/loopclosing.cpp:509-532) is not done by an insert's or an optimise's
 * update; it is RE-LINK's, below, on the device: the plan, the moved rows in the back end's tables and in the observation archive, the erased states
 * (myslam_map_relink_batch) and mode MYSLAM_MAP_AFTER_RELINK of myslam_map_update_batch, which is an insert's update without an outlier list (the
 * re-link makes neither a key-frame nor a point): refresh, snapshot, masks and window record follow the re-linked table.  mp_first_kf is NOT exact for
 * a point a re-link has touched (its list is no longer in key-frame order): a stream that re-links passes myslam_relink_first_kf_batch's array to
 * myslam_loop_correct_batch instead of myslam_map_loop_inputs_batch's d_first_kf.  Culled and erased links: LINK UPKEEP, below; whole tables from
 * a host map: myslam_loop_store_set_landmarks_batch.
 * ------------------------------------------------------------------------------------------ */
#define MYSLAM_MAP_AFTER_INSERT 0
#define MYSLAM_MAP_AFTER_OPTIMIZE 1
#define MYSLAM_MAP_AFTER_RELINK 2     /* RE-LINK, below */
#define MYSLAM_MAP_UPDATED 0
#define MYSLAM_MAP_SKIPPED 1
typedef struct myslam_map myslam_map;
typedef struct myslam_map_tables {
    int64_t* kf_id; double* kf_pose; int32_t* n_kf;
    int32_t* edge_v0; int32_t* edge_v1; double* meas; int32_t* n_edges;
    int64_t* mp_id; double* mp_pos; int32_t* mp_first_kf; uint8_t* mp_state; int32_t* n_mp;
    int32_t max_batch, kf_cap, edge_cap, point_cap, backend_mp_cap;
} myslam_map_tables;
int myslam_map_create(myslam_map** out, int max_batch, int kf_cap, int edge_cap, int point_cap, int backend_mp_cap);
int myslam_map_destroy(myslam_map* h);
int myslam_map_set_stream(myslam_map* h, void* hip_stream);
/* the device pointers and caps of the per-item tables: valid until destroy */
int myslam_map_view(const myslam_map* h, myslam_map_tables* out);
int myslam_map_load(myslam_map* h, int item, const int64_t* kf_id, const double* kf_pose, int n_kf, const int32_t* edge_v0, const int32_t* edge_v1,
                    const double* meas, int n_edges, const int64_t* mp_id, const double* mp_pos, const int32_t* mp_first_kf, const uint8_t* mp_state, int n_mp,
                    const int32_t* snapshot, int n_snapshot, const int32_t* mp_gone_kf, const uint16_t* mp_win_mask, const int32_t* win_kf, int n_win);
int myslam_map_get(myslam_map* h, int item, int64_t* kf_id, double* kf_pose, int* n_kf, int32_t* edge_v0, int32_t* edge_v1, double* meas, int* n_edges,
                   int64_t* mp_id, double* mp_pos, int32_t* mp_first_kf, uint8_t* mp_state, int* n_mp, int32_t* snapshot, int* n_snapshot,
                   int32_t* mp_gone_kf, uint16_t* mp_win_mask, int32_t* win_kf, int* n_win);
/* src/map.cpp InsertKeyFrame / InsertMapPoint / AddOutlierMapPoint / RemoveAllOutlierMapPoints and src/frontend.cpp:424-447 as described above */
int myslam_map_update_batch(myslam_map* h, int mode, const int64_t* d_kf_id, const double* d_kf_pose, const int32_t* d_n_kf, int be_kf_cap,
                            const int64_t* d_mp_id, const double* d_mp_pos, const int32_t* d_n_mp, int be_mp_cap, const int32_t* d_obs_mp,
                            const int32_t* d_obs_kf, const uint8_t* d_obs_flags, const int32_t* d_n_obs, int be_obs_cap, const int32_t* d_backend_status,
                            const int64_t* d_outlier_mp_id, const int32_t* d_n_outlier_mp, int outlier_cap, const uint8_t* d_mp_report, int batch,
                            int32_t* d_status);
/* kernel launches one myslam_map_update_batch enqueues (1) */
int myslam_map_launches_per_update(const myslam_map* h);
/* The optimised position of a map point that LEAVES the active set with the optimise.  Backend::OptimizeActiveMap sets the position of every vertex
 * (src/backend.cpp:259-261) before Map::RemoveOldActiveMapPoints (src/map.cpp:126-140) takes the points without an active observation out of the active
 * set, so Map::mmAllMapPoints holds the optimised position of such a point; the back end's compacted table no longer has its row.  With the two
 * pointers of myslam_backend_solve_view (of the back end whose tables the updates read; its mp_cap is the archive's backend_mp_cap) attached, an
 * update after optimise gives every snapshot row whose d_mp_report is 1 and that had a vertex the solve's position.  Without them (the state after
 * create; both NULL detaches) such a point keeps the position it had before the optimise.  One NULL and one not: MYSLAM_ERR_INVALID.  It concerns
 * a landmark that is not fixed and loses its last active observation to the optimiser while older rows remain; tests/test_whole_map_model.py holds
 * the shortest such history. */
int myslam_map_attach_solve(myslam_map* h, const double* d_solve_points, const int32_t* d_solve_mp_slot);
/* src/loopclosing.cpp:560-562 and the index inputs of :470-507 / :612-641 as described above */
int myslam_map_loop_inputs_batch(myslam_map* h, const int64_t* d_kf_id, const int32_t* d_n_kf, int be_kf_cap, const int64_t* d_mp_id, const int32_t* d_n_mp,
                                 int be_mp_cap, const int32_t* d_obs_mp, const int32_t* d_obs_kf, const uint8_t* d_obs_flags, const int32_t* d_n_obs,
                                 int be_obs_cap, const int64_t* d_cur_kf_id, const uint64_t* d_loop_kf_id, const int32_t* d_detect_status, int active_cap,
                                 int batch, int32_t* d_active, int32_t* d_n_active, int32_t* d_cur, int32_t* d_loop, int32_t* d_first_active,
                                 int32_t* d_first_kf, int32_t* d_n_points);
int myslam_map_write_backend_batch(myslam_map* h, const int64_t* d_kf_id, double* d_kf_pose, const int32_t* d_n_kf, int be_kf_cap, const int64_t* d_mp_id,
                                   double* d_mp_pos, const int32_t* d_n_mp, int be_mp_cap, const uint8_t* d_select, int batch);
int myslam_map_feature_slots_batch(myslam_map* h, const int64_t* d_feat_mp_id, const int32_t* d_n_feat, int feat_cap, int batch, int32_t* d_feat_landmark);

/* ------------------------------------------------------------------------------------------
 * LINK UPKEEP — a key-frame feature's mpMapPoint.lock() that goes null after the key-frame was made, on the device.  Two things do that:
 *   CULLED  Backend::OptimizeActiveMap removes an outlier edge and resets the feature's map point (src/backend.cpp:236-247).  KeyFrame shares its
 *           Feature objects with its Frame (src/keyframe.cpp:21): the next TrackLastFrame (src/frontend.cpp:127-171) sees the reset when the last
 *           frame is that key-frame's frame, and ComputeCorrectPose (src/loopclosing.cpp:218-237) sees it when the key-frame is a loop key-frame.
 *   ERASED  Map::RemoveAllOutlierMapPoints (src/map.cpp:166-175) drops the map's only shared_ptr: every feature that pointed at the point locks null.
 * Order of one key-frame:  ... optimise -> update(AFTER_OPTIMIZE) -> culled_view's lists -> myslam_loop_store_clear_links_batch (pending = the turn's
 * feature-slot table, which is put afterwards: the AddToDatabase order, src/loopclosing.cpp:73-75) + myslam_tracker_clear_links_batch -> put -> ...
 * -> detect -> myslam_map_filter_landmarks_batch on d_loop_feat_landmark -> match.  Filtering erased points at use is exact: an erased id never
 * returns, and ComputeCorrectPose asks lock() at that same moment.  Erased points need no tracker rule: the frontend resets the feature that made
 * it list a point (src/frontend.cpp:267).
 * Each of the three batch calls is ONE launch, one workgroup per item, on its handle's stream; nothing is allocated or synchronised, no device memory
 * is read from the host, no global atomics; an item's bytes depend neither on its slot nor on its neighbours; all are recordable between
 * myslam_graph_begin / _end (myslam_loop_store_clear_links_batch too: unlike put_batch it does no host bookkeeping, and it reads the ids and the
 * number of key-frames held on the device, so a replay sees what was put after the recording).
 *
 * myslam_backend_culled_view — the device pointers of the list k_backend_write_back writes with every myslam_backend_optimize_batch (still three
 * launches), valid until destroy, stride obs_cap:  d_kf_id (max_batch x obs_cap i64) = d_kf_id[b][d_obs_kf[row]] and d_tag (i32) = d_obs_tag[row] of
 * every INPUT row with d_obs_report == 1, in input row order (a removed edge row is ACTIVE, so d_obs_kf >= 0; the turn and the init write the
 * feature's index into d_feat_tag);  d_n_culled (max_batch i32) their number = d_n_outlier_edges.  A refused or EMPTY item: 0.  Items from the call's
 * batch on keep their bytes; entries from the count on are unspecified; before the first call every count is 0.
 *
 * myslam_loop_store_clear_links_batch — item b's list at d_kf_id / d_tag + b * list_cap, d_n[b] entries (clamped to [0, list_cap]).  An entry with
 * id >= 0 and tag >= 0:  the pending pointers are given, id == d_pending_kf_id[b] and tag < feat_cap -> d_pending_feat_landmark[b][tag] = -1;
 * otherwise the id is searched among the ids held: found and tag < that slot's stored feature count -> that entry of the slot's table = -1.  Anything
 * else (an id not held — key-frames that closed a loop and the five after it are never stored, src/loopclosing.cpp:671-681 —, a negative id, a
 * tag out of range) is ignored.  d_n_cleared[b] (may be NULL) = the entries that named a stored or pending feature: entries, not distinct features
 * (the writes are idempotent).  Call level, nothing enqueued: a required pointer NULL, exactly one pending pointer NULL, list_cap <= 0 or
 * batch <= 0 -> MYSLAM_ERR_INVALID; batch > 65535 -> MYSLAM_ERR_CAPACITY.
 *
 * myslam_map_filter_landmarks_batch — the whole row of d_feat_landmark (batch x feat_cap; the matcher indexes it by class_id without a count): an
 * entry e with 0 <= e < n_mp[b] and mp_state[b][e] == 2 becomes -1; every other value (-1 and out-of-range values included, which the matcher
 * reports itself) keeps its bits.  d_n_dropped[b] (may be NULL) = the entries changed.  NULL table or feat_cap <= 0 -> MYSLAM_ERR_INVALID; batch
 * beyond the handle's -> MYSLAM_ERR_CAPACITY.
 *
 * myslam_tracker_clear_links_batch — item s = stream s, lists strided by list_cap.  A stream is touched only when its ids are valid and
 * ref_frame_id == next_frame_id - 1 (the last frame is the reference key-frame's frame; frozen or not): every entry with d_kf_id == ref_kf_id and
 * 0 <= tag < n_feat sets that feature's landmark slot to -1.  The landmark table, ids, outlier list and everything else keep their bytes (the next
 * turn's rebuild drops landmarks nothing names).  Any other stream keeps every byte and reports 0 in d_n_cleared (S, may be NULL).
 * ------------------------------------------------------------------------------------------ */
/* src/backend.cpp:236-247: the features whose edge the solve removed */
int myslam_backend_culled_view(const myslam_backend* h, const int64_t** d_kf_id, const int32_t** d_tag, const int32_t** d_n_culled);
/* src/backend.cpp:236-247 as ComputeCorrectPose (src/loopclosing.cpp:218-237) sees it in a stored key-frame */
int myslam_loop_store_clear_links_batch(myslam_loop_store* h, const int64_t* d_kf_id, const int32_t* d_tag, const int32_t* d_n, int list_cap, int batch,
                                        const int64_t* d_pending_kf_id, int32_t* d_pending_feat_landmark, int32_t* d_n_cleared);
/* src/map.cpp:166-175 as src/loopclosing.cpp:218-237 sees it */
int myslam_map_filter_landmarks_batch(myslam_map* h, int32_t* d_feat_landmark, int feat_cap, int batch, int32_t* d_n_dropped);
/* src/backend.cpp:236-247 as TrackLastFrame (src/frontend.cpp:127-171) sees it through src/keyframe.cpp:21 */
int myslam_tracker_clear_links_batch(myslam_tracker* h, const int64_t* d_kf_id, const int32_t* d_tag, const int32_t* d_n, int list_cap,
                                     int32_t* d_n_cleared);

/* ------------------------------------------------------------------------------------------
 * OBSERVATION ARCHIVE — MapPoint::GetObservations() (src/mappoint.cpp:19-44) of every map point that is alive and NOT in the active set, per stream,
 * on the device.  The reference keeps that list in the MapPoint object for as long as the point lives; a point that Map::RemoveOldActiveMapPoints
 * (src/map.cpp:126-140) took out of the active set and that a feature of a later key-frame names again comes back with it, and since its front
 * observer is outside the window, src/backend.cpp:175-177 makes it a FIXED landmark.  The back end's tables hold a point's rows only while it is
 * active and myslam_map holds no rows at all: this handle is the source of the prior rows of myslam_backend_insert_keyframe_batch (d_prior_*,
 * d_n_prior).  The tracker keeps such a point by design (myslam_tracker_update_from_map_batch: absent ids keep their values) and the next turn names
 * it in d_feat_mp_id.
 * Order of one key-frame, all on one stream:  turn -> prior_rows -> insert (with those arrays) -> myslam_map_update_batch(AFTER_INSERT) ->
 * update(AFTER_INSERT) -> optimise -> myslam_map_update_batch(AFTER_OPTIMIZE) -> update(AFTER_OPTIMIZE, the optimise's d_obs_report) -> ...
 * CONTRACT, the map archive's: exactly one back-end call on an item lies between two updates of it, and the map's update of that call comes first.
 *
 * create: `map` is the map archive of the same streams (its tables are read through myslam_map_view; it must outlive this handle; max_batch at most
 * its own; the back end's mp_cap is its backend_mp_cap), be_obs_cap the back end's obs_cap, row_cap the stored rows one item can hold.  The handle
 * owns, per item: two POOLS of row_cap rows, one of which holds the segments; per map-point slot of `map` (offset, count); the MIRROR, two copies of
 * be_obs_cap rows with the ids and segment starts of the table's map points; and the counters.  Nothing moves after create.
 * A stored row is (observer's mnKFId i64, uv 2 x f32, tag i32, flags u8): uv and tag bit for bit what the back end's table held, flags only
 * MYSLAM_BACKEND_OBS_OUTLIER as the table held it (ACTIVE is never stored), a point's rows in its GetObservations() order = the table's order
 * within the segment.
 *
 * myslam_obs_archive_update_batch — device pointers, ONE launch (k_obs_update, one workgroup per item), after EACH myslam_map_update_batch.  It reads
 * the back end's thirteen tables as they stand after the call in myslam_backend_optimize_batch's order (d_kf_pose, d_mp_pos and d_mp_outlier are not
 * read and may be NULL) with that handle's three caps, d_backend_status = the back-end call's d_status, d_map_status = the map update's d_status, and
 * after an optimise its d_obs_report (by INPUT row: the row of the table as it stood at the previous update).  Per item everything is decided
 * before anything is written:
 *   1. d_backend_status[b] != 0 or d_map_status[b] == MYSLAM_MAP_SKIPPED: MYSLAM_MAP_SKIPPED, every byte kept.
 *   2. a point that was in the table at the previous update, is not in it now and has mp_state != 2 in the map LEAVES ALIVE: its rows are stored,
 *      after an insert all the rows it had, after an optimise those whose d_obs_report is not 1.
 *   3. a table row with d_obs_kf = -1 no longer says whose it is, and the compacted table no longer holds a leaving point's rows at all, so the
 *      mirror holds every row of the table whole, with the observer's mnKFId, and follows the rows through both compactions: at an insert a point's
 *      old rows stay in order at the front of its segment and the new key-frame's (the highest id's) rows follow; at an optimise the kept rows keep
 *      their order.  A point NEW to the table has its prior rows first: the number of its leading rows that are not the new key-frame's must equal
 *      the number of rows stored for it (0 for a point that is not stored or erased), and their ids come from the store.  If the number differs the
 *      caller did not pass this handle's rows: MYSLAM_ERR_INVALID.
 *   4. a point that is in the table now has no stored rows any more (it RETURNED); when it leaves again it is stored afresh.
 *   5. a point erased while outside the table (Map::RemoveAllOutlierMapPoints empties the whole list, src/map.cpp:166-175) has dead rows: mp_state
 *      is read at use, nothing runs at the erasure.
 *   6. dead rows are reclaimed: segments are bump-allocated; when the rows in use plus the rows to store exceed row_cap, the live segments go to the
 *      other pool in slot order first, in the same launch.  MYSLAM_ERR_CAPACITY comes when, and only when, the rows of the points alive and outside
 *      the table exceed row_cap.
 *   7. errors are STICKY: a map update that answered an error (the table moved on without this item), rule 3's mismatch, a table that does not
 *      continue the mirror or a count out of range (MYSLAM_ERR_INVALID) and rule 6's MYSLAM_ERR_CAPACITY.  The item keeps every byte, and every
 *      later update and prior_rows of it reports the same error (d_n_prior[b] = 0) until a load.
 *   otherwise MYSLAM_MAP_UPDATED.
 *
 * myslam_obs_archive_prior_rows_batch — ONE launch (k_obs_prior_rows), before the insert: d_feat_mp_id / d_n_feat (batch x feat_cap) of the turn and
 * the back end's d_mp_id / d_n_mp as they stand -> the insert's prior arrays (batch x prior_cap) and d_n_prior.  A row-set is written for every
 * DISTINCT id >= 0 among the item's features that is not in the table and that the map holds with state 0 or 1 (a listed point is still alive) and
 * that has stored rows; ids ascend and a point's rows are in stored order (what the insert demands of d_prior_mp_id).  Ids the map does not hold,
 * erased ids and ids in the table give no rows.  More rows than prior_cap: MYSLAM_ERR_CAPACITY for that item and d_n_prior[b] = 0, nothing is
 * truncated, not sticky; a count out of range: MYSLAM_ERR_INVALID, likewise.  Output slots from the count on keep their bytes.  d_status MYSLAM_OK else.
 *
 * myslam_obs_archive_load / _get — one item, host pointers, synchronous as myslam_map_load / _get (MYSLAM_ERR_UNSUPPORTED while the stream is
 * recorded); both read the map's ids and states of the item.  load takes the live segments (ids strictly ascending, each held by the map with
 * state 0 or 1 and not in the table, counts >= 1 summing to n_rows) with their rows, and the mirror: the ids of the back end's current table
 * (strictly ascending), the rows of each, and for every row of that table the observer's mnKFId with uv, tag and flags; flags with a bit other than
 * OUTLIER, or anything else above -> MYSLAM_ERR_INVALID, counts beyond the caps -> MYSLAM_ERR_CAPACITY, the item then keeps every byte.  It clears
 * the sticky error and the reclaim count.  get: the live segments concatenated in ascending id order with per-point counts (dead rows are never
 * visible; seg and row arrays sized row_cap), the mirror (sized mp_cap / obs_cap), the rows in use in the pool, the reclaims so far and the sticky
 * error; any pointer may be NULL.
 *
 * Both batch calls allocate nothing, never synchronise, read no device memory from the host, use no global atomics and are recordable between
 * myslam_graph_begin / _end; an item's bytes depend neither on its slot nor on its neighbours.  Call level, nothing enqueued: NULL required
 * pointers, an unknown mode, d_obs_report missing AFTER_OPTIMIZE, caps that do not match the handle or the map -> MYSLAM_ERR_INVALID; a batch beyond
 * the handle's -> MYSLAM_ERR_CAPACITY.
 * OUT OF SCOPE for the two calls above: the rows that LoopLocalFusion's re-linking moves (src/loopclosing.cpp:509-532; :521-525 appends a point's
 * observations to a point that is usually not active, so this store is where they are appended).  RE-LINK, below, does it on this handle:
 * myslam_relink_stage_batch reads the lists, myslam_relink_obs_update_batch is this handle's update after a re-link (myslam_obs_archive_update_batch
 * keeps its two modes), myslam_relink_first_kf_batch gives the front observers in list order.
 * ------------------------------------------------------------------------------------------ */
typedef struct myslam_obs_archive myslam_obs_archive;
int myslam_obs_archive_create(myslam_obs_archive** out, const myslam_map* map, int max_batch, int be_obs_cap, int row_cap);
int myslam_obs_archive_destroy(myslam_obs_archive* h);
int myslam_obs_archive_set_stream(myslam_obs_archive* h, void* hip_stream);
int myslam_obs_archive_load(myslam_obs_archive* h, int item, const int64_t* seg_mp_id, const int32_t* seg_count, int n_seg, const int64_t* row_kf_id,
                            const float* row_uv, const int32_t* row_tag, const uint8_t* row_flags, int n_rows, const int64_t* table_mp_id,
                            const int32_t* table_mp_rows, int n_table_mp, const int64_t* table_kf_id, const float* table_uv, const int32_t* table_tag,
                            const uint8_t* table_flags, int n_table_rows);
int myslam_obs_archive_get(myslam_obs_archive* h, int item, int64_t* seg_mp_id, int32_t* seg_count, int* n_seg, int64_t* row_kf_id, float* row_uv,
                           int32_t* row_tag, uint8_t* row_flags, int* n_rows, int64_t* table_mp_id, int32_t* table_mp_rows, int* n_table_mp,
                           int64_t* table_kf_id, float* table_uv, int32_t* table_tag, uint8_t* table_flags, int* n_table_rows, int* rows_in_use,
                           int* n_reclaims, int* error);
/* src/map.cpp:126-140 and src/mappoint.cpp:19-56 as the stored lists see them, as described above */
int myslam_obs_archive_update_batch(myslam_obs_archive* h, int mode, const int64_t* d_kf_id, const double* d_kf_pose, const int32_t* d_n_kf,
                                    const int64_t* d_mp_id, const double* d_mp_pos, const uint8_t* d_mp_outlier, const int32_t* d_n_mp,
                                    const int32_t* d_obs_mp, const int32_t* d_obs_kf, const uint8_t* d_obs_flags, const float* d_obs_uv,
                                    const int32_t* d_obs_tag, const int32_t* d_n_obs, int be_kf_cap, int be_mp_cap, int be_obs_cap,
                                    const int32_t* d_backend_status, const int32_t* d_map_status, const uint8_t* d_obs_report, int batch, int32_t* d_status);
/* kernel launches one myslam_obs_archive_update_batch enqueues (1) */
int myslam_obs_archive_launches_per_update(const myslam_obs_archive* h);
/* GetObservations() of the returning map points (src/keyframe.cpp:39-47 finds them in the objects the features hold) */
int myslam_obs_archive_prior_rows_batch(myslam_obs_archive* h, const int64_t* d_feat_mp_id, const int32_t* d_n_feat, int feat_cap, const int64_t* d_mp_id,
                                        const int32_t* d_n_mp, int be_mp_cap, int batch, int64_t* d_prior_mp_id, int64_t* d_prior_kf_id, float* d_prior_uv,
                                        int32_t* d_prior_tag, uint8_t* d_prior_flags, int32_t* d_n_prior, int prior_cap, int32_t* d_status);

/* ------------------------------------------------------------------------------------------
 * RE-LINK — the second half of LoopClosing::LoopLocalFusion (src/loopclosing.cpp:509-532) on the device: for every surviving feature match the
 * current key-frame's map point is merged into the loop key-frame's (:521-525 move its observations and point their features at the loop point,
 * :527 erases it with Map::RemoveMapPoint, src/map.cpp:144-155), and a feature without a point adopts the loop point (:529).  What this section
 * does on the device: the PLAN of the walk (which point goes where), the moved ROWS (the back end's thirteen tables, the observation archive's
 * segments and mirror), the erased states and the snapshot in the map archive, the front observers in list order, the features of EVERY key-frame that
 * observed a merged point (loop store) and the tracker's landmarks.  A device-resident stream needs no host map for it.
 * Order of one loop:  ... -> verify -> loop_inputs -> myslam_loop_correct_batch -> write_backend -> myslam_loop_relink_plan_batch ->
 * myslam_relink_stage_batch -> myslam_relink_backend_batch -> myslam_map_relink_batch -> myslam_map_update_batch(MYSLAM_MAP_AFTER_RELINK) ->
 * myslam_relink_obs_update_batch -> myslam_loop_store_set_links_batch (the moved rows' list, then the plan's) + myslam_tracker_relink_batch ->
 * myslam_tracker_update_from_map_batch -> the next key-frame's prior_rows / insert; myslam_relink_first_kf_batch before the next myslam_loop_correct_batch.
 * The re-link counts as the ONE back-end call between two updates.
 * Every batch call is ONE launch, one workgroup per item, on its handle's stream: device pointers, nothing allocated or synchronised, no device
 * memory read from the host, no global atomics, recordable between myslam_graph_begin / _end.  Per item everything is decided before anything is
 * written: an item with an error keeps every byte of every table (the plan's own lists of it are empty); an item's bytes depend neither on its
 * slot nor on its neighbours.
 *
 * myslam_relink_create — `map` is the map archive of the same streams (read through myslam_map_view for mp_state / n_mp; it must outlive this
 * handle; max_batch at most its own), out_cap the matcher's and verifier's cap (<= 4096), feat_cap the stride of the feature tables (<= 65536);
 * beyond those limits MYSLAM_ERR_CAPACITY.  The handle owns the lists of myslam_relink_view; nothing moves after create.
 *
 * myslam_loop_relink_plan_batch — per item: d_valid_pairs (batch x out_cap x 2: current feature, loop feature) and d_counts of
 * myslam_loop_match_batch, d_outlier (batch x out_cap) of myslam_loop_verify_batch, d_correct_status = myslam_loop_correct_batch's d_status,
 * d_cur_feat_landmark (batch x feat_cap, IN/OUT) the current key-frame's feature -> archive-slot table as myslam_map_feature_slots_batch wrote it with
 * link upkeep applied, d_loop_feat_landmark (batch x feat_cap) after myslam_map_filter_landmarks_batch, d_cur_kf_id (batch i64) the current
 * key-frame's mnKFId.  A status that is neither MYSLAM_LOOP_CORRECT_DONE nor MYSLAM_LOOP_CORRECT_FUSED_ONLY: MYSLAM_RELINK_SKIPPED, the lists are
 * empty (the reference returns at :438-442 before LoopLocalFusion).  Otherwise the pairs with d_outlier == 0 are walked serially, in their order
 * (_msetValidFeatureMatches after :423-428).  lock() of a slot is null for a slot < 0 or a point in state 2; states 0 and 1 are alive.
 *   loop_mp = lock(d_loop_feat_landmark[lf]), followed through the merges this walk has made (the loop feature is an observation of its point and
 *             moved with it); null: the pair is skipped (:514-517; a slot >= 0 in state 2 is counted as a dead loop point).
 *   cur_mp  = lock(the current table's entry for cf) AS THE WALK HAS LEFT IT: an observation follows the merges of its point ((c, l1) then (c, l2)
 *             merges L1 into L2); an adopted feature is no observation (:529 sets the pointer only), so when the point it adopted is merged
 *             away later its entry is null again.
 *   cur_mp null: ADOPT, the entry for cf becomes loop_mp.  cur_mp == loop_mp: skipped — a DECLARED DEVIATION (the reference would append a
 *   point's observations to itself and erase it; chain.py and host/myslam_system.hpp skip as well).  Otherwise MERGE cur_mp -> loop_mp.
 * After the walk every entry of the whole row of d_cur_feat_landmark (as myslam_map_filter_landmarks_batch, without a count) that names a merged
 * point names the point its features ended on; values outside [0, n_mp) keep their bits.  Outputs (myslam_relink_view, valid until destroy):
 *   merge / n_merge    max_batch x out_cap x 2 / max_batch i32   (from slot, to slot) in walk order
 *   adopt / n_adopt    max_batch x out_cap x 2 / max_batch i32   (feature, slot) in walk order
 *   target             max_batch x point_cap i32                 per archive slot below n_mp the slot its features end on (itself for a point
 *                                                                that only received), -1 = untouched
 *   link_kf_id / link_tag / link_slot / n_link   max_batch x feat_cap i64 / i32 / i32, max_batch i32   (d_cur_kf_id, feature, final slot; -1 = its
 *                      point is gone) of every feature of the current key-frame whose entry the walk changed, in feature order: the lists of
 *                      myslam_loop_store_set_links_batch and myslam_tracker_relink_batch
 *   report             max_batch x MYSLAM_RELINK_REPORT_INTS i32: pairs walked, merges, adopts, same-point skips, dead loop points, links
 * Slots from a count on keep their bytes.  MYSLAM_ERR_INVALID per item: d_counts outside [0, out_cap], n_mp outside [0, point_cap], a negative
 * d_cur_kf_id, a feature id of a walked pair outside [0, feat_cap), a slot those pairs name (either table) outside [-1, n_mp) — all found before
 * the first write; the item's lists are then empty and its target row -1.
 * DECLARED DEVIATION, order: the plan runs after the corrector, the reference's loop runs between the fusion and the pose-graph step.  Positions
 * are not touched here, so the only observable difference is a merge target without a single observation, which :623 asserts does not exist.
 *
 * myslam_map_relink_batch — Map::RemoveMapPoint (src/map.cpp:144-155, called at src/loopclosing.cpp:527) for a plan's merge list (d_merge /
 * d_n_merge with stride merge_cap = the plan's out_cap, d_plan_status = the plan's d_status): every from-slot gets state 2 wherever the point
 * was; targets keep their state, positions are not touched.  d_status: MYSLAM_MAP_UPDATED; MYSLAM_MAP_SKIPPED for a plan status other than
 * MYSLAM_RELINK_DONE; MYSLAM_ERR_INVALID (every byte kept) for a count outside [0, merge_cap] or a slot outside [0, n_mp).  d_plan_status is the
 * status of myslam_relink_backend_batch in the order above (0 = MYSLAM_RELINK_DONE: the rows moved), the plan's own where no rows are kept on the device.
 *
 * THE ROWS.  For each merge, in order, the reference appends GetObservations() of the merged point to the END of the target's list, in list order
 * (:521-525; AddObservation alone: the target's active list does not change).  So the final list of a point that stands is its own rows, then for
 * every merge into it, in order, the whole list the merged point had by then, and the OWN rows of every merged point stand at one place of one list.
 * myslam_relink_stage_batch (obs_archive.hip; `oa` is read, nothing of it is written; before the merged points are erased) finds that place with two
 * passes of one lane over the merge list and writes, into the plan's handle (myslam_relink_view, stage_cap rows per item): row_kf_id / row_uv /
 * row_tag / row_flags = the own rows of every merged point, merge by merge, in list order — the mirror's rows for a point of the back end's table (all
 * rows of its segment, with the observer's mnKFId and the OUTLIER bit), the stored segment for a point outside it (a chain merge) —, row_root_id /
 * row_slot = mnId and archive slot of the point the row ends on, row_place = its index in that point's list; per merge merge_from_id, merge_root_id,
 * merge_rows, merge_place.  (row_kf_id, row_tag, row_slot) with n_rows IS the link list of the moved rows for myslam_loop_store_set_links_batch: every
 * moved row once, with its final slot.  d_status: MYSLAM_RELINK_DONE; MYSLAM_RELINK_SKIPPED for a plan status other than DONE; the archive's sticky
 * error; MYSLAM_ERR_INVALID (a slot out of range, an erased point, a target that does not stand, an inconsistent mirror or segment);
 * MYSLAM_ERR_CAPACITY when, and only when, the rows of the points alive and outside the table after the re-link would exceed row_cap, or the table's
 * rows the back end's obs_cap, or the moved rows stage_cap — not sticky, nothing was written.
 * myslam_relink_backend_batch (backend.hip, that handle's copy of the tables): d_stage_status != 0 -> d_status = that value, every byte kept, d_mp_new_row
 * -1.  Else the merged points leave the map-point and observation tables with all their rows; a target in the table gets its rows at the end of its
 * segment, each at row_place: ACTIVE cleared, OUTLIER kept, uv and tag bit for bit, d_obs_kf found by id in the key-frame table, -1 when absent
 * (the rows with ACTIVE = 0 whose key-frame is in the window that myslam_backend_optimize_batch's section announces).  Both tables are compacted in
 * their order, d_obs_mp renumbered, the counts stored; rows from a new count on keep their bytes; d_mp_new_row (batch x mp_cap) by INPUT row, -1 for a
 * point that left.  MYSLAM_ERR_INVALID: the table checks of myslam_backend_optimize_batch, counts that are not the ones the rows were staged for, a
 * place outside what its point receives; MYSLAM_ERR_CAPACITY: more rows than obs_cap.
 * myslam_relink_obs_update_batch (after myslam_map_relink_batch and the map's update): d_backend_status != 0 or a skipped map update -> MYSLAM_MAP_SKIPPED.
 * The mirror follows the table, the appended rows with their observers' ids; a target outside the table has its list written afresh (stored rows,
 * then the moved ones) by update rule 6 (bump allocation, reclaim into the other pool in the same launch); the merged points' segments are dead rows.
 * Errors are STICKY as in myslam_obs_archive_update_batch.  (It uses the plan handle's work_size column as scratch: the handle is not const.)
 * myslam_relink_first_kf_batch: d_first_kf (batch x point_cap) with the meaning of myslam_map_loop_inputs_batch's output, but in LIST order: the archive
 * row of the observer of the first row of the mirror's segment (a point of the table) or of the stored segment, -1 without a row, for an erased point
 * and for an item with a sticky error.  A merged target's list is own rows ++ moved rows, and the moved rows may be of older key-frames: when its
 * front is culled later (src/backend.cpp:236-247) front() is the next row in list order, not the lowest observer.
 * LIMIT, adoptions across loops: whether a feature adopted its point (:529) is known within one walk only.  A feature that adopted a point in an
 * EARLIER loop is treated as an observation of it afterwards: it follows a later merge of that point where the reference's pointer would go null.
 *
 * myslam_loop_store_set_links_batch — myslam_loop_store_clear_links_batch with a value: entry j (d_kf_id, d_tag, d_slot) of item b, with id >= 0,
 * tag >= 0 and slot >= -1, sets that entry of the pending table or of the stored key-frame's table to d_slot, by exactly clear_links' lookup and
 * ignore rules (src/loopclosing.cpp:524, :529 as ComputeCorrectPose, :218-237, sees them in a stored key-frame); d_n_set[b] (may be NULL) = the
 * entries that named a stored or pending feature.  Call level as clear_links.
 *
 * myslam_tracker_relink_batch — item s = stream s = item s of `map`, lists strided by list_cap.  Guard and conditions of
 * myslam_tracker_clear_links_batch: a stream is touched only when its ids are valid and ref_frame_id == next_frame_id - 1, and only by entries
 * with d_kf_id == ref_kf_id and 0 <= tag < n_feat (src/loopclosing.cpp:524, :529 through src/keyframe.cpp:21).  slot -1: the feature loses its
 * landmark.  Otherwise the landmark of feature `tag` takes the target's mnId (map mp_id), its position (mp_pos) and outlier flag = (mp_state == 1);
 * a feature without a landmark gets the slot that already carries the target's id, else a new one at the end of the table.  next_mp_id and the
 * other counters are untouched.  d_status (S): MYSLAM_OK; MYSLAM_ERR_INVALID for a naming entry with a slot outside [-1, n_mp);
 * MYSLAM_ERR_CAPACITY when the landmark table is full — in both cases the stream keeps every byte.  d_n_relinked (S, may be NULL) = naming entries.
 * (The walk runs on the key-frame turn's scratch columns, which a refused stream leaves overwritten; list_cap is the caller's stride, checked against nothing.)
 * ------------------------------------------------------------------------------------------ */
#define MYSLAM_RELINK_DONE 0
#define MYSLAM_RELINK_SKIPPED 1
#define MYSLAM_RELINK_REPORT_INTS 6
typedef struct myslam_relink myslam_relink;
typedef struct myslam_relink_lists {
    int32_t* merge; int32_t* n_merge; int32_t* adopt; int32_t* n_adopt; int32_t* target;
    int64_t* link_kf_id; int32_t* link_tag; int32_t* link_slot; int32_t* n_link; int32_t* report;
    /* the moved rows, written by myslam_relink_stage_batch: max_batch x stage_cap */
    int64_t* row_kf_id; float* row_uv; int32_t* row_tag; uint8_t* row_flags; int64_t* row_root_id; int32_t* row_slot; int32_t* row_place; int32_t* n_rows;
    /* and per merge, max_batch x out_cap: the merged point's id, the id of the point its rows end on, its own rows, their place in that point's list */
    int64_t* merge_from_id; int64_t* merge_root_id; int32_t* merge_rows; int32_t* merge_place; int32_t* n_staged_merges;
    int32_t* table_mp; int32_t* table_rows;   /* max_batch: the back end's counts the rows were staged for */
    int32_t* work_size;                       /* max_batch x point_cap: the stage's scratch */
    int32_t max_batch, out_cap, feat_cap, point_cap, stage_cap;
} myslam_relink_lists;
int myslam_relink_create(myslam_relink** out, const myslam_map* map, int max_batch, int out_cap, int feat_cap, int stage_cap);
int myslam_relink_destroy(myslam_relink* h);
int myslam_relink_set_stream(myslam_relink* h, void* hip_stream);
/* the device pointers and caps of the plan's outputs: valid until destroy */
int myslam_relink_view(const myslam_relink* h, myslam_relink_lists* out);
/* kernel launches one myslam_loop_relink_plan_batch enqueues (1) */
int myslam_relink_launches_per_plan(const myslam_relink* h);
/* src/loopclosing.cpp:509-532: which point is merged into which, which feature adopts, as described above */
int myslam_loop_relink_plan_batch(myslam_relink* h, const int32_t* d_valid_pairs, const int32_t* d_counts, const uint8_t* d_outlier,
                                  const int32_t* d_correct_status, int32_t* d_cur_feat_landmark, const int32_t* d_loop_feat_landmark,
                                  const int64_t* d_cur_kf_id, int batch, int32_t* d_status);
/* src/loopclosing.cpp:521-525: GetObservations() of every merged point, read from the observation archive, staged in the plan's handle */
int myslam_relink_stage_batch(myslam_obs_archive* oa, myslam_relink* h, const int32_t* d_plan_status, int batch, int32_t* d_status);
/* src/loopclosing.cpp:521-527 on the back end's tables: moved rows appended (AddObservation alone), merged points out (src/map.cpp:144-155) */
int myslam_relink_backend_batch(myslam_backend* be, const myslam_relink* h, int64_t* d_kf_id, double* d_kf_pose, int32_t* d_n_kf, int64_t* d_mp_id,
                                double* d_mp_pos, uint8_t* d_mp_outlier, int32_t* d_n_mp, int32_t* d_obs_mp, int32_t* d_obs_kf, uint8_t* d_obs_flags,
                                float* d_obs_uv, int32_t* d_obs_tag, int32_t* d_n_obs, const int32_t* d_stage_status, int batch, int32_t* d_mp_new_row,
                                int32_t* d_status);
/* src/loopclosing.cpp:521-525 as the stored lists see them: the observation archive after the re-link, in the place of myslam_obs_archive_update_batch
 * (which keeps its two modes): after myslam_map_update_batch
 * (MYSLAM_MAP_AFTER_RELINK) of the same call; the tables and caps as there */
int myslam_relink_obs_update_batch(myslam_obs_archive* oa, myslam_relink* h, const int64_t* d_kf_id, const int32_t* d_n_kf, const int64_t* d_mp_id,
                                   const int32_t* d_n_mp, const int32_t* d_obs_mp, const int32_t* d_obs_kf, const uint8_t* d_obs_flags, const float* d_obs_uv,
                                   const int32_t* d_obs_tag, const int32_t* d_n_obs, int be_kf_cap, int be_mp_cap, int be_obs_cap,
                                   const int32_t* d_backend_status, const int32_t* d_map_status, int batch, int32_t* d_status);
/* GetObservations().front()->mpKF of every map point in LIST order (src/loopclosing.cpp:625-629 after :521-525 appended rows out of key-frame order) */
int myslam_relink_first_kf_batch(myslam_obs_archive* oa, int batch, int32_t* d_first_kf);
/* src/loopclosing.cpp:527 with src/map.cpp:144-155: the merged points are erased */
int myslam_map_relink_batch(myslam_map* h, const int32_t* d_merge, const int32_t* d_n_merge, int merge_cap, const int32_t* d_plan_status, int batch,
                            int32_t* d_status);
/* src/loopclosing.cpp:524 and :529 as src/loopclosing.cpp:218-237 sees them in a stored key-frame */
int myslam_loop_store_set_links_batch(myslam_loop_store* h, const int64_t* d_kf_id, const int32_t* d_tag, const int32_t* d_slot, const int32_t* d_n,
                                      int list_cap, int batch, const int64_t* d_pending_kf_id, int32_t* d_pending_feat_landmark, int32_t* d_n_set);
/* src/loopclosing.cpp:524 and :529 as TrackLastFrame (src/frontend.cpp:127-171) sees them through src/keyframe.cpp:21 */
int myslam_tracker_relink_batch(myslam_tracker* h, const int64_t* d_kf_id, const int32_t* d_tag, const int32_t* d_slot, const int32_t* d_n, int list_cap,
                                const myslam_map* map, int32_t* d_n_relinked, int32_t* d_status);

/* ------------------------------------------------------------------------------------------
 * MAPPER — the Backend thread's work for a bank of S streams behind one handle: Backend::ProcessNewKeyFrame + OptimizeActiveMap
 * (src/backend.cpp:82-121, :126-266; the thread loop BackendRun, :30-37, optimises only after InsertKeyFrame) and Map::InsertKeyFrame
 * (src/map.cpp:17-48) for every stream of the bank that made a key-frame in the turn (or the StereoInit) just taken, and for no other.  The decision
 * is taken on the device: one call is one asynchronous, recordable enqueue, whatever mix of turning and tracking streams the frame holds.
 * The handle owns one myslam_backend, one myslam_map (with the solve attached, myslam_map_attach_solve) and one myslam_obs_archive for S items, the
 * back end's 13 tables (zeroed: every table starts empty) and every prior, report and status array its stages hand to each other.  Nothing moves
 * after create; myslam_mapper_view gives the pointers, so the loop-closing units work on the same state.
 *
 * Order of one call, all on the handle's stream, one workgroup per item in every stage, item s = stream s:
 *   gate -> prior_rows -> insert (those priors, the turn's outlier list) -> myslam_map_update_batch(AFTER_INSERT) ->
 *   myslam_obs_archive_update_batch(AFTER_INSERT) -> optimise (flatten, solve, write-back) -> myslam_map_update_batch(AFTER_OPTIMIZE) ->
 *   myslam_obs_archive_update_batch(AFTER_OPTIMIZE, the optimise's d_obs_report) -> myslam_tracker_clear_links_batch on the back end's culled view ->
 *   myslam_tracker_update_from_map_batch -> status
 * so both contracts of the map archive hold by construction (one back-end call between two updates of an item, the map's update first).
 * myslam_mapper_launches_per_call = 13 with a tracker (the sum of the units' own counts + 2), 11 with trk == NULL (the two tracker launches are left out).
 *
 * THE GATE (k_mapper_gate, the first launch, one i32 per item): item s takes the key-frame iff its sticky fault is 0 && d_report[s][0] == 0 &&
 * d_new_kf_id[s] >= 0.  Everything else is MYSLAM_MAPPER_IDLE: MYSLAM_TRACKER_NO_TURN, MYSLAM_TRACKER_INIT_RETRY, a turn refused with
 * MYSLAM_ERR_CAPACITY, id -1, a faulted item.  For an IDLE item no byte of its tables, of its map-archive item or of its observation-archive item
 * changes (the (-1, pose) row that myslam_backend_insert_keyframe_batch would append to an EMPTY table is never appended), the solve does not run for
 * it, its culled count is 0 and the tracker's stream keeps every byte (the outlier flags its steps have set are not in the table yet).  The insert and
 * the flatten leave with MYSLAM_MAPPER_IDLE before they read a table (csrc/backend_launch.h; the public entry points pass no gate and write what
 * they always wrote); the solve skips through its d_skip path, the write-back's status branch zeroes the reports, the two archives skip on
 * d_backend_status != 0.  The optimise is gated on the INSERT's status: an item whose insert was refused is not re-optimised either.
 *
 * d_status: S x MYSLAM_MAPPER_STATUS_WORDS i32 (k_mapper_status, the last launch).  Item that passed the gate:
 *   [0] overall: 0 mapped, or the first negative of [1..7]      [1] prior_rows      [2] insert      [3] map update after the insert
 *   [4] obs update after the insert      [5] optimise (MYSLAM_BACKEND_DONE / MYSLAM_BACKEND_EMPTY — no error: the reference returns early and the
 *   later updates skip — / an error / MYSLAM_MAPPER_IDLE after a refused insert)      [6] map update after the optimise      [7] obs update after it
 * IDLE item: [0] = MYSLAM_MAPPER_IDLE, or the item's sticky fault; [1..7] = MYSLAM_MAPPER_IDLE.
 * A negative overall status is STICKY per stream: the tracker has taken the turn, so the stream's map no longer follows it.  Every later call idles
 * the item and reports the same error until myslam_mapper_reset_item; its neighbours are served as if it were not there.
 *
 * myslam_mapper_keyframe_batch: device pointers; the thirteen outputs of myslam_tracker_keyframe_batch / _init_batch in their layout (feature stride =
 * feat_cap, outlier stride = 2 x feat_cap; d_right_xy / d_right_ok are not read and may be NULL), window = Map.activeMap.size (src/map.cpp:44),
 * min_dis_th 0.2 (:101), the solve's arguments as myslam_backend_optimize_batch takes them.  Asynchronous, never synchronises, allocates nothing,
 * recordable between myslam_graph_begin / _end.  trk: the tracker of the same S streams and feature cap on the same stream, or NULL.
 * Call level, nothing enqueued: NULL required pointers, window < 1, max_rounds < 1, iters_per_round < 1, a tracker on another stream, of another bank
 * size or feature cap -> MYSLAM_ERR_INVALID.  create: streams / caps < 1 -> MYSLAM_ERR_INVALID, feat_cap or prior_cap beyond obs_cap ->
 * MYSLAM_ERR_CAPACITY, else whatever the owned units answer to their caps (kf_cap > MYSLAM_BA_MAX_WINDOW_POSES -> MYSLAM_ERR_UNSUPPORTED ...).
 * ONE CALL CONSUMES ONE OUTPUT SET.  A frame in which some streams start and others turn is init -> mapper, then turn -> mapper: the two tracker calls
 * never share an eligible stream, but each rewrites all S output items, so they must not share buffers across one mapper call.
 *
 * myslam_mapper_reset_item — host call, synchronous; MYSLAM_ERR_UNSUPPORTED while the stream is being recorded.  Empties the stream's tables, its
 * map-archive item and its observation-archive item and clears its sticky fault: a restart after LOST, together with myslam_tracker_reset_stream.
 * myslam_mapper_set_stream sets the stream of the three owned handles too.
 * OUT OF SCOPE: loop closing — the five-key-frame skip of src/loopclosing.cpp:671-681, the store's put and everything after it (for a bank they are
 * myslam_loop_bank_gate_batch, which reads this handle's d_status, and myslam_loop_bank_finish_batch) — and DeepLCD's in-place blur of the key-frame
 * image (src/deeplcd.cpp:46), which belongs with it.
 * ------------------------------------------------------------------------------------------ */
#define MYSLAM_MAPPER_IDLE 3           /* no key-frame of this item in this call: nothing of it was touched */
#define MYSLAM_MAPPER_STATUS_WORDS 8
typedef struct myslam_mapper myslam_mapper;
typedef struct myslam_mapper_tables {
    /* the back end's 13 tables, strided by kf_cap / mp_cap / obs_cap */
    int64_t* kf_id; double* kf_pose; int32_t* n_kf; int64_t* mp_id; double* mp_pos; uint8_t* mp_outlier; int32_t* n_mp;
    int32_t* obs_mp; int32_t* obs_kf; uint8_t* obs_flags; float* obs_uv; int32_t* obs_tag; int32_t* n_obs;
    /* prior_rows' outputs (S x prior_cap) */
    int64_t* prior_mp_id; int64_t* prior_kf_id; float* prior_uv; int32_t* prior_tag; uint8_t* prior_flags; int32_t* n_prior;
    /* the insert's reports */
    int32_t* feat_row; int32_t* mp_new_row; int64_t* removed_kf_id; int32_t* removed_kf_row; double* dis;
    /* the optimise's reports */
    uint8_t* obs_report; uint8_t* mp_report; int32_t* new_outlier_mp; int32_t* n_new_outlier_mp; double* obs_chi2; int32_t* rounds; int32_t* n_outlier_edges;
    int32_t* n_cleared;                 /* myslam_tracker_clear_links_batch's */
    /* per item: the gate (0 = takes the key-frame), the sticky fault, the seven stage statuses in the order of d_status[1..7] */
    int32_t* gate; int32_t* fault; int32_t* stage_status[7];
    myslam_backend* backend; myslam_map* map; myslam_obs_archive* obs;
    int32_t streams, kf_cap, mp_cap, obs_cap, feat_cap, prior_cap;
} myslam_mapper_tables;
int myslam_mapper_create(myslam_mapper** out, int streams, int kf_cap, int mp_cap, int obs_cap, int feat_cap, int archive_kf_cap, int archive_edge_cap,
                         int archive_point_cap, int obs_row_cap, int prior_cap);
int myslam_mapper_destroy(myslam_mapper* h);
int myslam_mapper_set_stream(myslam_mapper* h, void* hip_stream);
/* the device pointers, caps and owned handles: valid until destroy */
int myslam_mapper_view(const myslam_mapper* h, myslam_mapper_tables* out);
/* src/backend.cpp:82-121, :126-266 and src/map.cpp:17-48 for the streams that made a key-frame, as described above */
int myslam_mapper_keyframe_batch(myslam_mapper* h, myslam_tracker* trk, const int64_t* d_new_kf_id, const double* d_new_kf_pose, const int64_t* d_feat_mp_id,
                                 const double* d_feat_mp_pos, const float* d_feat_uv, const int32_t* d_feat_tag, const uint8_t* d_feat_flags,
                                 const int32_t* d_n_feat, const int64_t* d_outlier_mp_id, const int32_t* d_n_outlier_mp, const float* d_right_xy,
                                 const uint8_t* d_right_ok, const int32_t* d_report, int window, double min_dis_th, double fx, double fy, double cx, double cy,
                                 double huber_delta, double chi2_th, int max_rounds, int iters_per_round, int32_t* d_status);
/* kernel launches one myslam_mapper_keyframe_batch enqueues: 13, or 11 with with_tracker == 0 */
int myslam_mapper_launches_per_call(const myslam_mapper* h, int with_tracker);
int myslam_mapper_reset_item(myslam_mapper* h, int stream);

/* ------------------------------------------------------------------------------------------
 * Host-side formats of the reference's runner — plain host code, no device needed; the C++ forms live in
 * host/myslam_io.hpp and host/myslam_png.hpp.
 * ------------------------------------------------------------------------------------------ */
/* cv::imread(file, cv::IMREAD_GRAYSCALE) for the 8-bit single-channel PNGs of KITTI image_0 / image_1 (app/run_kitti_stereo.cpp:66-67).
 * out == NULL: size query (rows, cols only).  Non-interlaced grey 8 / 16 bit, RGB / RGBA 8 bit (BGR2GRAY fixed point); else INVALID. */
int myslam_io_read_png_gray(const char* path, uint8_t* out, size_t cap_bytes, int* rows, int* cols);
/* LoadImages (app/run_kitti_stereo.cpp:114-144): *n = number of frames listed in <sequence>/times.txt; timestamps may be NULL */
int myslam_io_load_images(const char* sequence_path, double* timestamps, int cap, int* n);
/* "<sequence>/image_0/000123.png" (right != 0: image_1), :135-141 */
int myslam_io_image_path(const char* sequence_path, int index, int right, char* buf, size_t cap);
/* System::SaveTrajectory (src/system.cpp:153-180): one line "id timestamp tx ty tz qx qy qz qw" per key-frame in ascending id order,
 * std::fixed / setprecision(6), pose = KeyFrame::Pose().inverse().  poses7_cw = Tcw as qx qy qz qw tx ty tz (what every entry point
 * of this library calls a pose). */
int myslam_io_save_trajectory(const char* path, const uint64_t* ids, const double* timestamps, const double* poses7_cw, int n);
/* System::SaveLoopEdges (src/system.cpp:188-224): two lines per loop (current key-frame, loop key-frame), ordered by the current id */
int myslam_io_save_loop_edges(const char* path, const uint64_t* cur_ids, const double* cur_ts, const double* cur_poses7_cw,
                              const uint64_t* loop_ids, const double* loop_ts, const double* loop_poses7_cw, int n);

/* ------------------------------------------------------------------------------------------
 * A whole batched step as ONE HIP graph — the per-frame call pattern of the reference (one frame at a time: src/frontend.cpp:302-328,
 * src/loopclosing.cpp:83-121) is launch-bound on a GPU: ~90 launches on 4-5 streams cost the host ~0.6 ms however few frames they carry.
 * Every *_batch entry point is asynchronous and allocation-free after its first call with a given shape, so a caller records one step
 * between begin and end — the calls it would make anyway, on the streams it would use — and replays it with one launch per step.
 *   begin: starts a thread-local capture on origin_stream and forks the side streams into it (they must be distinct from the origin);
 *   end:   joins the side streams back, ends the capture and instantiates the graph; a recording whose calls failed must still be ended with it.
 * Rules: run the step once eagerly first (lazy allocations); profiling must be off (MYSLAM_ERR_UNSUPPORTED); events passed to
 * myslam_orb_set_fast_gate must be recorded INSIDE the capture (the first handle of a ring takes no gate); buffers, handles, options and
 * streams the step uses must stay as they were; host code is not replayed — record TWO consecutive steps and replay them alternately so
 * that the extractor's FAST statistics keep ping-ponging, and feed the loop database's row limits through
 * myslam_lcddb_update_query_limits.  Results are bit-identical to the eager step (tests/test_gpu_graph.py).
 * Other threads: HIP's legacy NULL stream synchronises with every blocking stream, so while ANY thread records on a blocking stream no thread may
 * issue work on the legacy stream (HIP refuses it and the recording is lost).  The library stays off the legacy stream: handles and plans, the batch
 * entry points, and the synchronous host-pointer calls (PnP-RANSAC, pose graph, map-point correction: a non-blocking stream per calling thread) —
 * tests/test_gpu_threads.py runs four threads, each recording its own one-frame calls while the others create plans.  Only the myslam_*_debug_*
 * getters copy through it.
 * ------------------------------------------------------------------------------------------ */
typedef struct myslam_step_graph myslam_step_graph;
int myslam_graph_begin(void* origin_stream, void* const* side_streams, int n_side);
int myslam_graph_end(void* origin_stream, void* const* side_streams, int n_side, myslam_step_graph** out);
int myslam_graph_launch(myslam_step_graph* g, void* hip_stream);
int myslam_graph_node_count(const myslam_step_graph* g);
int myslam_graph_destroy(myslam_step_graph* g);

#ifdef __cplusplus
}
#endif
#endif /* MYSLAM_HIP_H */
