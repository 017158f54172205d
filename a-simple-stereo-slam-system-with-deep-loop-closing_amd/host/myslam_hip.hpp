// myslam_hip.hpp — C++ facade over the C ABI (include/myslam_hip.h) with the reference's own class and method
// names, so that Frontend / LoopClosing / Backend code of libmyslam.so keeps compiling against it:
//
//   myslam::ORBextractor   include/myslam/ORBextractor.h:52-110   (Detect, DetectAndCompute,
//                                                                  ScreenAndComputeKPsParams, CalcDescriptors, getters)
//   myslam::DeepLCD        include/myslam/deeplcd.h:21-48          (calcDescrOriginalImg, calcDescr, score, DescrVector)
//   myslam::BFMatcherHamming::match                                 (cv::BFMatcher use at src/loopclosing.cpp:33,172)
//   myslam::triangulation  include/myslam/algorithm.h:16-33        (stereo rig form)
//   myslam::LoopDatabase   LoopClosing::DetectLoop / AddToDatabase  src/loopclosing.cpp:124-161, 651-659
//   myslam::LoopDatabaseBank   the same per stream of a bank, ids and counts on the device   src/loopclosing.cpp:62, 126-143, 651-659
//   myslam::LocalBA::{Build,Optimize,OptimizeActiveMap}  Backend::OptimizeActiveMap  src/backend.cpp:126-243
//   myslam::PyrLKTracker::calcOpticalFlowPyrLK        cv::calcOpticalFlowPyrLK call sites        src/frontend.cpp:150-153, 358-361
//   myslam::EstimateCurrentPose                       g2o stage of Frontend::EstimateCurrentPose src/frontend.cpp:176-276
//   myslam::KeyFrameFeatures / MatchFeatures          KeyFrame::{mvPyramidKeyPoints, mORBDescriptors} + LoopClosing::ProcessNewKF /
//                                                     MatchFeatures bookkeeping                   src/loopclosing.cpp:83-121, 163-203
//   myslam::LoopLocalFusion                           arithmetic of LoopClosing::LoopLocalFusion  src/loopclosing.cpp:466-507
//   myslam::Camera::UndistortImage                    cv::undistort of Frontend::GrabStereoImage  src/camera.cpp:36-48, frontend.cpp:47-51
//
// No OpenCV / Eigen / g2o: images are (data, rows, cols, step) views, cv::KeyPoint is the layout-compatible
// myslam_keypoint, DescrVector is std::array<float,1064>.  Errors the reference reports by logging + return keep
// that behaviour (empty inputs are no-ops); everything else throws std::runtime_error.  There is no CPU fallback.
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <algorithm>
#include <vector>

#include "../../include/myslam_hip.h"

namespace myslam {

struct ImageView {            // cv::Mat CV_8UC1 stand-in
    uint8_t* data = nullptr;
    int rows = 0, cols = 0, step = 0;
    bool empty() const { return !data || rows <= 0 || cols <= 0; }
};
using KeyPoint = myslam_keypoint;                       // cv::KeyPoint layout
struct DMatch { int queryIdx, trainIdx, imgIdx; float distance; };
using Descriptors = std::vector<uint8_t>;               // N x 32, row-major (cv::Mat CV_8UC1 N x 32)

inline void check(int rc, const char* what) {
    if (rc != MYSLAM_OK) throw std::runtime_error(std::string(what) + " failed with status " + std::to_string(rc));
}

class ORBextractor {
   public:
    ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST)
        : nfeatures_(nfeatures), nlevels_(nlevels) {
        check(myslam_orb_create(&h_, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST), "myslam_orb_create");
        mvScaleFactor.resize(nlevels); mvInvScaleFactor.resize(nlevels); mnFeaturesPerLevel.resize(nlevels); umax.resize(16);
        check(myslam_orb_get_tables(h_, mvScaleFactor.data(), mvInvScaleFactor.data(), mnFeaturesPerLevel.data(), umax.data()),
              "myslam_orb_get_tables");
        mvLevelSigma2.resize(nlevels); mvInvLevelSigma2.resize(nlevels);
        for (int i = 0; i < nlevels; i++) { mvLevelSigma2[i] = mvScaleFactor[i] * mvScaleFactor[i]; mvInvLevelSigma2[i] = 1.0f / mvLevelSigma2[i]; }
    }
    ~ORBextractor() { if (h_) myslam_orb_destroy(h_); }
    ORBextractor(const ORBextractor&) = delete;
    ORBextractor& operator=(const ORBextractor&) = delete;

    // ORBextractor.h:61-63
    void DetectAndCompute(const ImageView& image, const ImageView& mask, std::vector<KeyPoint>& keypoints, Descriptors& descriptors) {
        keypoints.clear(); descriptors.clear();
        if (image.empty()) return;                                               // ORBextractor.cpp:924
        const int cap = myslam_orb_max_keypoints_for(h_, image.rows, image.cols);
        keypoints.resize(cap); descriptors.resize((size_t)cap * 32);
        int n = 0;
        check(myslam_orb_detect_and_compute(h_, image.data, image.rows, image.cols, image.step, mask.empty() ? nullptr : mask.data,
                                            mask.step, keypoints.data(), descriptors.data(), cap, &n), "myslam_orb_detect_and_compute");
        keypoints.resize(n); descriptors.resize((size_t)n * 32);
    }
    // ORBextractor.h:70-71
    void Detect(const ImageView& image, const ImageView& mask, std::vector<KeyPoint>& keypoints) {
        keypoints.clear();
        if (image.empty()) return;                                               // ORBextractor.cpp:990
        const int cap = myslam_orb_max_keypoints_for(h_, image.rows, image.cols);
        keypoints.resize(cap);
        int n = 0;
        check(myslam_orb_detect(h_, image.data, image.rows, image.cols, image.step, mask.empty() ? nullptr : mask.data, mask.step,
                                keypoints.data(), cap, &n), "myslam_orb_detect");
        keypoints.resize(n);
    }
    // ORBextractor.h:83-84 (keypoints is updated in place exactly as the reference's loop does)
    void ScreenAndComputeKPsParams(const ImageView& image, std::vector<KeyPoint>& keypoints, std::vector<KeyPoint>& out_keypoints) {
        out_keypoints.clear();
        if (image.empty() || keypoints.empty()) return;                          // ORBextractor.cpp:1085-1088
        out_keypoints.resize(keypoints.size());
        int n = 0;
        check(myslam_orb_screen_and_compute_params(h_, image.data, image.rows, image.cols, image.step, keypoints.data(),
                                                   (int)keypoints.size(), out_keypoints.data(), (int)out_keypoints.size(), &n),
              "myslam_orb_screen_and_compute_params");
        out_keypoints.resize(n);
    }
    // ORBextractor.h:65-67
    void CalcDescriptors(const ImageView& image, const std::vector<KeyPoint>& keypoints, Descriptors& descriptors) {
        descriptors.clear();
        if (image.empty() || keypoints.empty()) return;                          // ORBextractor.cpp:1183-1186
        descriptors.resize(keypoints.size() * 32);
        check(myslam_orb_calc_descriptors(h_, image.data, image.rows, image.cols, image.step, keypoints.data(), (int)keypoints.size(),
                                          descriptors.data()), "myslam_orb_calc_descriptors");
    }
    // scheduling / parity knobs (no reference counterpart; see include/myslam_hip.h)
    void SetOption(int option, int value) { check(myslam_orb_set_option(h_, option, value), "myslam_orb_set_option"); }
    void SetGaussTaps(const int32_t* q7) { check(myslam_orb_set_gauss_taps(h_, q7), "myslam_orb_set_gauss_taps"); }
    // getters, ORBextractor.h:87-107
    int GetLevels() const { return nlevels_; }
    float GetScaleFactor() const { return mvScaleFactor.size() > 1 ? mvScaleFactor[1] : 1.f; }
    const std::vector<float>& GetScaleFactors() const { return mvScaleFactor; }
    const std::vector<float>& GetInverseScaleFactors() const { return mvInvScaleFactor; }
    const std::vector<float>& GetScaleSigmaSquares() const { return mvLevelSigma2; }
    const std::vector<float>& GetInverseScaleSigmaSquares() const { return mvInvLevelSigma2; }
    myslam_orb* handle() { return h_; }

    std::vector<float> mvScaleFactor, mvInvScaleFactor, mvLevelSigma2, mvInvLevelSigma2;
    std::vector<int> mnFeaturesPerLevel, umax;

   private:
    myslam_orb* h_ = nullptr;
    int nfeatures_, nlevels_;
};

class DeepLCD {
   public:
    using DescrVector = std::array<float, MYSLAM_LCD_DIM>;     // Eigen::Matrix<float,1064,1>, deeplcd.h:25
    // DeepLCD(network_definition_file, pre_trained_model_file, gpu_id) deeplcd.h:33: the reference's own two files, read without Caffe
    DeepLCD(const std::string& network_definition_file, const std::string& pre_trained_model_file, int /*gpu_id*/ = -1) {
        check(myslam_lcd_create_from_caffe(&h_, network_definition_file.c_str(), pre_trained_model_file.c_str()), "myslam_lcd_create_from_caffe");
    }
    // own model file (CALCW1 / CALCW2, csrc/calc.hip)
    explicit DeepLCD(const std::string& weights_file) { check(myslam_lcd_create_from_file(&h_, weights_file.c_str()), "myslam_lcd_create_from_file"); }
    bool UsesFusedKernels() const { return myslam_lcd_uses_fused_kernels(h_) == 1; }
    DeepLCD(const float* weights, size_t n) { check(myslam_lcd_create(&h_, weights, n), "myslam_lcd_create"); }
    ~DeepLCD() { if (h_) myslam_lcd_destroy(h_); }
    DeepLCD(const DeepLCD&) = delete;
    DeepLCD& operator=(const DeepLCD&) = delete;
    float score(const DescrVector& d1, const DescrVector& d2) const { return myslam_lcd_score(d1.data(), d2.data()); }   // deeplcd.cpp:35-39
    // deeplcd.cpp:43-52 — blurs originalImg in place, like the reference
    DescrVector calcDescrOriginalImg(const ImageView& originalImg) {
        DescrVector d;
        check(myslam_lcd_calc_descr_original_img(h_, originalImg.data, originalImg.rows, originalImg.cols, originalImg.step, 1, d.data()),
              "myslam_lcd_calc_descr_original_img");
        return d;
    }
    DescrVector calcDescr(const ImageView& im160x120) {            // deeplcd.cpp:55-91
        DescrVector d;
        check(myslam_lcd_calc_descr(h_, im160x120.data, im160x120.step, d.data()), "myslam_lcd_calc_descr");
        return d;
    }

   private:
    myslam_lcd* h_ = nullptr;
};

struct BFMatcherHamming {      // cv::DescriptorMatcher::create("BruteForce-Hamming")->match(query, train, matches)
    static void match(const Descriptors& query, const Descriptors& train, std::vector<DMatch>& matches) {
        const int nq = (int)(query.size() / 32), nt = (int)(train.size() / 32);
        std::vector<int32_t> idx(nq), dist(nq);
        check(myslam_hamming_match(query.data(), nq, train.data(), nt, idx.data(), dist.data()), "myslam_hamming_match");
        matches.resize(nq);
        for (int i = 0; i < nq; i++) matches[i] = DMatch{i, idx[i], 0, (float)dist[i]};
    }
};

// What LoopClosing keeps per key-frame for loop verification (include/myslam/keyframe.h:44-52): the pyramid key-points that survived
// ScreenAndComputeKPsParams (class_id = index of the feature they belong to) and their descriptors.
struct KeyFrameFeatures {
    std::vector<KeyPoint> mvPyramidKeyPoints;
    Descriptors mORBDescriptors;
    // LoopClosing::ProcessNewKF, src/loopclosing.cpp:94-112.  `image` is the key-frame's left image AFTER DeepLCD::calcDescrOriginalImg
    // blurred it in place (the reference's order of calls); featureKeyPoints = mvpFeaturesLeft[i]->mkpPosition.
    void Compute(ORBextractor& extractor, const ImageView& image, const std::vector<KeyPoint>& featureKeyPoints) {
        const int nl = extractor.GetLevels();
        std::vector<KeyPoint> pyr(featureKeyPoints.size() * (size_t)nl);
        check(myslam_expand_pyramid_keypoints(featureKeyPoints.data(), (int)featureKeyPoints.size(), nl, pyr.data()), "myslam_expand_pyramid_keypoints");
        extractor.ScreenAndComputeKPsParams(image, pyr, mvPyramidKeyPoints);
        extractor.CalcDescriptors(image, mvPyramidKeyPoints, mORBDescriptors);
    }
};

// LoopClosing::MatchFeatures, src/loopclosing.cpp:163-203: BFMatcher(loop -> current), distance filter, (current feature, loop feature)
// pairs in the order of the reference's std::set.  false when fewer than 10 pairs survive (:196).
inline bool MatchFeatures(const KeyFrameFeatures& loopKF, const KeyFrameFeatures& currentKF, std::vector<std::pair<int, int>>& validFeatureMatches) {
    validFeatureMatches.clear();
    const int nq = (int)loopKF.mvPyramidKeyPoints.size(), nt = (int)currentKF.mvPyramidKeyPoints.size();
    if (nq == 0 || nt == 0) return false;
    std::vector<int32_t> idx(nq), dist(nq), pairs((size_t)nq * 2);
    check(myslam_hamming_match(loopKF.mORBDescriptors.data(), nq, currentKF.mORBDescriptors.data(), nt, idx.data(), dist.data()), "myslam_hamming_match");
    int np = 0;
    check(myslam_match_feature_pairs(idx.data(), dist.data(), nq, loopKF.mvPyramidKeyPoints.data(), currentKF.mvPyramidKeyPoints.data(), nt,
                                     pairs.data(), &np), "myslam_match_feature_pairs");
    for (int k = 0; k < np; k++) validFeatureMatches.emplace_back(pairs[2 * k], pairs[2 * k + 1]);
    return np >= 10;
}

// LoopClosing::LoopLocalFusion, src/loopclosing.cpp:466-507 (the arithmetic; re-linking observations :509-532 stays with the Map):
// activePoses (n x 7, in/out) move rigidly with the corrected current key-frame, points (n x 3, in/out) follow firstActiveKF[i] (< 0 = skip)
inline void LoopLocalFusion(std::vector<double>& activePoses, int currentIndex, const double correctedCurrentPose[7],
                            const std::vector<int32_t>& firstActiveKF, std::vector<double>& points) {
    check(myslam_loop_local_fusion(activePoses.data(), (int)(activePoses.size() / 7), currentIndex, correctedCurrentPose, firstActiveKF.data(),
                                   points.data(), (int)firstActiveKF.size()), "myslam_loop_local_fusion");
}

// triangulation() of algorithm.h:16-33 for the stereo rig (left ext = I, right ext t = (-baseline,0,0)); ok = success && z > 0
inline void triangulation(const std::vector<float>& xl, const std::vector<float>& yl, const std::vector<float>& xr,
                          const std::vector<float>& yr, double fx, double fy, double cx, double cy, double baseline,
                          std::vector<std::array<double, 3>>& pts, std::vector<uint8_t>& ok) {
    const int n = (int)xl.size();
    pts.resize(n); ok.resize(n);
    check(myslam_triangulate_stereo(xl.data(), yl.data(), xr.data(), yr.data(), n, fx, fy, cx, cy, baseline,
                                    reinterpret_cast<double*>(pts.data()), ok.data()), "myslam_triangulate_stereo");
}

class LoopDatabase {           // LoopClosing::_mvDatabase + DetectLoop + AddToDatabase
   public:
    explicit LoopDatabase(int capacity, float thresHigh = 0.94f, float thresLow = 0.92f) : th1_(thresHigh), th2_(thresLow) {
        check(myslam_lcddb_create(&h_, capacity), "myslam_lcddb_create");
    }
    ~LoopDatabase() { if (h_) myslam_lcddb_destroy(h_); }
    LoopDatabase(const LoopDatabase&) = delete;
    LoopDatabase& operator=(const LoopDatabase&) = delete;
    void AddToDatabase(unsigned long kfId, const DeepLCD::DescrVector& d) { check(myslam_lcddb_append(h_, kfId, d.data()), "myslam_lcddb_append"); }
    size_t size() const { return (size_t)myslam_lcddb_size(h_); }
    size_t capacity() const { return (size_t)myslam_lcddb_capacity(h_); }          // grows by itself (std::map has no bound); reserve() avoids the moves
    void reserve(int rows) { check(myslam_lcddb_reserve(h_, rows), "myslam_lcddb_reserve"); }
    // loopclosing.cpp:124-161: true + loop KF id when maxScore >= high threshold and at most 3 scores exceed the low one
    bool DetectLoop(unsigned long curKFId, const DeepLCD::DescrVector& d, unsigned long& loopKFId, float* maxScore = nullptr) {
        uint64_t best = 0; float mx = 0; int cnt = 0;
        check(myslam_lcddb_query(h_, d.data(), curKFId, th2_, &best, &mx, &cnt), "myslam_lcddb_query");
        if (maxScore) *maxScore = mx;
        if (mx < th1_ || cnt > 3) return false;
        loopKFId = best;
        return true;
    }

   private:
    myslam_lcddb* h_ = nullptr;
    float th1_, th2_;
};

// S LoopDatabases in one device allocation, item s = stream s of a TrackerBank: each stream's _mvDatabase with its ids, row count and scan limits on the
// device.  QueryBatch is the gate of LoopClosing::Run (src/loopclosing.cpp:62) and DetectLoop's scan (:126-143) per stream, and writes
// LoopKeyFrameStore::DetectBatch's three inputs; AppendBatch is AddToDatabase (:651-659) for the streams the caller selects.  Device pointers; every
// batch call enqueues on the handle's stream and returns, and can be recorded.  Load / Get / Sizes take host memory and wait.
class LoopDatabaseBank {
    myslam_lcdbank* h_ = nullptr;
    int streams_, rowsPerStream_;
public:
    LoopDatabaseBank(int streams, int rowsPerStream, float thresLow = 0.92f, int databaseMinSize = 0)
        : streams_(streams), rowsPerStream_(rowsPerStream), th2_(thresLow), minSize_(databaseMinSize) {
        check(myslam_lcdbank_create(&h_, streams, rowsPerStream), "myslam_lcdbank_create");
    }
    ~LoopDatabaseBank() { if (h_) myslam_lcdbank_destroy(h_); }
    LoopDatabaseBank(const LoopDatabaseBank&) = delete; LoopDatabaseBank& operator=(const LoopDatabaseBank&) = delete;
    int streams() const { return streams_; }
    int rowsPerStream() const { return rowsPerStream_; }
    static int rowTile() { return myslam_lcdbank_row_tile(); }
    static int launchesPerQuery() { return myslam_lcdbank_launches_per_query(); }
    void SetStream(void* hipStream) { check(myslam_lcdbank_set_stream(h_, hipStream), "myslam_lcdbank_set_stream"); }
    // status[s] = MYSLAM_LCDBANK_SCANNED / _GATED / _IDLE; d_active may be nullptr (every stream)
    void QueryBatch(const float* d_descr, const uint64_t* d_curKFId, const int32_t* d_active, uint64_t* d_bestId, float* d_maxScore,
                    int32_t* d_cntSuspected, int32_t* d_bestRow, int32_t* d_status) {
        check(myslam_lcdbank_query_batch(h_, d_descr, d_curKFId, d_active, th2_, minSize_, d_bestId, d_maxScore, d_cntSuspected, d_bestRow, d_status),
              "myslam_lcdbank_query_batch");
    }
    // status[s] = MYSLAM_LCDBANK_ADDED / _IDLE / MYSLAM_ERR_CAPACITY / MYSLAM_ERR_INVALID; d_add may be nullptr (every stream)
    void AppendBatch(const float* d_descr, const uint64_t* d_kfId, const int32_t* d_add, int32_t* d_status) {
        check(myslam_lcdbank_append_batch(h_, d_descr, d_kfId, d_add, d_status), "myslam_lcdbank_append_batch");
    }
    void ClearBatch(const int32_t* d_clear) { check(myslam_lcdbank_clear_batch(h_, d_clear), "myslam_lcdbank_clear_batch"); }
    void View(const float** d_rows, const uint64_t** d_ids, const int32_t** d_n) const { check(myslam_lcdbank_view(h_, d_rows, d_ids, d_n), "myslam_lcdbank_view"); }
    void Load(int stream, const std::vector<uint64_t>& ids, const std::vector<float>& rows) {
        if (rows.size() != ids.size() * MYSLAM_LCD_DIM) throw std::runtime_error("LoopDatabaseBank::Load: rows and ids differ in length");
        check(myslam_lcdbank_load(h_, stream, ids.data(), rows.data(), (int)ids.size()), "myslam_lcdbank_load");
    }
    void Get(int stream, std::vector<uint64_t>& ids, std::vector<float>& rows) {
        ids.assign(rowsPerStream_, 0); rows.assign((size_t)rowsPerStream_ * MYSLAM_LCD_DIM, 0.f);
        int n = 0;
        check(myslam_lcdbank_get(h_, stream, ids.data(), rows.data(), rowsPerStream_, &n), "myslam_lcdbank_get");
        ids.resize(n); rows.resize((size_t)n * MYSLAM_LCD_DIM);
    }
    std::vector<int32_t> Sizes() {
        std::vector<int32_t> n(streams_);
        check(myslam_lcdbank_sizes(h_, n.data()), "myslam_lcdbank_sizes");
        return n;
    }

private:
    float th2_;
    int minSize_;
};

struct LocalBA {               // flat-array form of the graph Backend::OptimizeActiveMap builds (backend.cpp:139-206)
    std::vector<double> poses, points, obs;          // nposes x 7 (qx qy qz qw tx ty tz = KeyFrame::Pose()), npts x 3, nedges x 2
    std::vector<int32_t> edge_pose, edge_pt;
    std::vector<uint8_t> fixed;                      // setFixed rule of backend.cpp:175-177
    double fx = 0, fy = 0, cx = 0, cy = 0, huber_delta = 5.991;   // backend.cpp:155,199
    std::vector<double> Hpp, Hll, Hpl, bp, bl, chi2;
    // --- Map -> flat arrays (backend.cpp:139-206): copy the Map's tables into the *Table members, call Flatten(), and the arrays above
    // are filled; after OptimizeActiveMap() pose slot p belongs to key-frame kf_ids[pose_src[p]], landmark slot j to map point
    // mp_ids[pt_src[j]] and edge k to observation row edge_src[k] (outlier[k] -> that feature's mbIsOutlier, :234-250)
    std::vector<uint64_t> kf_ids; std::vector<double> kf_pose7;                                       // Map::GetActiveKeyFrames(): mnKFId, Pose()
    std::vector<uint64_t> mp_ids, mp_first_observer_kf; std::vector<uint8_t> mp_outlier; std::vector<double> mp_pos;   // GetActiveMapPoints()
    std::vector<uint64_t> obs_mp_id, obs_kf_id; std::vector<float> obs_uv; std::vector<uint8_t> obs_feat_outlier;    // GetActiveObservations()
    std::vector<int32_t> pose_src, pt_src, edge_src;
    void AddKeyFrame(uint64_t kfId, const double pose7[7]) { kf_ids.push_back(kfId); kf_pose7.insert(kf_pose7.end(), pose7, pose7 + 7); }
    void AddMapPoint(uint64_t id, const double pos[3], bool isOutlier, uint64_t firstObserverKFId) {
        mp_ids.push_back(id); mp_pos.insert(mp_pos.end(), pos, pos + 3); mp_outlier.push_back(isOutlier); mp_first_observer_kf.push_back(firstObserverKFId);
    }
    void AddObservation(uint64_t mpId, uint64_t kfId, float u, float v, bool featureIsOutlier) {
        obs_mp_id.push_back(mpId); obs_kf_id.push_back(kfId); obs_uv.push_back(u); obs_uv.push_back(v); obs_feat_outlier.push_back(featureIsOutlier);
    }
    void Flatten() {
        const int nk = (int)kf_ids.size(), nm = (int)mp_ids.size(), no = (int)obs_mp_id.size();
        pose_src.assign(nk, 0); pt_src.assign(nm, 0); fixed.assign(nm, 0);
        edge_pose.assign(no, 0); edge_pt.assign(no, 0); edge_src.assign(no, 0); obs.assign((size_t)no * 2, 0);
        int32_t L = 0, E = 0;
        check(myslam_ba_flatten_window(kf_ids.data(), nk, mp_ids.data(), mp_outlier.data(), mp_first_observer_kf.data(), nm, obs_mp_id.data(),
                                       obs_kf_id.data(), obs_uv.data(), obs_feat_outlier.data(), no, pose_src.data(), pt_src.data(), &L,
                                       edge_pose.data(), edge_pt.data(), obs.data(), edge_src.data(), &E, fixed.data()), "myslam_ba_flatten_window");
        pt_src.resize(L); fixed.resize(L); edge_pose.resize(E); edge_pt.resize(E); edge_src.resize(E); obs.resize((size_t)E * 2);
        poses.resize((size_t)nk * 7); points.resize((size_t)L * 3);
        for (int p = 0; p < nk; p++) std::copy(kf_pose7.begin() + 7 * pose_src[p], kf_pose7.begin() + 7 * pose_src[p] + 7, poses.begin() + 7 * p);
        for (int j = 0; j < L; j++) std::copy(mp_pos.begin() + 3 * pt_src[j], mp_pos.begin() + 3 * pt_src[j] + 3, points.begin() + 3 * j);
    }
    void Build() {
        const int P = (int)(poses.size() / 7), L = (int)(points.size() / 3), E = (int)edge_pose.size();
        Hpp.assign((size_t)P * 36, 0); Hll.assign((size_t)L * 9, 0); Hpl.assign((size_t)E * 18, 0);
        bp.assign((size_t)P * 6, 0); bl.assign((size_t)L * 3, 0); chi2.assign(E, 0);
        check(myslam_ba_build(poses.data(), P, points.data(), L, edge_pose.data(), edge_pt.data(), obs.data(), E,
                              fixed.empty() ? nullptr : fixed.data(), fx, fy, cx, cy, huber_delta, Hpp.data(), Hll.data(), Hpl.data(),
                              bp.data(), bl.data(), chi2.data()), "myslam_ba_build");
    }
    // optimizer.optimize(n) of backend.cpp:212-214 on the device: poses / points are updated in place
    int Optimize(int iterations = 10, double* final_chi2 = nullptr) {
        const int P = (int)(poses.size() / 7), L = (int)(points.size() / 3), E = (int)edge_pose.size();
        int it = 0;
        check(myslam_ba_optimize(poses.data(), P, points.data(), L, edge_pose.data(), edge_pt.data(), obs.data(), E,
                                 fixed.empty() ? nullptr : fixed.data(), fx, fy, cx, cy, huber_delta, iterations, final_chi2, &it),
              "myslam_ba_optimize");
        return it;
    }
    // the whole solve stage, backend.cpp:208-243: rounds of optimize(10) until the inlier ratio passes 0.5, then the outlier
    // flags (outlier[k] != 0 <=> the reference sets feature->mbIsOutlier and detaches it, :232-249); chi2[k] = edge->chi2()
    std::vector<uint8_t> outlier;
    int OptimizeActiveMap(double chi2_th = 5.991, int max_rounds = 5, int iters_per_round = 10) {
        const int P = (int)(poses.size() / 7), L = (int)(points.size() / 3), E = (int)edge_pose.size();
        chi2.assign(E, 0); outlier.assign(E, 0);
        int rounds = 0, nout = 0;
        check(myslam_ba_optimize_active_map(poses.data(), P, points.data(), L, edge_pose.data(), edge_pt.data(), obs.data(), E,
                                            fixed.empty() ? nullptr : fixed.data(), fx, fy, cx, cy, huber_delta, chi2_th, max_rounds,
                                            iters_per_round, chi2.data(), outlier.data(), &rounds, &nout),
              "myslam_ba_optimize_active_map");
        return nout;
    }
};

// flat-array form of the graph LoopClosing::PoseGraphOptimization builds (loopclosing.cpp:546-601) and of its write-back (:612-640)
struct PoseGraph {
    std::vector<double> poses;                       // nKF x 7 (qx qy qz qw tx ty tz) = KeyFrame::Pose() of every key-frame, index = position in the list
    std::vector<uint8_t> fixed;                      // :557-562: active key-frames, the loop key-frame, key-frame 0
    std::vector<int32_t> edge_v0, edge_v1;           // EdgePoseGraph vertices 0 / 1 (:581-582, :594-595)
    std::vector<double> meas;                        // nedges x 7: mRelativePoseToLastKF / mRelativePoseToLoopKF (:583, :596)
    void AddKeyFrame(const double pose7[7], bool isFixed) { poses.insert(poses.end(), pose7, pose7 + 7); fixed.push_back(isFixed); }
    void AddEdge(int kf, int otherKf, const double relPose7[7]) { edge_v0.push_back(kf); edge_v1.push_back(otherKf); meas.insert(meas.end(), relPose7, relPose7 + 7); }
    // optimizer.initializeOptimization(); optimizer.optimize(20) (:605-606); poses are replaced by the optimised estimates (:636-638)
    int Optimize(int iterations = 20, double* final_chi2 = nullptr) {
        int it = 0;
        check(myslam_pose_graph_optimize(poses.data(), (int)(poses.size() / 7), fixed.data(), edge_v0.data(), edge_v1.data(), meas.data(),
                                         (int)edge_v0.size(), iterations, final_chi2, &it), "myslam_pose_graph_optimize");
        return it;
    }
    // :621-633: points (n x 3, in/out) keep their camera-frame position in first_kf[i] (index into poses; < 0 = skip)
    static void CorrectMapPoints(const std::vector<double>& old_poses, const std::vector<double>& new_poses, const std::vector<int32_t>& first_kf,
                                 std::vector<double>& points) {
        check(myslam_correct_map_points(old_poses.data(), new_poses.data(), (int)(old_poses.size() / 7), first_kf.data(), points.data(),
                                        (int)first_kf.size()), "myslam_correct_map_points");
    }
};

// cv::calcOpticalFlowPyrLK(prev, next, prevPts, nextPts, status, err, Size(11,11), 3, TermCriteria(COUNT+EPS,30,0.01),
// OPTFLOW_USE_INITIAL_FLOW) as Frontend::TrackLastFrame / FindFeaturesInRight call it (src/frontend.cpp:150-153, 358-361)
struct Point2f { float x, y; };
class PyrLKTracker {
    myslam_lk* h_ = nullptr;
public:
    explicit PyrLKTracker(int win = 11, int maxLevel = 3, int maxCount = 30, float epsilon = 0.01f, float minEigThreshold = 1e-4f) {
        check(myslam_lk_create(&h_, win, maxLevel, maxCount, epsilon, minEigThreshold), "myslam_lk_create");
    }
    ~PyrLKTracker() { if (h_) myslam_lk_destroy(h_); }
    PyrLKTracker(const PyrLKTracker&) = delete; PyrLKTracker& operator=(const PyrLKTracker&) = delete;
    // nextPts carries the initial flow on entry (the reference always provides one)
    void calcOpticalFlowPyrLK(const ImageView& prevImg, const ImageView& nextImg, const std::vector<Point2f>& prevPts,
                              std::vector<Point2f>& nextPts, std::vector<uint8_t>& status, std::vector<float>& err) {
        const int n = (int)prevPts.size();
        if ((int)nextPts.size() != n) nextPts = prevPts;
        status.assign(n, 0); err.assign(n, 0.f);
        if (n == 0) return;
        check(myslam_lk_track(h_, prevImg.data, nextImg.data, prevImg.rows, prevImg.cols, prevImg.step, nextImg.step,
                              reinterpret_cast<const float*>(prevPts.data()), reinterpret_cast<float*>(nextPts.data()), n, status.data(), err.data()),
              "myslam_lk_track");
    }
    // the same with the handle's two-image cache (myslam_lk_track_cached): a non-zero token names an image whose bytes never change
    void calcOpticalFlowPyrLK(const ImageView& prevImg, uint64_t prevToken, const ImageView& nextImg, uint64_t nextToken, const std::vector<Point2f>& prevPts,
                              std::vector<Point2f>& nextPts, std::vector<uint8_t>& status, std::vector<float>& err) {
        const int n = (int)prevPts.size();
        if ((int)nextPts.size() != n) nextPts = prevPts;
        status.assign(n, 0); err.assign(n, 0.f);
        if (n == 0) return;
        check(myslam_lk_track_cached(h_, prevImg.data, prevToken, nextImg.data, nextToken, prevImg.rows, prevImg.cols, prevImg.step, nextImg.step,
                                     reinterpret_cast<const float*>(prevPts.data()), reinterpret_cast<float*>(nextPts.data()), n, status.data(), err.data()),
              "myslam_lk_track_cached");
    }
    // asynchronous upload + pyramid of the image the next cached call will name by `token` (it must stay valid and unchanged until then)
    void Prefetch(const ImageView& img, uint64_t token) { check(myslam_lk_prefetch(h_, img.data, token, img.rows, img.cols, img.step), "myslam_lk_prefetch"); }
};

// Frontend::Track() (src/frontend.cpp:86-122) for `streams` cameras of one image size and calibration at once, the tracker state of every
// stream on the device (myslam_tracker_*): Step() advances every stream that is not frozen by one frame and never waits for the device;
// a stream whose result says needs_host takes its key-frame work on the host between GetFrame() and SetFrame().
class TrackerBank {
    myslam_tracker* h_ = nullptr;
    int streams_, rows_, cols_, cap_, lmCap_;
public:
    struct StreamState {            // what SetFrame uploads and GetFrame downloads
        std::vector<Point2f> features; std::vector<int32_t> landmarkOf;          // last frame's features, slot of the landmark table or -1
        std::vector<double> landmarkPos; std::vector<uint8_t> landmarkIsOutlier;   // n x 3, n
        double refPose[7] = {0, 0, 0, 1, 0, 0, 0}; int refFrameId = 0;
        double lastRel[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, relMotion[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        int nextFrameId = 0, status = 0, kfEvery = 0, frozen = 0;
        std::vector<int32_t> outlierLandmarks;                                     // GetFrame only: Map::AddOutlierMapPoint order
    };
    TrackerBank(int streams, int rows, int cols, int cap, int landmarkCap, double fx, double fy, double cx, double cy, int trackingGood = 50,
                int trackingBad = 10, int win = 11, int maxLevel = 3, int maxCount = 30, float epsilon = 0.01f, float minEigThreshold = 1e-4f)
        : streams_(streams), rows_(rows), cols_(cols), cap_(cap), lmCap_(landmarkCap) {
        check(myslam_tracker_create(&h_, streams, rows, cols, cap, landmarkCap, fx, fy, cx, cy, trackingGood, trackingBad, win, maxLevel, maxCount, epsilon,
                                    minEigThreshold), "myslam_tracker_create");
    }
    ~TrackerBank() { if (h_) myslam_tracker_destroy(h_); }
    TrackerBank(const TrackerBank&) = delete; TrackerBank& operator=(const TrackerBank&) = delete;
    int streams() const { return streams_; }
    myslam_tracker* handle() const { return h_; }
    int launchesPerStep() const { return myslam_tracker_launches_per_step(h_); }
    void SetStream(void* hipStream) { check(myslam_tracker_set_stream(h_, hipStream), "myslam_tracker_set_stream"); }
    // prevImage: the image the next step tracks FROM (a key-frame's image after DeepLCD blurred it in place); nullptr keeps the last step's
    void SetFrame(int stream, const StreamState& s, const ImageView* prevImage = nullptr) {
        check(myslam_tracker_set_frame(h_, stream, reinterpret_cast<const float*>(s.features.data()), s.landmarkOf.data(), (int)s.features.size(),
                                       s.landmarkPos.data(), s.landmarkIsOutlier.data(), (int)s.landmarkIsOutlier.size(), s.refPose, s.refFrameId, s.lastRel,
                                       s.relMotion, s.nextFrameId, s.status, s.kfEvery, prevImage ? prevImage->data : nullptr, prevImage ? prevImage->step : 0),
              "myslam_tracker_set_frame");
    }
    void GetFrame(int stream, StreamState& s) {
        s.features.resize(cap_); s.landmarkOf.resize(cap_); s.landmarkPos.resize((size_t)lmCap_ * 3); s.landmarkIsOutlier.resize(lmCap_);
        s.outlierLandmarks.resize((size_t)2 * cap_);
        int nf = 0, nl = 0, no = 0;
        check(myslam_tracker_get_frame(h_, stream, reinterpret_cast<float*>(s.features.data()), s.landmarkOf.data(), &nf, s.landmarkPos.data(),
                                       s.landmarkIsOutlier.data(), &nl, s.refPose, &s.refFrameId, s.lastRel, s.relMotion, &s.nextFrameId, &s.status, &s.kfEvery,
                                       &s.frozen, s.outlierLandmarks.data(), &no, nullptr, 0), "myslam_tracker_get_frame");
        s.features.resize(nf); s.landmarkOf.resize(nf); s.landmarkPos.resize((size_t)nl * 3); s.landmarkIsOutlier.resize(nl); s.outlierLandmarks.resize(no);
    }
    // device pointers: image s at d_left + s * stride; d_results: streams() records; asynchronous on the handle's stream
    void Step(const uint8_t* d_left, int step, size_t stride, myslam_tracker_result* d_results) {
        check(myslam_tracker_step_batch(h_, d_left, step, stride, d_results), "myslam_tracker_step_batch");
    }
    // ---- key-frame turns on the device (include/myslam_hip.h, "Key-frame turns on the device": every rule and error is stated there) ----
    struct StreamIds {              // MapPoint::mnId by landmark slot, the reference key-frame's mnKFId and the stream's id counters
        std::vector<int64_t> landmarkId; int64_t refKfId = 0, nextKfId = 0, nextMpId = 0; int valid = 0;
    };
    struct TurnOutputs {            // device pointers, the layout myslam_backend_insert_keyframe_batch reads (feature stride cap, outlier stride 2 cap)
        int64_t* newKfId; double* newKfPose; int64_t* featMpId; double* featMpPos; float* featUv; int32_t* featTag; uint8_t* featFlags; int32_t* nFeat;
        int64_t* outlierMpId; int32_t* nOutlierMp; float* rightXy; uint8_t* rightOk; int32_t* report;      // report: streams() x 8
    };
    int keyframeLaunches() const { return myslam_tracker_keyframe_launches(h_); }
    void SetIds(int stream, const StreamIds& ids) {
        check(myslam_tracker_set_ids(h_, stream, ids.landmarkId.data(), (int)ids.landmarkId.size(), ids.refKfId, ids.nextKfId, ids.nextMpId),
              "myslam_tracker_set_ids");
    }
    void GetIds(int stream, StreamIds& ids) {
        ids.landmarkId.resize(lmCap_);
        int n = 0;
        check(myslam_tracker_get_ids(h_, stream, ids.landmarkId.data(), &n, &ids.refKfId, &ids.nextKfId, &ids.nextMpId, &ids.valid), "myslam_tracker_get_ids");
        ids.landmarkId.resize(n);
    }
    // every stream's detection mask in myslam_orb_detect_batch's d_masks layout (all 0 where no turn is due)
    void KeyframeMasks(uint8_t* d_masks, int step, size_t stride) {
        check(myslam_tracker_keyframe_masks(h_, d_masks, step, stride), "myslam_tracker_keyframe_masks");
    }
    // d_right: the right images of the step that froze the streams; d_newKps / d_nNew: what detect_batch found under the masks
    void KeyframeBatch(const uint8_t* d_right, int step, size_t stride, const myslam_keypoint* d_newKps, const int32_t* d_nNew, int kpCap, double baseline,
                       const TurnOutputs& o) {
        check(withOutputs(myslam_tracker_keyframe_batch, o, h_, d_right, step, stride, d_newKps, d_nNew, kpCap, baseline), "myslam_tracker_keyframe_batch");
    }
    // the back end's tables (item s = stream s) after they moved: running streams follow their ids
    void UpdateFromMap(const int64_t* d_kfId, const double* d_kfPose, const int32_t* d_nKf, int kfCap, const int64_t* d_mpId, const double* d_mpPos,
                       const uint8_t* d_mpOutlier, const int32_t* d_nMp, int mpCap) {
        check(myslam_tracker_update_from_map_batch(h_, d_kfId, d_kfPose, d_nKf, kfCap, d_mpId, d_mpPos, d_mpOutlier, d_nMp, mpCap),
              "myslam_tracker_update_from_map_batch");
    }
    // Backend::CulledView's lists (stream s at + s * listCap): a stream whose last frame is its reference key-frame's frame drops the landmark of every
    // listed feature of that key-frame (src/keyframe.cpp:21: the Feature objects are shared); any other stream keeps every byte
    void ClearLinksBatch(const int64_t* d_kfId, const int32_t* d_tag, const int32_t* d_n, int listCap, int32_t* d_nCleared = nullptr) {
        check(myslam_tracker_clear_links_batch(h_, d_kfId, d_tag, d_n, listCap, d_nCleared), "myslam_tracker_clear_links_batch");
    }
    // Relink::View()'s link lists against the map archive of the same streams (MapArchive::handle()): under ClearLinksBatch's guard the landmark of every
    // listed feature of the reference key-frame takes the target's id, position and outlier flag (src/loopclosing.cpp:524, :529), a feature without one
    // gets the slot that carries the id or a new one; status[s] = MYSLAM_OK, or MYSLAM_ERR_INVALID / _CAPACITY with every byte of the stream kept
    void RelinkBatch(const int64_t* d_kfId, const int32_t* d_tag, const int32_t* d_slot, const int32_t* d_n, int listCap, const myslam_map* map,
                     int32_t* d_nRelinked, int32_t* d_status) {
        check(myslam_tracker_relink_batch(h_, d_kfId, d_tag, d_slot, d_n, listCap, map, d_nRelinked, d_status), "myslam_tracker_relink_batch");
    }
    // the stored previous left image of the selected streams <- d_imgs[s] (a key-frame's image after DeepLCD blurred it)
    void SetImageBatch(const uint8_t* d_imgs, int step, size_t stride, const uint8_t* d_select) {
        check(myslam_tracker_set_image_batch(h_, d_imgs, step, stride, d_select), "myslam_tracker_set_image_batch");
    }
    // ---- StereoInit on the device (include/myslam_hip.h, "StereoInit on the device"): masks -> detect_batch on the INIT extractor -> InitBatch ----
    int initLaunches() const { return myslam_tracker_init_launches(h_); }
    // back into the created (init-eligible) state with the given id counters: a restart after LOST, or streams that share an id space
    void ResetStream(int stream, int nextFrameId = 0, int64_t nextKfId = 0, int64_t nextMpId = 0, int kfEvery = 0) {
        check(myslam_tracker_reset_stream(h_, stream, nextFrameId, nextKfId, nextMpId, kfEvery), "myslam_tracker_reset_stream");
    }
    // all 255 for every init-eligible stream, all 0 for the others (KeyframeMasks' layout)
    void InitMasks(uint8_t* d_masks, int step, size_t stride) {
        check(myslam_tracker_init_masks(h_, d_masks, step, stride), "myslam_tracker_init_masks");
    }
    // d_left / d_right: the streams' first stereo pairs; the report's status is 0, MYSLAM_TRACKER_INIT_RETRY, MYSLAM_TRACKER_NO_TURN or an error
    void InitBatch(const uint8_t* d_left, const uint8_t* d_right, int step, size_t stride, const myslam_keypoint* d_newKps, const int32_t* d_nNew, int kpCap,
                   double baseline, int initGood, const TurnOutputs& o) {
        check(withOutputs(myslam_tracker_init_batch, o, h_, d_left, d_right, step, stride, d_newKps, d_nNew, kpCap, baseline, initGood), "myslam_tracker_init_batch");
    }
private:
    // call(lead..., the 13 pointers of o): the order in which myslam_tracker_keyframe_batch and myslam_tracker_init_batch end
    template <class Call, class... Lead>
    static int withOutputs(Call call, const TurnOutputs& o, Lead... lead) {
        return call(lead..., o.newKfId, o.newKfPose, o.featMpId, o.featMpPos, o.featUv, o.featTag, o.featFlags, o.nFeat, o.outlierMpId, o.nOutlierMp, o.rightXy,
                    o.rightOk, o.report);
    }
};

// Camera::UndistortImage (include/myslam/camera.h, src/camera.cpp:36-48): cv::undistort(src, dst, K, distCoef) for one camera at one image
// size, as Frontend::GrabStereoImage calls it on both images when Camera.bNeedUndistortion is 1 (src/frontend.cpp:47-51).  K = fx fy cx cy,
// D = k1 k2 p1 p2.  src and dst may be the same image (the reference's in-place call).
class Camera {
    myslam_undistort* h_ = nullptr;
    int rows_ = 0, cols_ = 0;
public:
    Camera(int rows, int cols, const float K[4], const float D[4]) : rows_(rows), cols_(cols) {
        check(myslam_undistort_create(&h_, rows, cols, K, D), "myslam_undistort_create");
    }
    ~Camera() { if (h_) myslam_undistort_destroy(h_); }
    Camera(const Camera&) = delete; Camera& operator=(const Camera&) = delete;
    int rows() const { return rows_; }
    int cols() const { return cols_; }
    void UndistortImage(const ImageView& src, ImageView& dst) {
        if (src.rows != rows_ || src.cols != cols_ || dst.rows != rows_ || dst.cols != cols_) throw std::runtime_error("Camera::UndistortImage: image size");
        check(myslam_undistort_image(h_, src.data, src.step, dst.data, dst.step), "myslam_undistort_image");
    }
    // OpenCV's CV_16SC2 / CV_16UC1 maps (rows x cols x 2 / rows x cols)
    void GetMap(std::vector<int16_t>& xy, std::vector<uint16_t>& frac) const {
        xy.resize((size_t)rows_ * cols_ * 2); frac.resize((size_t)rows_ * cols_);
        check(myslam_undistort_get_map(h_, xy.data(), frac.data()), "myslam_undistort_get_map");
    }
};

// the g2o stage of Frontend::EstimateCurrentPose (src/frontend.cpp:176-276); returns features.size() - cntOutliers.
// preOptimize = 1 gives LoopClosing::OptimizeCurrentPose (src/loopclosing.cpp:339-433)
inline int EstimateCurrentPose(double pose_qt[7], const std::vector<double>& mapPoints /*n x 3*/, const std::vector<double>& pixels /*n x 2*/,
                               double fx, double fy, double cx, double cy, std::vector<uint8_t>& isOutlier,
                               double chi2_th = 5.991, int numIterations = 4, int optimizeIters = 10, int preOptimize = 0) {
    const int n = (int)(mapPoints.size() / 3);
    isOutlier.assign(n, 0);
    int inl = 0;
    check(myslam_pose_only_optimize(pose_qt, mapPoints.data(), pixels.data(), n, fx, fy, cx, cy, chi2_th, numIterations, optimizeIters,
                                    preOptimize, n ? isOutlier.data() : nullptr, &inl), "myslam_pose_only_optimize");
    return inl;
}

// cv::solvePnPRansac(points3d, points2d, K, cv::Mat(), rvec, tvec, false, 100, 5.991, 0.99) + cv::Rodrigues as
// LoopClosing::ComputeCorrectPose uses them (src/loopclosing.cpp:262-272).  pose7 = (qx qy qz qw tx ty tz) of SE3d(R, t).
// false where OpenCV returns false (fewer than 5 matches, no model) — the reference wraps the call in try / catch and gives up.
struct Point3f { float x, y, z; };
inline bool solvePnPRansac(const std::vector<Point3f>& objectPoints, const std::vector<Point2f>& imagePoints, double fx, double fy, double cx,
                           double cy, double pose7[7], std::vector<uint8_t>* inliers = nullptr, int iterationsCount = 100,
                           float reprojectionError = 5.991f, double confidence = 0.99) {
    if (objectPoints.size() != imagePoints.size()) throw std::runtime_error("solvePnPRansac: size mismatch");
    const int n = (int)objectPoints.size();
    std::vector<uint8_t> mask((size_t)std::max(n, 1));
    int ninl = 0;
    const int rc = myslam_solve_pnp_ransac(reinterpret_cast<const float*>(objectPoints.data()), reinterpret_cast<const float*>(imagePoints.data()), n,
                                           fx, fy, cx, cy, iterationsCount, (double)reprojectionError, confidence, pose7, mask.data(), &ninl);
    if (rc == MYSLAM_ERR_UNSUPPORTED) return false;
    check(rc, "myslam_solve_pnp_ransac");
    if (inliers) { mask.resize(n); *inliers = mask; }
    return true;
}

// The same verification for a batch of loop candidates that already live on the device (myslam_pnp_*): the handle owns the workspace, the calls
// take device pointers (points batch x cap x 3 / pixels batch x cap x 2 float, counts batch), enqueue on the handle's stream and never wait.
// SolveBatch = solvePnPRansac per item (src/loopclosing.cpp:262-272); VerifyBatch = the arithmetic of LoopClosing::ComputeCorrectPose (:208-335):
// PnP, OptimizeCurrentPose over all the item's matches, and the two size gates, status[b] = MYSLAM_VERIFY_*.
class PnPSolver {
    myslam_pnp* h_ = nullptr;
    int maxBatch_, cap_, maxIterations_;
public:
    PnPSolver(int maxBatch, int cap, int maxIterations = 100) : maxBatch_(maxBatch), cap_(cap), maxIterations_(maxIterations) {
        check(myslam_pnp_create(&h_, maxBatch, cap, maxIterations), "myslam_pnp_create");
    }
    ~PnPSolver() { if (h_) myslam_pnp_destroy(h_); }
    PnPSolver(const PnPSolver&) = delete; PnPSolver& operator=(const PnPSolver&) = delete;
    int maxBatch() const { return maxBatch_; }
    int cap() const { return cap_; }
    int maxIterations() const { return maxIterations_; }
    void SetStream(void* hipStream) { check(myslam_pnp_set_stream(h_, hipStream), "myslam_pnp_set_stream"); }
    void SolveBatch(const float* d_points3d, const float* d_points2d, const int32_t* d_counts, int batch, double fx, double fy, double cx, double cy,
                    double* d_pose7, uint8_t* d_inlier, int32_t* d_nInliers, int32_t* d_status, int iterationsCount = 100,
                    double reprojectionError = 5.991, double confidence = 0.99) {
        check(myslam_solve_pnp_ransac_batch(h_, d_points3d, d_points2d, d_counts, batch, fx, fy, cx, cy, iterationsCount, reprojectionError, confidence,
                                            d_pose7, d_inlier, d_nInliers, d_status), "myslam_solve_pnp_ransac_batch");
    }
    // d_pnpPose7 / d_pnpInlier (optional): PnP's own pose and consensus mask
    void VerifyBatch(const float* d_points3d, const float* d_points2d, const int32_t* d_counts, int batch, double fx, double fy, double cx, double cy,
                     double* d_pose7, uint8_t* d_outlier, int32_t* d_nInliers, int32_t* d_status, double* d_pnpPose7 = nullptr,
                     uint8_t* d_pnpInlier = nullptr, int iterationsCount = 100, double reprojectionError = 5.991, double confidence = 0.99,
                     int minMatches = 10, double chi2_th = 5.991, int numIterations = 4, int optimizeIters = 10) {
        check(myslam_loop_verify_batch(h_, d_points3d, d_points2d, d_counts, batch, fx, fy, cx, cy, iterationsCount, reprojectionError, confidence,
                                       minMatches, chi2_th, numIterations, optimizeIters, d_pose7, d_outlier, d_nInliers, d_status, d_pnpPose7, d_pnpInlier),
              "myslam_loop_verify_batch");
    }
};

// LoopClosing::LoopCorrect's arithmetic (src/loopclosing.cpp:437-463) for a batch of maps on the device: the handle owns the workspace of maxBatch maps
// of up to kfCap key-frames, edgeCap edges, activeCap active key-frames and pointCap map points.  CorrectBatch takes the strided tables of
// myslam_loop_correct_batch (include/myslam_hip.h), d_correctedPose7 / d_verifyStatus being PnPSolver::VerifyBatch's d_pose7 / d_status (nullptr = every
// item is confirmed); status[b] = MYSLAM_LOOP_CORRECT_* or a negative error.  Enqueues on the handle's stream and returns.
class LoopCorrector {
    myslam_loop_corrector* h_ = nullptr;
    int maxBatch_, kfCap_, edgeCap_, activeCap_, pointCap_;
public:
    LoopCorrector(int maxBatch, int kfCap, int edgeCap, int activeCap, int pointCap)
        : maxBatch_(maxBatch), kfCap_(kfCap), edgeCap_(edgeCap), activeCap_(activeCap), pointCap_(pointCap) {
        check(myslam_loop_corrector_create(&h_, maxBatch, kfCap, edgeCap, activeCap, pointCap), "myslam_loop_corrector_create");
    }
    ~LoopCorrector() { if (h_) myslam_loop_corrector_destroy(h_); }
    LoopCorrector(const LoopCorrector&) = delete; LoopCorrector& operator=(const LoopCorrector&) = delete;
    int maxBatch() const { return maxBatch_; }
    int kfCap() const { return kfCap_; }
    int edgeCap() const { return edgeCap_; }
    int activeCap() const { return activeCap_; }
    int pointCap() const { return pointCap_; }
    void SetStream(void* hipStream) { check(myslam_loop_corrector_set_stream(h_, hipStream), "myslam_loop_corrector_set_stream"); }
    void CorrectBatch(double* d_poses, const int32_t* d_nKF, const int32_t* d_active, const int32_t* d_nActive, const int32_t* d_cur, const int32_t* d_loop,
                      const double* d_correctedPose7, const int32_t* d_verifyStatus, int32_t* d_edgeV0, int32_t* d_edgeV1, double* d_meas, int32_t* d_nEdges,
                      double* d_points, const int32_t* d_nPoints, const int32_t* d_firstActive, const int32_t* d_firstKF, int batch, double correctThreshold /*1.0, :285*/,
                      int maxIters /*20, :606*/, double* d_chi2, int32_t* d_iters, int32_t* d_status) {
        check(myslam_loop_correct_batch(h_, d_poses, d_nKF, d_active, d_nActive, d_cur, d_loop, d_correctedPose7, d_verifyStatus, d_edgeV0, d_edgeV1, d_meas,
                                        d_nEdges, d_points, d_nPoints, d_firstActive, d_firstKF, batch, correctThreshold, maxIters, d_chi2, d_iters, d_status),
              "myslam_loop_correct_batch");
    }
    // the separator rule of CorrectBatch for one map, on the host: false = the map would come back MYSLAM_LOOP_CORRECT_FUSED_ONLY
    static bool Structure(int nKF, const int32_t* active, int nActive, int loop, const int32_t* edgeV0, const int32_t* edgeV1, int nEdges,
                          int* nSeparators = nullptr, int* chainLength = nullptr) {
        int ok = 0;
        check(myslam_loop_correct_structure(nKF, active, nActive, loop, edgeV0, edgeV1, nEdges, nSeparators, chainLength, &ok), "myslam_loop_correct_structure");
        return ok != 0;
    }
};

// Backend::OptimizeActiveMap (src/backend.cpp:126-266) for a batch of active maps held in device tables: the handle owns the flat windows and the
// solve's workspace of maxBatch maps of up to kfCap active key-frames, mpCap active map points and obsCap observation rows.  OptimizeBatch takes the
// strided tables of myslam_backend_optimize_batch (include/myslam_hip.h) and updates them in place; status[b] = MYSLAM_BACKEND_DONE / _EMPTY or a
// negative error.  Enqueues three launches on the handle's stream and returns; DebugFlat synchronises.
class Backend {
    myslam_backend* h_ = nullptr;
    int maxBatch_, kfCap_, mpCap_, obsCap_;
public:
    myslam_backend* handle() { return h_; }
    Backend(int maxBatch, int kfCap, int mpCap, int obsCap) : maxBatch_(maxBatch), kfCap_(kfCap), mpCap_(mpCap), obsCap_(obsCap) {
        check(myslam_backend_create(&h_, maxBatch, kfCap, mpCap, obsCap), "myslam_backend_create");
    }
    ~Backend() { if (h_) myslam_backend_destroy(h_); }
    Backend(const Backend&) = delete; Backend& operator=(const Backend&) = delete;
    int maxBatch() const { return maxBatch_; }
    int kfCap() const { return kfCap_; }
    int mpCap() const { return mpCap_; }
    int obsCap() const { return obsCap_; }
    void SetStream(void* hipStream) { check(myslam_backend_set_stream(h_, hipStream), "myslam_backend_set_stream"); }
    int LaunchesPerCall() const { return myslam_backend_launches_per_call(h_); }
    // the last optimise's positions by landmark slot and the slot of every input map-point row (device pointers): MapArchive::AttachSolve
    void SolveView(const double** d_points, const int32_t** d_mpSlot) const {
        check(myslam_backend_solve_view(h_, d_points, d_mpSlot), "myslam_backend_solve_view");
    }
    // the features whose edge the last OptimizeBatch removed (src/backend.cpp:236-247): (key-frame id, feature index) per item in input row order,
    // stride obsCap, and their counts; valid until destruction.  LoopKeyFrameStore::ClearLinksBatch / TrackerBank::ClearLinksBatch take them
    void CulledView(const int64_t** d_kfId, const int32_t** d_tag, const int32_t** d_nCulled) const {
        check(myslam_backend_culled_view(h_, d_kfId, d_tag, d_nCulled), "myslam_backend_culled_view");
    }
    void OptimizeBatch(const int64_t* d_kfId, double* d_kfPose, const int32_t* d_nKF, int64_t* d_mpId, double* d_mpPos, uint8_t* d_mpOutlier, int32_t* d_nMP,
                       int32_t* d_obsMP, int32_t* d_obsKF, uint8_t* d_obsFlags, float* d_obsUV, int32_t* d_obsTag, int32_t* d_nObs, int batch, double fx,
                       double fy, double cx, double cy, uint8_t* d_obsReport, uint8_t* d_mpReport, int32_t* d_newOutlierMP, int32_t* d_nNewOutlierMP,
                       double* d_obsChi2, int32_t* d_rounds, int32_t* d_nOutlierEdges, int32_t* d_status, double huberDelta = 5.991 /* :199 */,
                       double chi2Th = 5.991 /* :155 */, int maxRounds = 5 /* :212 */, int itersPerRound = 10 /* :214 */) {
        check(myslam_backend_optimize_batch(h_, d_kfId, d_kfPose, d_nKF, d_mpId, d_mpPos, d_mpOutlier, d_nMP, d_obsMP, d_obsKF, d_obsFlags, d_obsUV, d_obsTag,
                                            d_nObs, batch, fx, fy, cx, cy, huberDelta, chi2Th, maxRounds, itersPerRound, d_obsReport, d_mpReport,
                                            d_newOutlierMP, d_nNewOutlierMP, d_obsChi2, d_rounds, d_nOutlierEdges, d_status),
              "myslam_backend_optimize_batch");
    }
    // Map::InsertKeyFrame (src/map.cpp:17-48, :78-140) per item on the same tables, all in/out (myslam_backend_insert_keyframe_batch): the new
    // key-frame's features as device arrays of featCap rows per item, optionally (nullptr counts = none) the observations a re-entering map point already
    // has and the ids given to Map::AddOutlierMapPoint.  One launch on the handle's stream; status[b] = 0 or a negative error.
    int InsertLaunchesPerCall() const { return myslam_backend_insert_launches_per_call(h_); }
    void InsertKeyFrameBatch(int64_t* d_kfId, double* d_kfPose, int32_t* d_nKF, int64_t* d_mpId, double* d_mpPos, uint8_t* d_mpOutlier, int32_t* d_nMP,
                             int32_t* d_obsMP, int32_t* d_obsKF, uint8_t* d_obsFlags, float* d_obsUV, int32_t* d_obsTag, int32_t* d_nObs,
                             const int64_t* d_newKFId, const double* d_newKFPose, const int64_t* d_featMPId, const double* d_featMPPos,
                             const float* d_featUV, const int32_t* d_featTag, const uint8_t* d_featFlags, const int32_t* d_nFeat, int featCap,
                             const int64_t* d_priorMPId, const int64_t* d_priorKFId, const float* d_priorUV, const int32_t* d_priorTag,
                             const uint8_t* d_priorFlags, const int32_t* d_nPrior, int priorCap, const int64_t* d_outlierMPId,
                             const int32_t* d_nOutlierMP, int outlierCap, int batch, int window /* Map.activeMap.size */, int32_t* d_featRow,
                             int32_t* d_mpNewRow, int64_t* d_removedKFId, int32_t* d_removedKFRow, double* d_dis, int32_t* d_status,
                             double minDisTh = 0.2 /* map.cpp:101 */) {
        check(myslam_backend_insert_keyframe_batch(h_, d_kfId, d_kfPose, d_nKF, d_mpId, d_mpPos, d_mpOutlier, d_nMP, d_obsMP, d_obsKF, d_obsFlags, d_obsUV,
                                                   d_obsTag, d_nObs, d_newKFId, d_newKFPose, d_featMPId, d_featMPPos, d_featUV, d_featTag, d_featFlags,
                                                   d_nFeat, featCap, d_priorMPId, d_priorKFId, d_priorUV, d_priorTag, d_priorFlags, d_nPrior, priorCap,
                                                   d_outlierMPId, d_nOutlierMP, outlierCap, batch, window, minDisTh, d_featRow, d_mpNewRow, d_removedKFId,
                                                   d_removedKFRow, d_dis, d_status),
              "myslam_backend_insert_keyframe_batch");
    }
    // the flat window of one item as the last call built it (host arrays of kfCap / mpCap / obsCap elements, any but sizes3 may be nullptr)
    void DebugFlat(int item, int32_t* poseSrc, int32_t* ptSrc, int32_t* edgePose, int32_t* edgePt, double* edgeObs, int32_t* edgeSrc, uint8_t* fixed,
                   int32_t* sizes3) {
        check(myslam_backend_debug_flat(h_, item, poseSrc, ptSrc, edgePose, edgePt, edgeObs, edgeSrc, fixed, sizes3), "myslam_backend_debug_flat");
    }
    // what the solve left for that window, in slot / edge order
    void DebugSolved(int item, double* poses, double* points, double* edgeChi2, uint8_t* edgeOutlier, int32_t* roundsOutliers2) {
        check(myslam_backend_debug_solved(h_, item, poses, points, edgeChi2, edgeOutlier, roundsOutliers2), "myslam_backend_debug_solved");
    }
};

// Map::mmAllKeyFrames / mmAllMapPoints and KeyFrame::mpLastKF / mRelativePoseToLastKF of maxBatch streams as device tables (myslam_map_*,
// include/myslam_hip.h): UpdateBatch after EVERY Backend call on the same stream keeps them current, and they are laid out as
// LoopCorrector::CorrectBatch's tables (View() gives the device pointers).  Order of a key-frame: InsertKeyFrameBatch -> UpdateBatch(AFTER_INSERT) ->
// OptimizeBatch -> UpdateBatch(AFTER_OPTIMIZE) -> Backend::CulledView's lists into LoopKeyFrameStore::ClearLinksBatch and TrackerBank::ClearLinksBatch
// -> ... -> DetectBatch -> FilterLandmarksBatch -> MatchFeaturesBatch -> ... -> LoopInputsBatch -> CorrectBatch -> WriteBackendBatch ->
// Relink (below: PlanBatch ... ObsUpdateBatch, with RelinkBatch and UpdateBatch(MYSLAM_MAP_AFTER_RELINK) of this class) -> Tracker::UpdateFromMap.
class MapArchive {
    myslam_map* h_ = nullptr;
public:
    MapArchive(int maxBatch, int kfCap, int edgeCap, int pointCap, int backendMpCap) {
        check(myslam_map_create(&h_, maxBatch, kfCap, edgeCap, pointCap, backendMpCap), "myslam_map_create");
    }
    ~MapArchive() { if (h_) myslam_map_destroy(h_); }
    MapArchive(const MapArchive&) = delete; MapArchive& operator=(const MapArchive&) = delete;
    void SetStream(void* hipStream) { check(myslam_map_set_stream(h_, hipStream), "myslam_map_set_stream"); }
    int LaunchesPerUpdate() const { return myslam_map_launches_per_update(h_); }
    // a map point that leaves the active set with an optimise takes the solve's position (src/backend.cpp:259-261 come before src/map.cpp:126-140)
    void AttachSolve(const Backend& be) {
        const double* pts = nullptr; const int32_t* slot = nullptr;
        be.SolveView(&pts, &slot);
        check(myslam_map_attach_solve(h_, pts, slot), "myslam_map_attach_solve");
    }
    myslam_map_tables View() const { myslam_map_tables t; check(myslam_map_view(h_, &t), "myslam_map_view"); return t; }
    // one item from / to host arrays (synchronous); Get's arrays are sized by the caps, any pointer may be nullptr
    void Load(int item, const int64_t* kfId, const double* kfPose, int nKF, const int32_t* edgeV0, const int32_t* edgeV1, const double* meas, int nEdges,
              const int64_t* mpId, const double* mpPos, const int32_t* mpFirstKF, const uint8_t* mpState, int nMP, const int32_t* snapshot = nullptr,
              int nSnapshot = 0, const int32_t* mpGoneKF = nullptr, const uint16_t* mpWinMask = nullptr, const int32_t* winKF = nullptr, int nWin = 0) {
        check(myslam_map_load(h_, item, kfId, kfPose, nKF, edgeV0, edgeV1, meas, nEdges, mpId, mpPos, mpFirstKF, mpState, nMP, snapshot, nSnapshot, mpGoneKF,
                              mpWinMask, winKF, nWin),
              "myslam_map_load");
    }
    void Get(int item, int64_t* kfId, double* kfPose, int* nKF, int32_t* edgeV0, int32_t* edgeV1, double* meas, int* nEdges, int64_t* mpId, double* mpPos,
             int32_t* mpFirstKF, uint8_t* mpState, int* nMP, int32_t* snapshot = nullptr, int* nSnapshot = nullptr,
             int32_t* mpGoneKF = nullptr, uint16_t* mpWinMask = nullptr, int32_t* winKF = nullptr, int* nWin = nullptr) {
        check(myslam_map_get(h_, item, kfId, kfPose, nKF, edgeV0, edgeV1, meas, nEdges, mpId, mpPos, mpFirstKF, mpState, nMP, snapshot, nSnapshot, mpGoneKF,
                             mpWinMask, winKF, nWin),
              "myslam_map_get");
    }
    // mode = MYSLAM_MAP_AFTER_INSERT (d_backendStatus = InsertKeyFrameBatch's status, the turn's outlier ids, d_mpReport unused) or
    // MYSLAM_MAP_AFTER_OPTIMIZE (OptimizeBatch's status and d_mpReport); status[b] = MYSLAM_MAP_UPDATED / _SKIPPED or a negative error
    void UpdateBatch(int mode, const Backend& be, const int64_t* d_kfId, const double* d_kfPose, const int32_t* d_nKF, const int64_t* d_mpId,
                     const double* d_mpPos, const int32_t* d_nMP, const int32_t* d_obsMP, const int32_t* d_obsKF, const uint8_t* d_obsFlags,
                     const int32_t* d_nObs, const int32_t* d_backendStatus, const int64_t* d_outlierMPId, const int32_t* d_nOutlierMP, int outlierCap,
                     const uint8_t* d_mpReport, int batch, int32_t* d_status) {
        check(myslam_map_update_batch(h_, mode, d_kfId, d_kfPose, d_nKF, be.kfCap(), d_mpId, d_mpPos, d_nMP, be.mpCap(), d_obsMP, d_obsKF, d_obsFlags, d_nObs,
                                      be.obsCap(), d_backendStatus, d_outlierMPId, d_nOutlierMP, outlierCap, d_mpReport, batch, d_status),
              "myslam_map_update_batch");
    }
    // LoopCorrector::CorrectBatch's per-loop index inputs (activeCap = that corrector's)
    void LoopInputsBatch(const Backend& be, const int64_t* d_kfId, const int32_t* d_nKF, const int64_t* d_mpId, const int32_t* d_nMP, const int32_t* d_obsMP,
                         const int32_t* d_obsKF, const uint8_t* d_obsFlags, const int32_t* d_nObs, const int64_t* d_curKFId, const uint64_t* d_loopKFId,
                         const int32_t* d_detectStatus, int activeCap, int batch, int32_t* d_active, int32_t* d_nActive, int32_t* d_cur, int32_t* d_loop,
                         int32_t* d_firstActive, int32_t* d_firstKF, int32_t* d_nPoints) {
        check(myslam_map_loop_inputs_batch(h_, d_kfId, d_nKF, be.kfCap(), d_mpId, d_nMP, be.mpCap(), d_obsMP, d_obsKF, d_obsFlags, d_nObs, be.obsCap(),
                                           d_curKFId, d_loopKFId, d_detectStatus, activeCap, batch, d_active, d_nActive, d_cur, d_loop, d_firstActive,
                                           d_firstKF, d_nPoints), "myslam_map_loop_inputs_batch");
    }
    void WriteBackendBatch(const Backend& be, const int64_t* d_kfId, double* d_kfPose, const int32_t* d_nKF, const int64_t* d_mpId, double* d_mpPos,
                           const int32_t* d_nMP, const uint8_t* d_select /*nullptr = all*/, int batch) {
        check(myslam_map_write_backend_batch(h_, d_kfId, d_kfPose, d_nKF, be.kfCap(), d_mpId, d_mpPos, d_nMP, be.mpCap(), d_select, batch),
              "myslam_map_write_backend_batch");
    }
    // map-point id -> archive slot per feature: LoopKeyFrameStore::PutBatch's d_featureLandmark
    void FeatureSlotsBatch(const int64_t* d_featMPId, const int32_t* d_nFeat, int featCap, int batch, int32_t* d_featureLandmark) {
        check(myslam_map_feature_slots_batch(h_, d_featMPId, d_nFeat, featCap, batch, d_featureLandmark), "myslam_map_feature_slots_batch");
    }
    // DetectBatch's d_loopFeatureLandmark before MatchFeaturesBatch: links to points erased since the key-frame was stored become -1 (src/map.cpp:166-175)
    void FilterLandmarksBatch(int32_t* d_featureLandmark, int featCap, int batch, int32_t* d_nDropped = nullptr) {
        check(myslam_map_filter_landmarks_batch(h_, d_featureLandmark, featCap, batch, d_nDropped), "myslam_map_filter_landmarks_batch");
    }
    // Relink::View()'s merge list (stride mergeCap = its outCap) and Relink::PlanBatch's status: the merged points are erased (src/loopclosing.cpp:527)
    void RelinkBatch(const int32_t* d_merge, const int32_t* d_nMerge, int mergeCap, const int32_t* d_planStatus, int batch, int32_t* d_status) {
        check(myslam_map_relink_batch(h_, d_merge, d_nMerge, mergeCap, d_planStatus, batch, d_status), "myslam_map_relink_batch");
    }
    const myslam_map* handle() const { return h_; }
};

// The plan of LoopClosing::LoopLocalFusion's re-linking (src/loopclosing.cpp:509-532) for a batch of corrected loops on the device (myslam_relink_*,
// include/myslam_hip.h, RE-LINK): which map point of the current key-frame is merged into which point of the loop key-frame, which feature adopts a loop
// point, where every archive slot's features end; and the moved observation rows, staged in this handle and carried into the back end's tables and
// the two archives.  `map` is the MapArchive of the same streams and must outlive this object.  Order of one loop: CorrectBatch -> WriteBackendBatch ->
// PlanBatch -> StageBatch -> BackendBatch -> MapArchive::RelinkBatch (View().merge, BackendBatch's status) -> MapArchive::UpdateBatch
// (MYSLAM_MAP_AFTER_RELINK) -> ObsUpdateBatch -> LoopKeyFrameStore::SetLinksBatch (View().row_kf_id / row_tag / row_slot, then View().link_*) and
// TrackerBank::RelinkBatch (View().link_*) -> TrackerBank::UpdateFromMap; FirstKfBatch before the next CorrectBatch.
class Relink {
    myslam_relink* h_ = nullptr;
public:
    Relink(const MapArchive& map, int maxBatch, int outCap, int featCap, int stageCap) {
        check(myslam_relink_create(&h_, map.handle(), maxBatch, outCap, featCap, stageCap), "myslam_relink_create");
    }
    ~Relink() { if (h_) myslam_relink_destroy(h_); }
    Relink(const Relink&) = delete; Relink& operator=(const Relink&) = delete;
    void SetStream(void* hipStream) { check(myslam_relink_set_stream(h_, hipStream), "myslam_relink_set_stream"); }
    int LaunchesPerPlan() const { return myslam_relink_launches_per_plan(h_); }
    // device pointers and caps of the plan's outputs, valid until destruction
    myslam_relink_lists View() const {
        myslam_relink_lists v;
        check(myslam_relink_view(h_, &v), "myslam_relink_view");
        return v;
    }
    // MatchFeaturesBatch's pairs and counts, VerifyBatch's outlier flags, CorrectBatch's status, the current key-frame's feature -> slot table (in/out),
    // the gathered loop table, the current mnKFId; status[b] = MYSLAM_RELINK_DONE / _SKIPPED or MYSLAM_ERR_INVALID
    void PlanBatch(const int32_t* d_validPairs, const int32_t* d_counts, const uint8_t* d_outlier, const int32_t* d_correctStatus,
                   int32_t* d_curFeatureLandmark, const int32_t* d_loopFeatureLandmark, const int64_t* d_curKfId, int batch, int32_t* d_status) {
        check(myslam_loop_relink_plan_batch(h_, d_validPairs, d_counts, d_outlier, d_correctStatus, d_curFeatureLandmark, d_loopFeatureLandmark, d_curKfId,
                                            batch, d_status), "myslam_loop_relink_plan_batch");
    }
    // the rows (src/loopclosing.cpp:521-527): StageBatch -> BackendBatch -> MapArchive::RelinkBatch -> MapArchive::UpdateBatch(MYSLAM_MAP_AFTER_RELINK) ->
    // ObsUpdateBatch; FirstKfBatch gives CorrectBatch's d_firstKF in list order from then on.  The raw handles come from ObsArchive::handle() / Backend::handle()
    void StageBatch(myslam_obs_archive* obs, const int32_t* d_planStatus, int batch, int32_t* d_status) {
        check(myslam_relink_stage_batch(obs, h_, d_planStatus, batch, d_status), "myslam_relink_stage_batch");
    }
    void BackendBatch(myslam_backend* be, int64_t* d_kfId, double* d_kfPose, int32_t* d_nKF, int64_t* d_mpId, double* d_mpPos, uint8_t* d_mpOutlier, int32_t* d_nMP,
                      int32_t* d_obsMP, int32_t* d_obsKF, uint8_t* d_obsFlags, float* d_obsUV, int32_t* d_obsTag, int32_t* d_nObs, const int32_t* d_stageStatus,
                      int batch, int32_t* d_mpNewRow, int32_t* d_status) {
        check(myslam_relink_backend_batch(be, h_, d_kfId, d_kfPose, d_nKF, d_mpId, d_mpPos, d_mpOutlier, d_nMP, d_obsMP, d_obsKF, d_obsFlags, d_obsUV, d_obsTag, d_nObs,
                                          d_stageStatus, batch, d_mpNewRow, d_status), "myslam_relink_backend_batch");
    }
    void ObsUpdateBatch(myslam_obs_archive* obs, const int64_t* d_kfId, const int32_t* d_nKF, const int64_t* d_mpId, const int32_t* d_nMP, const int32_t* d_obsMP,
                        const int32_t* d_obsKF, const uint8_t* d_obsFlags, const float* d_obsUV, const int32_t* d_obsTag, const int32_t* d_nObs, int kfCap, int mpCap,
                        int obsCap, const int32_t* d_backendStatus, const int32_t* d_mapStatus, int batch, int32_t* d_status) {
        check(myslam_relink_obs_update_batch(obs, h_, d_kfId, d_nKF, d_mpId, d_nMP, d_obsMP, d_obsKF, d_obsFlags, d_obsUV, d_obsTag, d_nObs, kfCap, mpCap, obsCap,
                                             d_backendStatus, d_mapStatus, batch, d_status), "myslam_relink_obs_update_batch");
    }
    static void FirstKfBatch(myslam_obs_archive* obs, int batch, int32_t* d_firstKF) {
        check(myslam_relink_first_kf_batch(obs, batch, d_firstKF), "myslam_relink_first_kf_batch");
    }
};

// MapPoint::GetObservations() (src/mappoint.cpp:19-44) of every map point that is alive and not in the back end's table, per stream, on the device
// (myslam_obs_archive_*, include/myslam_hip.h): the source of Backend::InsertKeyFrameBatch's prior rows, so that a map point that comes back is the
// fixed landmark src/backend.cpp:175-177 makes of it.  `map` is the MapArchive of the same streams and must outlive this object.  Order of a key-frame
// on one stream: PriorRowsBatch -> InsertKeyFrameBatch (with those arrays) -> MapArchive::UpdateBatch -> UpdateBatch -> OptimizeBatch ->
// MapArchive::UpdateBatch -> UpdateBatch (with OptimizeBatch's d_obsReport).  Errors of an item are sticky until Load.
class ObsArchive {
    myslam_obs_archive* h_ = nullptr;
public:
    ObsArchive(const MapArchive& map, int maxBatch, int backendObsCap, int rowCap) {
        check(myslam_obs_archive_create(&h_, map.handle(), maxBatch, backendObsCap, rowCap), "myslam_obs_archive_create");
    }
    ~ObsArchive() { if (h_) myslam_obs_archive_destroy(h_); }
    ObsArchive(const ObsArchive&) = delete; ObsArchive& operator=(const ObsArchive&) = delete;
    void SetStream(void* hipStream) { check(myslam_obs_archive_set_stream(h_, hipStream), "myslam_obs_archive_set_stream"); }
    myslam_obs_archive* handle() { return h_; }
    int LaunchesPerUpdate() const { return myslam_obs_archive_launches_per_update(h_); }
    // one item from / to host arrays (synchronous): the live segments (ids ascending) with their rows, and the mirror of the back end's current table
    void Load(int item, const int64_t* segMPId, const int32_t* segCount, int nSeg, const int64_t* rowKFId, const float* rowUV, const int32_t* rowTag,
              const uint8_t* rowFlags, int nRows, const int64_t* tableMPId = nullptr, const int32_t* tableMPRows = nullptr, int nTableMP = 0,
              const int64_t* tableKFId = nullptr, const float* tableUV = nullptr, const int32_t* tableTag = nullptr, const uint8_t* tableFlags = nullptr,
              int nTableRows = 0) {
        check(myslam_obs_archive_load(h_, item, segMPId, segCount, nSeg, rowKFId, rowUV, rowTag, rowFlags, nRows, tableMPId, tableMPRows, nTableMP, tableKFId,
                                      tableUV, tableTag, tableFlags, nTableRows), "myslam_obs_archive_load");
    }
    // seg and row arrays sized rowCap, table arrays by the back end's mpCap / obsCap; any pointer may be nullptr
    void Get(int item, int64_t* segMPId, int32_t* segCount, int* nSeg, int64_t* rowKFId, float* rowUV, int32_t* rowTag, uint8_t* rowFlags, int* nRows,
             int64_t* tableMPId = nullptr, int32_t* tableMPRows = nullptr, int* nTableMP = nullptr, int64_t* tableKFId = nullptr, float* tableUV = nullptr,
             int32_t* tableTag = nullptr, uint8_t* tableFlags = nullptr, int* nTableRows = nullptr, int* rowsInUse = nullptr, int* nReclaims = nullptr,
             int* error = nullptr) {
        check(myslam_obs_archive_get(h_, item, segMPId, segCount, nSeg, rowKFId, rowUV, rowTag, rowFlags, nRows, tableMPId, tableMPRows, nTableMP, tableKFId,
                                     tableUV, tableTag, tableFlags, nTableRows, rowsInUse, nReclaims, error), "myslam_obs_archive_get");
    }
    // after EACH MapArchive::UpdateBatch: the back end's tables as they stand, the back-end call's and the map update's status, and after an optimise
    // its d_obsReport (nullptr after an insert); status[b] = MYSLAM_MAP_UPDATED / _SKIPPED or a negative, sticky error
    void UpdateBatch(int mode, const Backend& be, const int64_t* d_kfId, const int32_t* d_nKF, const int64_t* d_mpId, const int32_t* d_nMP,
                     const int32_t* d_obsMP, const int32_t* d_obsKF, const uint8_t* d_obsFlags, const float* d_obsUV, const int32_t* d_obsTag,
                     const int32_t* d_nObs, const int32_t* d_backendStatus, const int32_t* d_mapStatus, const uint8_t* d_obsReport, int batch,
                     int32_t* d_status) {
        check(myslam_obs_archive_update_batch(h_, mode, d_kfId, nullptr, d_nKF, d_mpId, nullptr, nullptr, d_nMP, d_obsMP, d_obsKF, d_obsFlags, d_obsUV, d_obsTag,
                                              d_nObs, be.kfCap(), be.mpCap(), be.obsCap(), d_backendStatus, d_mapStatus, d_obsReport, batch, d_status),
              "myslam_obs_archive_update_batch");
    }
    // before the insert: the stored rows of every distinct stored point a feature names, ids ascending, in InsertKeyFrameBatch's prior arrays
    void PriorRowsBatch(const Backend& be, const int64_t* d_featMPId, const int32_t* d_nFeat, int featCap, const int64_t* d_mpId, const int32_t* d_nMP,
                        int batch, int64_t* d_priorMPId, int64_t* d_priorKFId, float* d_priorUV, int32_t* d_priorTag, uint8_t* d_priorFlags,
                        int32_t* d_nPrior, int priorCap, int32_t* d_status) {
        check(myslam_obs_archive_prior_rows_batch(h_, d_featMPId, d_nFeat, featCap, d_mpId, d_nMP, be.mpCap(), batch, d_priorMPId, d_priorKFId, d_priorUV,
                                                  d_priorTag, d_priorFlags, d_nPrior, priorCap, d_status), "myslam_obs_archive_prior_rows_batch");
    }
};

// What ProcessNewKF leaves in a KeyFrame (mvPyramidKeyPoints, mORBDescriptors, which features still name a map point), resident on the device for up to
// kfCapacity key-frames of cap rows and featCap features, and LoopClosing::DetectLoop's decision (src/loopclosing.cpp:147, :151) over
// LoopDatabase's batched scan: DetectBatch writes the chosen key-frames' arrays exactly where MatchFeaturesBatch reads its loop side, status[b] =
// MYSLAM_LOOP_DETECT_* or MYSLAM_ERR_INVALID (an id that is not held); a rejected item has nLoop 0 and falls through the later stages.  PutBatch takes
// ProcessNewKFBatch's outputs (ids ascending, on the host); SetLandmarksBatch replaces the landmark tables of key-frames already held.  Every call
// enqueues on the handle's stream and returns; DetectBatch is one launch and can be recorded.
class LoopKeyFrameStore {
    myslam_loop_store* h_ = nullptr;
    int cap_, featCap_;
public:
    LoopKeyFrameStore(int kfCapacity, int cap, int featCap) : cap_(cap), featCap_(featCap) {
        check(myslam_loop_store_create(&h_, kfCapacity, cap, featCap), "myslam_loop_store_create");
    }
    ~LoopKeyFrameStore() { if (h_) myslam_loop_store_destroy(h_); }
    LoopKeyFrameStore(const LoopKeyFrameStore&) = delete; LoopKeyFrameStore& operator=(const LoopKeyFrameStore&) = delete;
    int cap() const { return cap_; }
    int featCap() const { return featCap_; }
    int size() const { return myslam_loop_store_size(h_); }
    int capacity() const { return myslam_loop_store_capacity(h_); }
    void SetStream(void* hipStream) { check(myslam_loop_store_set_stream(h_, hipStream), "myslam_loop_store_set_stream"); }
    void PutBatch(const std::vector<uint64_t>& ids, const KeyPoint* d_pyramidKeyPoints, const uint8_t* d_descriptors, const int32_t* d_counts,
                  const int32_t* d_kfStatus /*may be nullptr*/, const int32_t* d_featureLandmark, const int32_t* d_nFeatures) {
        check(myslam_loop_store_put_batch(h_, ids.data(), (int)ids.size(), d_pyramidKeyPoints, d_descriptors, d_counts, d_kfStatus, d_featureLandmark,
                                          d_nFeatures), "myslam_loop_store_put_batch");
    }
    void SetLandmarksBatch(const std::vector<uint64_t>& ids, const int32_t* d_featureLandmark, const int32_t* d_nFeatures) {
        check(myslam_loop_store_set_landmarks_batch(h_, ids.data(), (int)ids.size(), d_featureLandmark, d_nFeatures), "myslam_loop_store_set_landmarks_batch");
    }
    // Backend::CulledView's lists: the named feature of a key-frame held, or of the pending one (its id per item and its table, both or neither), loses its
    // landmark; ids that are not held are ignored.  One launch, no host bookkeeping: it can be recorded
    void ClearLinksBatch(const int64_t* d_kfId, const int32_t* d_tag, const int32_t* d_n, int listCap, int batch, const int64_t* d_pendingKfId = nullptr,
                         int32_t* d_pendingFeatureLandmark = nullptr, int32_t* d_nCleared = nullptr) {
        check(myslam_loop_store_clear_links_batch(h_, d_kfId, d_tag, d_n, listCap, batch, d_pendingKfId, d_pendingFeatureLandmark, d_nCleared),
              "myslam_loop_store_clear_links_batch");
    }
    // ClearLinksBatch with a value per entry (Relink::View()'s link lists): the named feature points at d_slot (>= -1) afterwards (src/loopclosing.cpp:524, :529)
    void SetLinksBatch(const int64_t* d_kfId, const int32_t* d_tag, const int32_t* d_slot, const int32_t* d_n, int listCap, int batch,
                       const int64_t* d_pendingKfId = nullptr, int32_t* d_pendingFeatureLandmark = nullptr, int32_t* d_nSet = nullptr) {
        check(myslam_loop_store_set_links_batch(h_, d_kfId, d_tag, d_slot, d_n, listCap, batch, d_pendingKfId, d_pendingFeatureLandmark, d_nSet),
              "myslam_loop_store_set_links_batch");
    }
    void DetectBatch(const uint64_t* d_bestId, const float* d_maxScore, const int32_t* d_cntSuspected, int nq, uint8_t* d_loopDescriptors, int32_t* d_nLoop,
                     KeyPoint* d_loopPyramidKeyPoints, int32_t* d_loopFeatureLandmark, int32_t* d_loopSlot, int32_t* d_status, float thrHigh = 0.94f /*:147*/,
                     int maxSuspected = 3 /*:147*/) {
        check(myslam_loop_detect_batch(h_, d_bestId, d_maxScore, d_cntSuspected, nq, thrHigh, maxSuspected, d_loopDescriptors, d_nLoop,
                                       d_loopPyramidKeyPoints, d_loopFeatureLandmark, d_loopSlot, d_status), "myslam_loop_detect_batch");
    }
};

// One LoopKeyFrameStore per stream of a bank, in device memory, with the decisions of LoopClosingRun between the batched units on the device:
// LoopClosing::InsertNewKeyFrame's five-key-frames rule (src/loopclosing.cpp:671-681), DetectLoop's decision and `_mvDatabase.at(bestId)` (:147, :151) by
// the row LoopDatabaseBank::QueryBatch found, `if(!bConfirmedLoopKF) AddToDatabase()` (:73-75) and `_mpLastClosedKF = _mpCurrentKF` (:331).  Device
// pointers, S entries each; every Batch call enqueues on the handle's stream and returns, and can be recorded.  Load / Get / Sizes take host memory and wait.
class LoopKeyFrameStoreBank {
    myslam_loop_bank* h_ = nullptr;
    int streams_, kfsPerStream_, cap_, featCap_;
public:
    struct Stream {                 // one stream in host memory: whole slots, kps n x cap, desc n x cap x 32, featureLandmark n x featCap
        std::vector<uint64_t> ids; std::vector<KeyPoint> kps; std::vector<uint8_t> desc; std::vector<int32_t> rows, featureLandmark, nFeatures;
        int64_t lastClosedKFId = -1;        // _mpLastClosedKF->mnKFId, -1 = nullptr
    };
    LoopKeyFrameStoreBank(int streams, int kfsPerStream, int cap, int featCap) : streams_(streams), kfsPerStream_(kfsPerStream), cap_(cap), featCap_(featCap) {
        check(myslam_loop_bank_create(&h_, streams, kfsPerStream, cap, featCap), "myslam_loop_bank_create");
    }
    ~LoopKeyFrameStoreBank() { if (h_) myslam_loop_bank_destroy(h_); }
    LoopKeyFrameStoreBank(const LoopKeyFrameStoreBank&) = delete; LoopKeyFrameStoreBank& operator=(const LoopKeyFrameStoreBank&) = delete;
    int streams() const { return streams_; }
    int kfsPerStream() const { return kfsPerStream_; }
    int cap() const { return cap_; }
    int featCap() const { return featCap_; }
    static int launchesPerFinish() { return myslam_loop_bank_launches_per_finish(); }
    void SetStream(void* hipStream) { check(myslam_loop_bank_set_stream(h_, hipStream), "myslam_loop_bank_set_stream"); }
    myslam_loop_bank_arrays View() const { myslam_loop_bank_arrays v; check(myslam_loop_bank_view(h_, &v), "myslam_loop_bank_view"); return v; }
    // status[s] = MYSLAM_LOOP_BANK_TURN / _SKIPPED / _IDLE; d_itemStatus (Mapper's d_status, stride MYSLAM_MAPPER_STATUS_WORDS) may be nullptr
    void GateBatch(const int64_t* d_newKFId, const int32_t* d_itemStatus, int statusStride, int32_t* d_active, int32_t* d_status) {
        check(myslam_loop_bank_gate_batch(h_, d_newKFId, d_itemStatus, statusStride, d_active, d_status), "myslam_loop_bank_gate_batch");
    }
    void DetectBatch(const uint64_t* d_bestId, const int32_t* d_bestRow, const float* d_maxScore, const int32_t* d_cntSuspected, uint8_t* d_loopDescriptors,
                     int32_t* d_nLoop, KeyPoint* d_loopPyramidKeyPoints, int32_t* d_loopFeatureLandmark, int32_t* d_loopSlot, int32_t* d_status,
                     float thrHigh = 0.94f /*:147*/, int maxSuspected = 3 /*:147*/) {
        check(myslam_loop_bank_detect_batch(h_, d_bestId, d_bestRow, d_maxScore, d_cntSuspected, thrHigh, maxSuspected, d_loopDescriptors, d_nLoop,
                                            d_loopPyramidKeyPoints, d_loopFeatureLandmark, d_loopSlot, d_status), "myslam_loop_bank_detect_batch");
    }
    // status[s] = MYSLAM_LOOP_BANK_IDLE / _CLOSED / _STORED / MYSLAM_ERR_CAPACITY / MYSLAM_ERR_INVALID; d_add is LoopDatabaseBank::AppendBatch's
    void FinishBatch(const uint64_t* d_curKFId, const int32_t* d_active, const int32_t* d_verifyStatus, const KeyPoint* d_pyramidKeyPoints,
                     const uint8_t* d_descriptors, const int32_t* d_counts, const int32_t* d_kfStatus /*may be nullptr*/, const int32_t* d_featureLandmark,
                     const int32_t* d_nFeatures, int32_t* d_add, int32_t* d_status) {
        check(myslam_loop_bank_finish_batch(h_, d_curKFId, d_active, d_verifyStatus, d_pyramidKeyPoints, d_descriptors, d_counts, d_kfStatus,
                                            d_featureLandmark, d_nFeatures, d_add, d_status), "myslam_loop_bank_finish_batch");
    }
    // LoopKeyFrameStore::SetLinksBatch per stream (d_value nullptr: ClearLinksBatch); item s names key-frames of stream s only
    void SetLinksBatch(const int64_t* d_kfId, const int32_t* d_tag, const int32_t* d_value, const int32_t* d_n, int listCap,
                       const int64_t* d_pendingKfId = nullptr, int32_t* d_pendingFeatureLandmark = nullptr, int32_t* d_nSet = nullptr) {
        check(myslam_loop_bank_links_batch(h_, d_kfId, d_tag, d_value, d_n, listCap, d_pendingKfId, d_pendingFeatureLandmark, d_nSet),
              "myslam_loop_bank_links_batch");
    }
    void ClearBatch(const int32_t* d_reset) { check(myslam_loop_bank_clear_batch(h_, d_reset), "myslam_loop_bank_clear_batch"); }
    void Load(int stream, const Stream& s) {
        const size_t n = s.ids.size();
        if (s.kps.size() != n * cap_ || s.desc.size() != n * cap_ * 32 || s.rows.size() != n || s.featureLandmark.size() != n * featCap_ || s.nFeatures.size() != n)
            throw std::runtime_error("LoopKeyFrameStoreBank::Load: the arrays do not hold ids.size() whole slots");
        check(myslam_loop_bank_load(h_, stream, s.ids.data(), s.kps.data(), s.desc.data(), s.rows.data(), s.featureLandmark.data(), s.nFeatures.data(), (int)n,
                                    s.lastClosedKFId), "myslam_loop_bank_load");
    }
    Stream Get(int stream) {
        Stream s;
        const size_t K = kfsPerStream_;
        s.ids.assign(K, 0); s.kps.assign(K * cap_, KeyPoint{}); s.desc.assign(K * cap_ * 32, 0); s.rows.assign(K, 0); s.featureLandmark.assign(K * featCap_, 0);
        s.nFeatures.assign(K, 0);
        int n = 0;
        check(myslam_loop_bank_get(h_, stream, s.ids.data(), s.kps.data(), s.desc.data(), s.rows.data(), s.featureLandmark.data(), s.nFeatures.data(),
                                   kfsPerStream_, &n, &s.lastClosedKFId), "myslam_loop_bank_get");
        s.ids.resize(n); s.kps.resize((size_t)n * cap_); s.desc.resize((size_t)n * cap_ * 32); s.rows.resize(n); s.featureLandmark.resize((size_t)n * featCap_);
        s.nFeatures.resize(n);
        return s;
    }
    std::vector<int32_t> Sizes() {
        std::vector<int32_t> n(streams_);
        check(myslam_loop_bank_sizes(h_, n.data()), "myslam_loop_bank_sizes");
        return n;
    }
};

// The Backend thread for a bank of streams (src/backend.cpp:30-37, :82-121, :126-266 with Map::InsertKeyFrame, src/map.cpp:17-48): one enqueue maps
// exactly the streams that made a key-frame in the turn or the StereoInit whose outputs it is given; the others keep every byte.  The handle owns the
// back end, the map archive, the observation archive and every table between them (View()).  Device pointers; KeyFrameBatch enqueues on the
// handle's stream and returns, and can be recorded.  ResetItem / Status take host memory and wait.
class Mapper {
    myslam_mapper* h_ = nullptr;
    int streams_;
public:
    struct TurnOutputs {            // what myslam_tracker_keyframe_batch / _init_batch wrote (feature stride = featCap, outlier stride = 2 featCap)
        const int64_t* newKFId; const double* newKFPose; const int64_t* featMapPointId; const double* featMapPointPos; const float* featPixels;
        const int32_t* featTag; const uint8_t* featFlags; const int32_t* nFeat; const int64_t* outlierMapPointId; const int32_t* nOutlierMapPoint;
        const float* rightPixels; const uint8_t* rightOk; const int32_t* report;
    };
    Mapper(int streams, int kfCap, int mpCap, int obsCap, int featCap, int archiveKFCap, int archiveEdgeCap, int archivePointCap, int obsRowCap,
           int priorCap) : streams_(streams) {
        check(myslam_mapper_create(&h_, streams, kfCap, mpCap, obsCap, featCap, archiveKFCap, archiveEdgeCap, archivePointCap, obsRowCap, priorCap),
              "myslam_mapper_create");
    }
    ~Mapper() { if (h_) myslam_mapper_destroy(h_); }
    Mapper(const Mapper&) = delete; Mapper& operator=(const Mapper&) = delete;
    int streams() const { return streams_; }
    int launchesPerCall(bool withTracker = true) const { return myslam_mapper_launches_per_call(h_, withTracker ? 1 : 0); }
    void SetStream(void* hipStream) { check(myslam_mapper_set_stream(h_, hipStream), "myslam_mapper_set_stream"); }
    myslam_mapper_tables View() const {
        myslam_mapper_tables t;
        check(myslam_mapper_view(h_, &t), "myslam_mapper_view");
        return t;
    }
    // d_status: streams x MYSLAM_MAPPER_STATUS_WORDS; [0] = 0 mapped / MYSLAM_MAPPER_IDLE / the stream's (sticky) error.  tracker may be nullptr
    void KeyFrameBatch(TrackerBank* tracker, const TurnOutputs& o, int window, double fx, double fy, double cx, double cy, int32_t* d_status,
                       double minDisTh = 0.2, double huberDelta = 5.991, double chi2Th = 5.991, int maxRounds = 5, int itersPerRound = 10) {
        check(myslam_mapper_keyframe_batch(h_, tracker ? tracker->handle() : nullptr, o.newKFId, o.newKFPose, o.featMapPointId, o.featMapPointPos, o.featPixels,
                                           o.featTag, o.featFlags, o.nFeat, o.outlierMapPointId, o.nOutlierMapPoint, o.rightPixels, o.rightOk, o.report, window,
                                           minDisTh, fx, fy, cx, cy, huberDelta, chi2Th, maxRounds, itersPerRound, d_status),
              "myslam_mapper_keyframe_batch");
    }
    void ResetItem(int stream) { check(myslam_mapper_reset_item(h_, stream), "myslam_mapper_reset_item"); }
    std::vector<int32_t> Status(const int32_t* d_status) const {
        std::vector<int32_t> w((size_t)streams_ * MYSLAM_MAPPER_STATUS_WORDS);
        check(myslam_debug_peek(d_status, w.data(), w.size() * sizeof(int32_t)), "myslam_debug_peek");
        return w;
    }
};

// The ORB half of LoopClosing::ProcessNewKF (src/loopclosing.cpp:93-113) for a batch of key-frames whose images and feature pixels live on the device:
// every feature expanded over the extractor's levels, ScreenAndComputeKPsParams, CalcDescriptors.  Writes mvPyramidKeyPoints (batch x cap),
// mORBDescriptors (batch x cap x 32) and their counts exactly where MatchFeaturesBatch reads them; status[b] = MYSLAM_OK or MYSLAM_ERR_CAPACITY.  The
// key-frame's image is the one DeepLCD::calcDescrOriginalImg blurred in place: enqueue that call first, on the extractor's stream.  Enqueues and returns.
inline void ProcessNewKFBatch(ORBextractor& extractor, const uint8_t* d_images, int batch, int rows, int cols, int step, size_t imageStride,
                              const float* d_featurePixels, const int32_t* d_nFeatures, int featCap, KeyPoint* d_pyramidKeyPoints,
                              uint8_t* d_descriptors, int32_t* d_counts, int32_t* d_status, int cap) {
    check(myslam_orb_process_keyframes_batch(extractor.handle(), d_images, batch, rows, cols, step, imageStride, d_featurePixels, d_nFeatures, featCap,
                                             d_pyramidKeyPoints, d_descriptors, d_counts, d_status, cap),
          "myslam_orb_process_keyframes_batch");
}

// LoopClosing::MatchFeatures (src/loopclosing.cpp:167-203) and the gather of ComputeCorrectPose (:210-253) for a batch of candidates whose key-frames
// live on the device: descriptors and mvPyramidKeyPoints of the loop and current key-frames (batch x cap), the current features' pixels and the loop
// features' landmark slots (batch x featCap, -1 = no map point), the landmark positions (landmarkStride 0 = one table for all items).  Writes the
// matcher's output, _msetValidFeatureMatches in the std::set's order, and vLoopPoints3d / vCurrentPoints2d / their count exactly where
// PnPSolver::VerifyBatch reads them (outCap = that solver's cap); status[b] = MYSLAM_LOOP_MATCH_* or a negative error.  Enqueues and returns.
inline void MatchFeaturesBatch(const uint8_t* d_loopDescriptors, const int32_t* d_nLoop, const uint8_t* d_currentDescriptors, const int32_t* d_nCurrent,
                               const KeyPoint* d_loopPyramidKeyPoints, const KeyPoint* d_currentPyramidKeyPoints, int batch, int cap,
                               const float* d_currentFeaturePixels, const int32_t* d_loopFeatureLandmark, int featCap, const double* d_landmarkPos,
                               size_t landmarkStride, int landmarkCap, int outCap, int32_t* d_trainIdx, int32_t* d_distance, int32_t* d_pairs,
                               int32_t* d_nPairs, int32_t* d_validPairs, float* d_points3d, float* d_points2d, int32_t* d_counts, int32_t* d_status,
                               void* hipStream = nullptr, int minMatches = 10) {
    check(myslam_loop_match_batch(d_loopDescriptors, d_nLoop, d_currentDescriptors, d_nCurrent, d_loopPyramidKeyPoints, d_currentPyramidKeyPoints, batch,
                                  cap, d_currentFeaturePixels, d_loopFeatureLandmark, featCap, d_landmarkPos, landmarkStride, landmarkCap, minMatches,
                                  outCap, d_trainIdx, d_distance, d_pairs, d_nPairs, d_validPairs, d_points3d, d_points2d, d_counts, d_status, hipStream),
          "myslam_loop_match_batch");
}

}  // namespace myslam
