// tracker.hip — Frontend::Track() (src/frontend.cpp:86-122) for S independent camera streams per call, all tracker state in device memory:
// constant-velocity prediction and the LK start points (:90-93, :136-147), TrackLastFrame's feature hand-over (:156-170), the inputs of
// EstimateCurrentPose (:183-205), its outlier bookkeeping (:261-270), the GOOD / BAD / LOST decision (:97-110), the relative motion (:122) and
// the key-frame rule (:112).  LK and the pose-only optimisation are the kernels of lk.hip / ba.hip (frontend_launch.h); everything between them
// is here, so that a step never returns to the host.  See include/myslam_hip.h for the rules.
//
// One step = head (image copy into the stream's free buffer + rule 1) -> pyramid levels -> LK -> compaction -> pose-only -> tail.
// The SE3 arithmetic restates chain.py / host/myslam_system.hpp operation by operation with explicitly rounded f64 products and sums:
// the LK start points are rounded to float, and one ulp there moves a converged track by up to 5e-3 px.
#include <algorithm>
#include <vector>

#include "dev_tables.h"
#include "backend_launch.h"
#include "frontend_launch.h"
#include "se3_chain.h"
#include "tri_solve.h"

namespace myslam_hip {

constexpr int TRK_NT = 256;                 // threads of the per-stream blocks
constexpr int TRK_COPY_ROWS = 4;            // image rows one copy block of the head kernel moves
enum { TRK_INITING = 0, TRK_GOOD = 1, TRK_BAD = 2, TRK_LOST = 3 };
enum { TRK_WHY_NONE = 0, TRK_WHY_KEYFRAME = 1, TRK_WHY_LOST = 2, TRK_WHY_CAPACITY = 3 };      // why the last step froze the stream
enum { KF_GO = 0, KF_NO_TURN = 1, KF_CAPACITY = 2 };                        // the turn's head tells its tail
constexpr int MASK_ROWS = 8;                // mask rows one block of k_kf_masks holds in LDS

struct TrkState {
    double ref_pose[7];
    double last_rel[16], rel_motion[16];
    int32_t ref_frame_id, next_frame_id, status, frozen, kf_every;
    int32_t n_feat, n_lm, n_outl;
    int32_t slot;                           // which of the two (image, pyramid) buffers holds the stream's previous image
    int32_t overflow;                       // set_frame did not fit: the next step reports it
    int32_t why;                            // TRK_WHY_*: written by the step that froze the stream, cleared by set_frame and by a turn
    int32_t idsValid;                       // set_ids since the last set_frame (a turn keeps it)
};
static_assert(sizeof(TrkState) == 7 * 8 + 2 * 16 * 8 + 12 * 4, "TrkState");


struct TrkArgs {
    TrkState* st; int S, cap, lmCap, rows, cols;
    double fx, fy, cx, cy; int good, bad;
    // state tables
    float* xy; int32_t* lm;                 // S x cap (x 2)
    double* lmPos; uint8_t* lmOutl;         // S x lmCap (x 3)
    int32_t* outlList;                      // S x 2 cap
    // images
    const uint8_t* left; int step; size_t stride; uint8_t* img; size_t imgBytes, imgSel;
    // step scratch
    int32_t* sel; int32_t* counts;          // S
    float* p0; float* p1; float* nxt; uint8_t* lkSt;          // S x cap
    float* curXy; int32_t* curLm; int32_t* curPo; int32_t* curN;
    double* poPose; double* poPts; double* poObs; int32_t* poCounts; uint8_t* poOutl; int32_t* poInl; int32_t* poStatus;
    myslam_tracker_result* res;
    // ids (MapPoint::mnId by landmark slot; ref_kf_id, next_kf_id, next_mp_id per stream)
    int64_t* lmId; int64_t* ids;            // S x lmCap; S x 3
    // key-frame turn scratch (its own: myslam_tracker_debug_last_step keeps reading the last STEP's)
    int32_t* kfSel; int32_t* kfCounts; int32_t* kfCode;       // S
    float* kfP0; float* kfNxt; uint8_t* kfSt;                 // S x cap: left pixels, right start points -> right points, LK status
    double* kfXyz; uint8_t* kfTok; int32_t* kfSlot;           // S x cap: triangulation (camera frame), its ok, the slot a feature opens or -1
    int32_t* kfFirst; int32_t* kfMap;                         // S x lmCap: first referencing feature, old slot -> new slot
    double* kfPos; uint8_t* kfOutl; int64_t* kfId;            // S x lmCap: the rebuilt landmark table before it is committed
};

// ordered positions among a stream's features, TRK_NT at a time, come from dev_tables.h's block_rank<TRK_NW> (its contract is stated there)
constexpr int TRK_NW = TRK_NT / WAVE;
// ---- the pieces the step, the key-frame turn and StereoInit are built from: each rule below has this one definition ----
// stream s's image buffer `slot` (rows packed at `cols` bytes; every buffer starts on a 256-byte boundary)
__device__ __forceinline__ uint8_t* trk_image(const TrkArgs& a, int s, int slot) { return a.img + (size_t)slot * a.imgSel + (size_t)s * a.imgBytes; }

// copy block `band` (blockIdx.x - 1 in trk_copy_grid) moves its TRK_COPY_ROWS rows of one stream's image: 4-byte words when the widths and THIS source's base allow it
__device__ __forceinline__ void copy_image_rows(const TrkArgs& a, int band, const uint8_t* src, int step, uint8_t* dst) {
    const int t = threadIdx.x, r0 = band * TRK_COPY_ROWS, r1 = min(r0 + TRK_COPY_ROWS, a.rows);
    if (((a.cols | step) & 3) == 0 && (((size_t)src) & 3) == 0) {
        const int w4 = a.cols >> 2;
        for (int r = r0; r < r1; r++) {
            const uint32_t* sp = reinterpret_cast<const uint32_t*>(src + (size_t)r * step);
            uint32_t* dp = reinterpret_cast<uint32_t*>(dst + (size_t)r * a.cols);
            for (int x = t; x < w4; x += TRK_NT) dp[x] = sp[x];
        }
    } else {
        for (int r = r0; r < r1; r++)
            for (int x = t; x < a.cols; x += TRK_NT) dst[(size_t)r * a.cols + x] = src[(size_t)r * step + x];
    }
}

// Tcw = rel * T(ref pose), one thread.  (The step forms this product around its own T(ref pose): its tail needs that again, its head 28 VGPRs more here)
__device__ __forceinline__ void tcw_of(const double* rel, const double* ref_pose, double* Tcw) {
    double Tref[16];
    se3_T_of(ref_pose, Tref); se3_mm(rel, Tref, Tcw);
}

// q = mv(R, p) + t of the 4 x 4 T: a landmark into the camera frame, a triangulated point into the world
__device__ __forceinline__ void se3_apply(const double* T, const double* p, double* q) {
    for (int r = 0; r < 3; r++) q[r] = dadd(dadd(dadd(dmul(T[4 * r], p[0]), dmul(T[4 * r + 1], p[1])), dmul(T[4 * r + 2], p[2])), T[4 * r + 3]);
}
// camera2pixel, rounded to the float LK starts from: (fx pc.x / pc.z + cx, fy pc.y / pc.z + cy).  A right camera shifts pc first (k_kf_head)
__device__ __forceinline__ void pixel_of(const TrkArgs& a, const double* pc, float& u, float& v) {
    u = __double2float_rn(dadd(ddiv(dmul(a.fx, pc[0]), pc[2]), a.cx));
    v = __double2float_rn(dadd(ddiv(dmul(a.fy, pc[1]), pc[2]), a.cy));
}

// ---- head: blockIdx.x == 0 predicts (rule 1) for stream blockIdx.y; the other blocks copy the stream's new image into its free buffer ----
__global__ __launch_bounds__(TRK_NT) void k_trk_head(TrkArgs a) {
    const int s = blockIdx.y, t = threadIdx.x;
    const TrkState& st = a.st[s];
    const bool idle = st.frozen != 0;
    if (blockIdx.x > 0) {
        if (!idle && !st.overflow) copy_image_rows(a, blockIdx.x - 1, a.left + (size_t)s * a.stride, a.step, trk_image(a, s, 1 - st.slot));
        return;
    }
    if (idle) {
        if (t == 0) { a.sel[s] = -1; a.counts[s] = 0; a.poCounts[s] = 0; }
        return;
    }
    if (st.overflow) {                       // set_frame did not fit: say so once, freeze
        if (t == 0) {
            myslam_tracker_result r;
            for (int k = 0; k < 7; k++) r.pose7[k] = st.ref_pose[k];
            r.n_inliers = 0; r.n_features = 0; r.status = MYSLAM_ERR_CAPACITY; r.frame_id = st.next_frame_id; r.needs_host = 1; r.reserved = 0;
            a.res[s] = r;
            a.sel[s] = -1; a.counts[s] = 0; a.poCounts[s] = 0;
            a.st[s].frozen = 1; a.st[s].why = TRK_WHY_CAPACITY;
        }
        return;
    }
    __shared__ double sT[16];
    if (t == 0) {
        double Tref[16], rel[16], p7[7];
        se3_T_of(st.ref_pose, Tref);
        se3_mm(st.rel_motion, st.last_rel, rel);         // cur.rel = rel_motion * last.rel
        se3_mm(rel, Tref, sT);                           // Tcw
        se3_p7_of(sT, p7);
        for (int k = 0; k < 7; k++) a.poPose[(size_t)s * 7 + k] = p7[k];
        a.sel[s] = 1 - st.slot; a.counts[s] = st.n_feat;
    }
    __syncthreads();
    const int n = st.n_feat;
    const size_t fb = (size_t)s * a.cap;
    const double* pos = a.lmPos + (size_t)s * a.lmCap * 3;
    const uint8_t* outl = a.lmOutl + (size_t)s * a.lmCap;
    for (int i = t; i < n; i += TRK_NT) {
        const float x = a.xy[(fb + i) * 2], y = a.xy[(fb + i) * 2 + 1];
        float u = x, v = y;
        const int l = a.lm[fb + i];
        if (l >= 0 && !outl[l]) {                         // world2pixel of the left camera
            double pc[3];
            se3_apply(sT, pos + 3 * l, pc);
            pixel_of(a, pc, u, v);
        }
        a.p0[(fb + i) * 2] = x; a.p0[(fb + i) * 2 + 1] = y;
        a.p1[(fb + i) * 2] = u; a.p1[(fb + i) * 2 + 1] = v;
        a.nxt[(fb + i) * 2] = u; a.nxt[(fb + i) * 2 + 1] = v;
    }
}

// ---- rule 3: one block per stream, ballot + prefix per 256 features, order kept ----
__global__ __launch_bounds__(TRK_NT) void k_trk_compact(TrkArgs a) {
    __shared__ int s_w[TRK_NW];
    const int s = blockIdx.x, t = threadIdx.x;
    if (a.sel[s] < 0) return;
    const int n = a.counts[s];
    const size_t fb = (size_t)s * a.cap;
    const double* pos = a.lmPos + (size_t)s * a.lmCap * 3;
    const uint8_t* outl = a.lmOutl + (size_t)s * a.lmCap;
    int nKeep = 0, nPo = 0;
    for (int base = 0; base < n; base += TRK_NT) {
        const int i = base + t;
        int l = -1; bool keep = false, po = false;
        if (i < n) {
            l = a.lm[fb + i];
            keep = a.lkSt[fb + i] != 0 && l >= 0;
            po = keep && !outl[l];
        }
        int tk, tp;
        const int rk = block_rank<TRK_NW>(keep, s_w, tk), rp = block_rank<TRK_NW>(po, s_w, tp);
        if (keep) {
            const int j = nKeep + rk;
            const float x = a.nxt[(fb + i) * 2], y = a.nxt[(fb + i) * 2 + 1];
            a.curXy[(fb + j) * 2] = x; a.curXy[(fb + j) * 2 + 1] = y;
            a.curLm[fb + j] = l;
            a.curPo[fb + j] = po ? nPo + rp : -1;
            if (po) {
                const int k = nPo + rp;
                a.poPts[(fb + k) * 3] = pos[3 * l]; a.poPts[(fb + k) * 3 + 1] = pos[3 * l + 1]; a.poPts[(fb + k) * 3 + 2] = pos[3 * l + 2];
                a.poObs[(fb + k) * 2] = (double)x; a.poObs[(fb + k) * 2 + 1] = (double)y;
            }
        }
        nKeep += tk; nPo += tp;
    }
    if (t == 0) { a.curN[s] = nKeep; a.poCounts[s] = nPo; }
}

// ---- rules 5 + 6: one block per stream ----
__global__ __launch_bounds__(TRK_NT) void k_trk_tail(TrkArgs a) {
    __shared__ int s_w[TRK_NW];
    const int s = blockIdx.x, t = threadIdx.x;
    if (a.sel[s] < 0) return;
    TrkState& st = a.st[s];
    const int m = a.curN[s], id = st.next_frame_id;
    const bool fresh = id - st.ref_frame_id <= 2;        // a map point that fails right after its creation leaves the map (:264-268)
    const size_t fb = (size_t)s * a.cap;
    uint8_t* lmOutl = a.lmOutl + (size_t)s * a.lmCap;
    int32_t* list = a.outlList + (size_t)s * 2 * a.cap;
    const int listCap = 2 * a.cap;
    int nList = st.n_outl;
    bool listFull = false;
    for (int base = 0; base < m; base += TRK_NT) {
        const int j = base + t;
        int l = -1; bool o = false;
        if (j < m) {
            l = a.curLm[fb + j];
            const int k = a.curPo[fb + j];
            o = k >= 0 && a.poOutl[fb + k] != 0;
        }
        int tot;
        const int r = block_rank<TRK_NW>(o && fresh, s_w, tot);
        if (o && fresh) {
            lmOutl[l] = 1;
            if (nList + r < listCap) list[nList + r] = l;
        }
        if (nList + tot > listCap) listFull = true;
        nList = min(nList + tot, listCap);
        if (j < m) {
            a.xy[(fb + j) * 2] = a.curXy[(fb + j) * 2]; a.xy[(fb + j) * 2 + 1] = a.curXy[(fb + j) * 2 + 1];
            a.lm[fb + j] = o ? -1 : l;
        }
    }
    if (t != 0) return;
    double Tp[16], Tref[16], Tri[16], rel[16], Li[16], Tcw[16];
    myslam_tracker_result r;
    se3_T_of(a.poPose + (size_t)s * 7, Tp);
    se3_T_of(st.ref_pose, Tref);
    se3_inv(Tref, Tri);
    se3_mm(Tp, Tri, rel);                                // cur.rel = T(pose) * T(ref)^-1
    se3_inv(st.last_rel, Li);
    se3_mm(rel, Li, st.rel_motion);                      // rel_motion = cur.rel * last.rel^-1
    for (int k = 0; k < 16; k++) st.last_rel[k] = rel[k];
    se3_mm(rel, Tref, Tcw);
    se3_p7_of(Tcw, r.pose7);
    const int ninl = a.poInl[s];
    int status = ninl > a.good ? TRK_GOOD : (ninl > a.bad ? TRK_BAD : TRK_LOST);
    const bool insert = st.kf_every <= 0 ? status == TRK_BAD : (status != TRK_LOST && id % st.kf_every == 0);
    int needs = (insert || status == TRK_LOST) ? 1 : 0;
    st.status = status;
    if (a.poStatus[s] != MYSLAM_OK || listFull) { status = MYSLAM_ERR_CAPACITY; needs = 1; }
    r.n_inliers = ninl; r.n_features = m; r.status = status; r.frame_id = id; r.needs_host = needs; r.reserved = 0;
    a.res[s] = r;
    st.n_feat = m; st.n_outl = nList; st.next_frame_id = id + 1; st.slot = 1 - st.slot; st.frozen = needs;
    st.why = !needs ? TRK_WHY_NONE : (status == MYSLAM_ERR_CAPACITY ? TRK_WHY_CAPACITY : (status == TRK_LOST ? TRK_WHY_LOST : TRK_WHY_KEYFRAME));
}

// =====================================================================================================================================
// The key-frame turn (include/myslam_hip.h, myslam_tracker_keyframe_*): Frontend::DetectFeatures' mask (:305-309), FindFeaturesInRight
// (:335-379), TriangulateNewPoints (:451-488) and the pose lines of InsertKeyFrame (:422-446) for every ELIGIBLE stream, on the state above.
struct KfArgs {
    const uint8_t* right; int step; size_t stride;
    const myslam_keypoint* newKps; const int32_t* nNew; int kpCap; double baseline;
    int64_t* newKfId; double* newKfPose; int64_t* featMpId; double* featMpPos; float* featUv; int32_t* featTag; uint8_t* featFlags; int32_t* nFeat;
    int64_t* outlMpId; int32_t* nOutlMp; float* rightXy; uint8_t* rightOk; int32_t* report;
};

__device__ __forceinline__ bool kf_eligible(const TrkState& st) { return st.frozen != 0 && st.why == TRK_WHY_KEYFRAME && st.idsValid != 0; }

// cvRound(float) = rint, ties to even; saturates far outside the image, where the clip below gives the same rectangle
__device__ __forceinline__ int cv_round(float v) { return __float2int_rn(v); }

// block blockIdx.x of a mask kernel owns rows [r0, r1) of stream blockIdx.y's mask; returns the band's byte count
__device__ __forceinline__ int mask_band(const TrkArgs& a, int& r0, int& r1) { r0 = blockIdx.x * MASK_ROWS; r1 = min(r0 + MASK_ROWS, a.rows); return (r1 - r0) * a.cols; }
// the band's nb bytes (row-major, `cols` wide) into the stream's mask: band[k], or `fill` everywhere when there is no band
__device__ __forceinline__ void store_mask_band(const TrkArgs& a, uint8_t* masks, int step, size_t stride, int r0, int nb, const uint8_t* band, uint8_t fill) {
    uint8_t* dst = masks + (size_t)blockIdx.y * stride;
    for (int k = threadIdx.x; k < nb; k += TRK_NT) dst[(size_t)(r0 + k / a.cols) * step + k % a.cols] = band ? band[k] : fill;
}

// ---- masks: block (x, s) holds MASK_ROWS rows of stream s's mask in LDS: 255, then 0 under every rectangle, then one coalesced store ----
__global__ __launch_bounds__(TRK_NT) void k_kf_masks(TrkArgs a, uint8_t* masks, int step, size_t stride) {
    extern __shared__ uint8_t s_band[];                  // MASK_ROWS x cols
    const int s = blockIdx.y, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const TrkState& st = a.st[s];
    int r0, r1; const int nb = mask_band(a, r0, r1);
    const bool el = kf_eligible(st);
    for (int k = t; k < nb; k += TRK_NT) s_band[k] = el ? 255 : 0;
    __syncthreads();
    if (el) {
        const size_t fb = (size_t)s * a.cap;
        for (int i = wv; i < st.n_feat; i += TRK_NT / 64) {              // one wave per feature
            const float x = a.xy[(fb + i) * 2], y = a.xy[(fb + i) * 2 + 1];
            if (!isfinite(x) || !isfinite(y)) continue;                   // no rectangle (the hosts cannot reach this: LK never keeps such a point)
            const int x0 = max(cv_round(x - 20.f), 0), x1 = min(cv_round(x + 20.f), a.cols - 1);
            const int y0 = max(max(cv_round(y - 20.f), 0), r0), y1 = min(min(cv_round(y + 20.f), a.rows - 1), r1 - 1);
            if (x0 > x1 || y0 > y1) continue;
            const int w = x1 - x0 + 1, cnt = w * (y1 - y0 + 1);           // <= 41 x MASK_ROWS
            for (int k = lane; k < cnt; k += 64) s_band[(y0 - r0 + k / w) * a.cols + x0 + k % w] = 0;
        }
    }
    __syncthreads();
    store_mask_band(a, masks, step, stride, r0, nb, s_band, 0);
}

// one feature's row of a turn's or an init's outputs: its map point (id -1, position 0 = none), its left pixel, its right match
__device__ __forceinline__ void write_feature_row(const TrkArgs& a, const KfArgs& k, size_t fb, int i, int64_t id, const double* p, bool rok) {
    k.featMpId[fb + i] = id; k.featTag[fb + i] = i; k.featFlags[fb + i] = 0; k.rightOk[fb + i] = rok ? 1 : 0;
    for (int r = 0; r < 3; r++) k.featMpPos[(fb + i) * 3 + r] = p[r];
    k.featUv[(fb + i) * 2] = a.kfP0[(fb + i) * 2]; k.featUv[(fb + i) * 2 + 1] = a.kfP0[(fb + i) * 2 + 1];
    k.rightXy[(fb + i) * 2] = a.kfNxt[(fb + i) * 2]; k.rightXy[(fb + i) * 2 + 1] = a.kfNxt[(fb + i) * 2 + 1];
}

// feature f of the scratch tables: triangulate its left pixel and right match in the left camera's frame when `attempt`, store the point and whether it stands
__device__ __forceinline__ bool triangulate_feature(const TrkArgs& a, double baseline, size_t f, bool attempt, double* X) {
    bool tri = false; X[0] = 0; X[1] = 0; X[2] = 0;
    if (attempt) {
        const double ul = a.kfP0[f * 2], vl = a.kfP0[f * 2 + 1], ur = a.kfNxt[f * 2], vr = a.kfNxt[f * 2 + 1];
        const double P[2][12] = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0},
                                 {1, 0, 0, -baseline, 0, 1, 0, 0, 0, 0, 1, 0}};                  // as match_tri.hip's k_triangulate
        const double pt[2][2] = {{(ul - a.cx) / a.fx, (vl - a.cy) / a.fy}, {(ur - a.cx) / a.fx, (vr - a.cy) / a.fy}};
        double ratio; tri_solve(P, pt, X, ratio);
        tri = ratio < 1e-2 && X[2] > 0;
    }
    a.kfXyz[f * 3] = X[0]; a.kfXyz[f * 3 + 1] = X[1]; a.kfXyz[f * 3 + 2] = X[2]; a.kfTok[f] = tri ? 1 : 0;
    return tri;
}

// what a turn or an init tells about stream s (thread 0): the new key-frame's id, feature and outlier counts, and the 8-int report
__device__ __forceinline__ void write_report(const KfArgs& k, int s, int64_t kfId, int nFeatOut, int nOutlMp, int status, int frameId, int nNew, int nRight,
                                             int nTri, int nFeat, int nLm) {
    int32_t* rep = k.report + (size_t)s * 8;
    k.newKfId[s] = kfId; k.nFeat[s] = nFeatOut; k.nOutlMp[s] = nOutlMp;
    rep[0] = status; rep[1] = frameId; rep[2] = nNew; rep[3] = nRight; rep[4] = nTri; rep[5] = nFeat; rep[6] = nLm; rep[7] = 0;
}

// (uniform) no key-frame: no id, no features, and the table sizes the stream keeps
__device__ __forceinline__ void refuse(const KfArgs& k, int s, const TrkState& st, int status, int frameId, int nNew, int nRight) {
    if (threadIdx.x == 0) write_report(k, s, -1, 0, 0, status, frameId, nNew, nRight, 0, st.n_feat, st.n_lm);
}

// the rebuilt landmark table kfId / kfOutl / kfPos[0, nLm) becomes the stream's (all threads, after a barrier behind the last read of the old one)
__device__ __forceinline__ void commit_landmarks(const TrkArgs& a, size_t lb, int nLm) {
    for (int j = threadIdx.x; j < nLm; j += TRK_NT) {
        a.lmId[lb + j] = a.kfId[lb + j]; a.lmOutl[lb + j] = a.kfOutl[lb + j];
        for (int r = 0; r < 3; r++) a.lmPos[(lb + j) * 3 + r] = a.kfPos[(lb + j) * 3 + r];
    }
}

// thread 0, last: frame frameId becomes key-frame ids[1] at `pose` and the stream's reference, cur.rel = I (:440), nTri map-point ids are spent,
// the stream holds m features on nLm landmarks, runs again, and reports
__device__ __forceinline__ void adopt_keyframe(const TrkArgs& a, const KfArgs& k, int s, const double* pose, int frameId, int nNew, int nRight, int nTri, int m,
                                               int nLm, int nOutl) {
    TrkState& st = a.st[s]; int64_t* ids = a.ids + (size_t)s * 3;
    const int64_t kfId = ids[1];
    for (int c = 0; c < 7; c++) { st.ref_pose[c] = pose[c]; k.newKfPose[(size_t)s * 7 + c] = pose[c]; }
    for (int c = 0; c < 16; c++) st.last_rel[c] = (c % 5 == 0) ? 1.0 : 0.0;
    ids[0] = kfId; ids[1] = kfId + 1; ids[2] += nTri;
    st.ref_frame_id = frameId; st.n_feat = m; st.n_lm = nLm; st.n_outl = 0; st.frozen = 0; st.why = TRK_WHY_NONE;
    write_report(k, s, kfId, m, nOutl, MYSLAM_OK, frameId, nNew, nRight, nTri, m, nLm);
}

// ---- turn head: blockIdx.x == 0 decides eligibility, appends the detected key-points and writes the right start points (rules a + b);
//      the other blocks copy the stream's right image into its free buffer (rule c) ----
__global__ __launch_bounds__(TRK_NT) void k_kf_head(TrkArgs a, KfArgs k) {
    const int s = blockIdx.y, t = threadIdx.x;
    const TrkState& st = a.st[s];
    const bool el = kf_eligible(st);
    const int n = st.n_feat, nNew = clamped_count(k.nNew, s, k.kpCap), m = n + nNew;
    const bool go = el && m <= a.cap;
    if (blockIdx.x > 0) {
        if (go) copy_image_rows(a, blockIdx.x - 1, k.right + (size_t)s * k.stride, k.step, trk_image(a, s, 1 - st.slot));
        return;
    }
    if (!go) {
        if (t == 0) { a.kfSel[s] = -1; a.kfCounts[s] = 0; a.kfCode[s] = el ? KF_CAPACITY : KF_NO_TURN; }
        return;
    }
    __shared__ double sT[16];
    if (t == 0) {
        tcw_of(st.last_rel, st.ref_pose, sT);            // :340
        a.kfSel[s] = 1 - st.slot; a.kfCounts[s] = m; a.kfCode[s] = KF_GO;
    }
    __syncthreads();
    const size_t fb = (size_t)s * a.cap;
    const double* pos = a.lmPos + (size_t)s * a.lmCap * 3;
    const uint8_t* outl = a.lmOutl + (size_t)s * a.lmCap;
    const myslam_keypoint* kps = k.newKps + (size_t)s * k.kpCap;
    for (int i = t; i < m; i += TRK_NT) {
        float x, y;
        int l = -1;
        if (i < n) { x = a.xy[(fb + i) * 2]; y = a.xy[(fb + i) * 2 + 1]; l = a.lm[fb + i]; }
        else { x = kps[i - n].x; y = kps[i - n].y; }
        float u = x, v = y;
        if (l >= 0 && !outl[l]) {                        // world2pixel of the RIGHT camera: pc = mv(R, pw) + t, then pc + (-baseline, 0, 0) (:342-349)
            double pc[3];
            se3_apply(sT, pos + 3 * l, pc);
            pc[0] = dadd(pc[0], -k.baseline); pc[1] = dadd(pc[1], 0.0); pc[2] = dadd(pc[2], 0.0);      // (the sums with 0.0 turn -0.0 into +0.0, as the hosts')
            pixel_of(a, pc, u, v);
        }
        a.kfP0[(fb + i) * 2] = x; a.kfP0[(fb + i) * 2 + 1] = y;
        a.kfNxt[(fb + i) * 2] = u; a.kfNxt[(fb + i) * 2 + 1] = v;
    }
}

// ---- turn tail: rules d - g, one block per stream.  Everything is built in scratch and in the output arrays; the state is written last ----
__global__ __launch_bounds__(TRK_NT) void k_kf_tail(TrkArgs a, KfArgs k) {
    __shared__ int s_w[TRK_NW];
    __shared__ double sTcw[16], sTwc[16];
    const int s = blockIdx.x, t = threadIdx.x;
    TrkState& st = a.st[s];
    const int code = a.kfCode[s];
    const int n = st.n_feat, nNew = clamped_count(k.nNew, s, k.kpCap), m = n + nNew, nLm = st.n_lm, nOutl = st.n_outl;
    const int frameId = st.next_frame_id - 1;            // the frame the last step tracked
    // no turn: the stream keeps every byte
    if (code != KF_GO) { refuse(k, s, st, code == KF_CAPACITY ? MYSLAM_ERR_CAPACITY : MYSLAM_TRACKER_NO_TURN, frameId, nNew, 0); return; }
    const size_t fb = (size_t)s * a.cap, lb = (size_t)s * a.lmCap;
    const int64_t nextMp = a.ids[(size_t)s * 3 + 2];
    if (t == 0) {
        tcw_of(st.last_rel, st.ref_pose, sTcw);
        se3_inv(sTcw, sTwc);                             // Twc of TriangulateNewPoints (:453)
    }
    for (int l = t; l < nLm; l += TRK_NT) { a.kfFirst[lb + l] = 0x7fffffff; a.kfMap[lb + l] = -1; }
    // the outlier list's ids (Map::AddOutlierMapPoint order), read from the table as it is BEFORE the rebuild
    for (int j = t; j < nOutl; j += TRK_NT) k.outlMpId[(size_t)s * 2 * a.cap + j] = a.lmId[lb + a.outlList[(size_t)s * 2 * a.cap + j]];
    __syncthreads();
    // first reference of every old slot (a minimum: the same whatever the order of arrival)
    for (int i = t; i < n; i += TRK_NT) { const int l = a.lm[fb + i]; if (l >= 0) atomicMin(&a.kfFirst[lb + l], i); }
    __syncthreads();
    // rule d (triangulation, feature order) and rule e (slots in order of first reference), 256 features at a time
    int nTri = 0, nSlots = 0, nRight = 0;
    for (int base = 0; base < m; base += TRK_NT) {
        const int i = base + t;
        int l = -1; bool rok = false, tri = false, opens = false;
        double X[3] = {0, 0, 0};
        if (i < m) {
            l = i < n ? a.lm[fb + i] : -1;
            rok = a.kfSt[fb + i] != 0;
            tri = triangulate_feature(a, k.baseline, fb + i, l < 0 && rok, X);       // expired() && mvpFeaturesRight[i] != nullptr (:458-459)
            // (the minimum was formed by atomics in L2: read it there, not from a line this CU may still hold)
            opens = tri || (l >= 0 && __hip_atomic_load(&a.kfFirst[lb + l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == i);
        }
        int tt, ts, tr;
        const int rt = block_rank<TRK_NW>(tri, s_w, tt), rs = block_rank<TRK_NW>(opens, s_w, ts);
        (void)block_rank<TRK_NW>(rok, s_w, tr);
        if (i < m) {
            const int slot = opens ? nSlots + rs : -1;
            a.kfSlot[fb + i] = slot;
            int64_t id = -1;
            double p[3] = {0, 0, 0};
            if (tri) {                                   // a new map point: id by rank, pos = mv(Twc.R, p) + Twc.t (:474-476)
                id = nextMp + nTri + rt;
                se3_apply(sTwc, X, p);
            } else if (l >= 0) {
                id = a.lmId[lb + l];
                for (int r = 0; r < 3; r++) p[r] = a.lmPos[(lb + l) * 3 + r];
            }
            if (opens && slot < a.lmCap) {               // (beyond lmCap the turn is refused below)
                if (l >= 0) a.kfMap[lb + l] = slot;
                a.kfId[lb + slot] = id; a.kfOutl[lb + slot] = l >= 0 ? a.lmOutl[lb + l] : 0;
                for (int r = 0; r < 3; r++) a.kfPos[(lb + slot) * 3 + r] = p[r];
            }
            write_feature_row(a, k, fb, i, id, p, rok);
        }
        nTri += tt; nSlots += ts; nRight += tr;
    }
    if (nSlots > a.lmCap) { refuse(k, s, st, MYSLAM_ERR_CAPACITY, frameId, nNew, 0); return; }
    __syncthreads();                                     // kfMap, kfPos .. are complete; every read of the old tables is done
    // ---- commit ----
    for (int i = t; i < m; i += TRK_NT) {
        const int l = i < n ? a.lm[fb + i] : -1;
        const int slot = a.kfSlot[fb + i];
        a.lm[fb + i] = slot >= 0 ? slot : (l >= 0 ? a.kfMap[lb + l] : -1);
        if (i >= n) { a.xy[(fb + i) * 2] = a.kfP0[(fb + i) * 2]; a.xy[(fb + i) * 2 + 1] = a.kfP0[(fb + i) * 2 + 1]; }
    }
    commit_landmarks(a, lb, nSlots);
    if (t != 0) return;
    double pose[7];
    se3_p7_of(sTcw, pose);                               // kf.pose = p7(cur.rel * T(ref pose)) (:433)
    adopt_keyframe(a, k, s, pose, frameId, nNew, nRight, nTri, m, nSlots, nOutl);
}

// ---- the map moved under the tracker (back end, loop closer): landmarks and the reference pose follow their ids ----
// (g: dev_tables.h's view of the back end's tables; the observation columns are not given)
// (gate, NULL = none: a stream whose entry is not 0 keeps every byte — the mapper's idle items, backend_launch.h)
__global__ __launch_bounds__(TRK_NT) void k_kf_update(TrkArgs a, BeTablesRead g, const int32_t* gate) {
    const int s = blockIdx.x, t = threadIdx.x;
    TrkState& st = a.st[s];
    if (st.frozen != 0 || st.idsValid == 0 || (gate && gate[s] != 0)) return;
    const size_t lb = (size_t)s * a.lmCap;
    const int nMp = clamped_count(g.n_mp, s, g.mp_cap), nKf = clamped_count(g.n_kf, s, g.kf_cap);
    const auto m = g.item(s);
    for (int l = t; l < st.n_lm; l += TRK_NT) {
        const int r = find_row(m.mp_id, nMp, a.lmId[lb + l]);
        if (r < 0) continue;
        for (int c = 0; c < 3; c++) a.lmPos[(lb + l) * 3 + c] = m.mp_pos[3 * r + c];
        a.lmOutl[lb + l] = m.mp_outlier[r];
    }
    if (t == 0) {
        const int r = find_row(m.kf_id, nKf, a.ids[(size_t)s * 3]);
        if (r >= 0) for (int c = 0; c < 7; c++) st.ref_pose[c] = m.kf_pose[7 * r + c];
    }
}

// ---- the optimiser reset features of the reference key-frame (src/backend.cpp:236-247).  KeyFrame shares its Feature objects with its Frame
//      (src/keyframe.cpp:21), so while the last frame IS that key-frame's frame (no step since the turn or the init) TrackLastFrame
//      (src/frontend.cpp:127-171) sees the reset: feature `tag` of the stream loses its landmark.  Nothing else of the stream changes ----
__global__ __launch_bounds__(TRK_NT) void k_trk_clear_links(TrkArgs a, const int64_t* kf_id, const int32_t* tag, const int32_t* n, int list_cap, int32_t* n_cleared) {
    __shared__ int s_w[TRK_NW];
    const int s = blockIdx.x, t = threadIdx.x;
    const TrkState& st = a.st[s];
    const bool on = st.idsValid != 0 && st.ref_frame_id == st.next_frame_id - 1;          // uniform
    const int cnt = on ? clamped_count(n, s, list_cap) : 0, nFeat = clamped_count(st.n_feat, a.cap);
    const int64_t ref = a.ids[(size_t)s * 3];
    int cleared = 0;
    for (int base = 0; base < cnt; base += TRK_NT) {
        const int j = base + t;
        bool hit = false;
        if (j < cnt) {
            const int f = tag[(size_t)s * list_cap + j];
            hit = kf_id[(size_t)s * list_cap + j] == ref && f >= 0 && f < nFeat;
            if (hit) a.lm[(size_t)s * a.cap + f] = -1;
        }
        int tot;
        (void)block_rank<TRK_NW>(hit, s_w, tot);
        cleared += tot;
    }
    if (t == 0 && n_cleared) n_cleared[s] = cleared;
}

// ---- LoopLocalFusion re-linked features of the reference key-frame (src/loopclosing.cpp:521-530).  Same sharing and same guard as above: while
//      the last frame is that key-frame's frame, feature `tag` names the point its list entry gives (an archive slot of the map, -1 = none).  A
//      feature that has a landmark keeps its slot, and the slot takes the target's id, position and outlier flag (every feature of the frame that
//      shared the slot observed the same point and moved with it); a feature without one takes the slot that carries the target's id, else a new
//      one.  The entries are walked in list order on copies (the turn's scratch: kfId, kfMap = the archive slot a landmark slot takes its values
//      from, kfSlot = the features' slots), the landmark search of an entry is the block's; nothing of the stream is written before the walk has
//      shown that every slot is in range and the table holds the new landmarks ----
struct TrkRelink {
    const int64_t* kf_id; const int32_t* tag; const int32_t* slot; const int32_t* n; int list_cap;
    const int64_t* mp_id; const double* mp_pos; const uint8_t* mp_state; const int32_t* n_mp; int point_cap;
    int32_t* n_relinked; int32_t* status;
};
__global__ __launch_bounds__(TRK_NT) void k_trk_relink(TrkArgs a, TrkRelink r) {
    __shared__ int s_found, s_bad;
    const int s = blockIdx.x, t = threadIdx.x;
    TrkState& st = a.st[s];
    if (st.idsValid == 0 || st.ref_frame_id != st.next_frame_id - 1) {     // uniform: the frame has moved on, every byte kept
        if (t == 0) { r.status[s] = MYSLAM_OK; if (r.n_relinked) r.n_relinked[s] = 0; }
        return;
    }
    const int cnt = clamped_count(r.n, s, r.list_cap), nFeat = clamped_count(st.n_feat, a.cap), nLm = clamped_count(st.n_lm, a.lmCap);
    const int aM = clamped_count(r.n_mp, s, r.point_cap);
    const int64_t ref = a.ids[(size_t)s * 3];
    const size_t fb = (size_t)s * a.cap, lb = (size_t)s * a.lmCap, lo = (size_t)s * r.list_cap, pb = (size_t)s * r.point_cap;
    const auto names = [&](int j) { const int f = r.tag[lo + j]; return r.kf_id[lo + j] == ref && f >= 0 && f < nFeat; };
    if (t == 0) { s_found = 0x7fffffff; s_bad = 0; }
    __syncthreads();
    bool bad = false;
    for (int j = t; j < cnt; j += TRK_NT)
        if (names(j)) { const int v = r.slot[lo + j]; bad |= v < -1 || v >= aM; }
    if (bad) s_bad = 1;
    for (int l = t; l < nLm; l += TRK_NT) { a.kfId[lb + l] = a.lmId[lb + l]; a.kfMap[lb + l] = -1; }
    for (int f = t; f < nFeat; f += TRK_NT) a.kfSlot[fb + f] = a.lm[fb + f];
    __syncthreads();
    if (s_bad) {                                                            // uniform; every byte of the stream kept
        if (t == 0) { r.status[s] = MYSLAM_ERR_INVALID; if (r.n_relinked) r.n_relinked[s] = 0; }
        return;
    }
    int nNew = 0, hits = 0;
    bool full = false;
    for (int j = 0; j < cnt; j++) {                                         // uniform: every thread reads the same entry
        __syncthreads();                                                    // what the entry before wrote
        if (!names(j)) continue;
        hits++;
        const int f = r.tag[lo + j], v = r.slot[lo + j];
        if (v < 0) { if (t == 0) a.kfSlot[fb + f] = -1; continue; }
        const int64_t id = r.mp_id[pb + v];
        const int L = a.kfSlot[fb + f];
        if (L >= 0 && L < nLm + nNew) {                                     // an observation moved with its point: the slot is the target's now
            if (t == 0) { a.kfId[lb + L] = id; a.kfMap[lb + L] = v; }
            continue;
        }
        int mine = 0x7fffffff;
        for (int l = t; l < nLm + nNew; l += TRK_NT)
            if (a.kfId[lb + l] == id) { mine = l; break; }
        if (mine != 0x7fffffff) atomicMin(&s_found, mine);                 // LDS
        __syncthreads();
        const int found = s_found;
        __syncthreads();
        const bool opens = found == 0x7fffffff;
        if (opens && nLm + nNew >= a.lmCap) { full = true; continue; }      // uniform
        const int slot = opens ? nLm + nNew : found;
        if (t == 0) {
            s_found = 0x7fffffff;
            a.kfSlot[fb + f] = slot; a.kfId[lb + slot] = id; a.kfMap[lb + slot] = v;
        }
        nNew += opens;
    }
    __syncthreads();
    if (full) {                                                             // uniform; only the scratch was written
        if (t == 0) { r.status[s] = MYSLAM_ERR_CAPACITY; if (r.n_relinked) r.n_relinked[s] = 0; }
        return;
    }
    // ---- commit ----
    for (int l = t; l < nLm + nNew; l += TRK_NT) {
        const int v = a.kfMap[lb + l];
        if (v < 0) continue;
        a.lmId[lb + l] = a.kfId[lb + l]; a.lmOutl[lb + l] = r.mp_state[pb + v] == 1;
        for (int c = 0; c < 3; c++) a.lmPos[(lb + l) * 3 + c] = r.mp_pos[(pb + v) * 3 + c];
    }
    for (int f = t; f < nFeat; f += TRK_NT) a.lm[fb + f] = a.kfSlot[fb + f];
    if (t == 0) {
        st.n_lm = nLm + nNew;
        r.status[s] = MYSLAM_OK;
        if (r.n_relinked) r.n_relinked[s] = hits;
    }
}

// ---- the stored previous left image of the selected streams <- imgs (the pyramid follows in lk_bank_pyramid) ----
__global__ __launch_bounds__(TRK_NT) void k_kf_set_image(TrkArgs a, const uint8_t* imgs, int step, size_t stride, const uint8_t* select) {
    const int s = blockIdx.y, t = threadIdx.x;
    const bool on = select[s] != 0;
    const int slot = a.st[s].slot;
    if (blockIdx.x == 0) { if (t == 0) a.kfSel[s] = on ? slot : -1; return; }
    if (on) copy_image_rows(a, blockIdx.x - 1, imgs + (size_t)s * stride, step, trk_image(a, s, slot));
}

// =====================================================================================================================================
// StereoInit (include/myslam_hip.h, myslam_tracker_init_*): Frontend::StereoInit (:282-295) with DetectFeatures' mask over an empty table
// (:305-309), FindFeaturesInRight (:335-379), BuildInitMap (:385-417) and InsertKeyFrame's INITING branch (:427-428, :441-443) for every
// INIT-ELIGIBLE stream.  Its head and tail are kernels of their own (no landmark to project or to keep, a pose of I, the retry rule) over the
// pieces the turn's kernels are made of.
__device__ __forceinline__ bool init_eligible(const TrkState& st) { return st.frozen != 0 && st.status == TRK_INITING && st.why == TRK_WHY_NONE && st.overflow == 0; }

// ---- masks: 255 everywhere for an init-eligible stream (no feature draws a rectangle), 0 otherwise; no LDS ----
__global__ __launch_bounds__(TRK_NT) void k_init_masks(TrkArgs a, uint8_t* masks, int step, size_t stride) {
    int r0, r1; const int nb = mask_band(a, r0, r1);
    store_mask_band(a, masks, step, stride, r0, nb, nullptr, init_eligible(a.st[blockIdx.y]) ? 255 : 0);
}

// ---- init head: blockIdx.x == 0 decides eligibility and writes the detected key-points as left pixels and right start points (rules a + b);
//      the other blocks copy the left image into the stream's buffer `slot` and the right image into buffer 1 - slot ----
__global__ __launch_bounds__(TRK_NT) void k_init_head(TrkArgs a, KfArgs k, const uint8_t* left, int32_t* selLeft) {
    const int s = blockIdx.y, t = threadIdx.x;
    const TrkState& st = a.st[s];
    const bool el = init_eligible(st);
    const int m = clamped_count(k.nNew, s, k.kpCap);
    const bool go = el && m <= a.cap;
    if (blockIdx.x > 0) {
        if (!go) return;
        uint8_t *dstL = trk_image(a, s, st.slot), *dstR = trk_image(a, s, 1 - st.slot);      // (both before the first store: `slot` is read once)
        copy_image_rows(a, blockIdx.x - 1, left + (size_t)s * k.stride, k.step, dstL);
        copy_image_rows(a, blockIdx.x - 1, k.right + (size_t)s * k.stride, k.step, dstR);
        return;
    }
    if (t == 0) {
        selLeft[s] = go ? st.slot : -1; a.kfSel[s] = go ? 1 - st.slot : -1;       // LK tracks from buffer 1 - kfSel into buffer kfSel
        a.kfCounts[s] = go ? m : 0; a.kfCode[s] = go ? KF_GO : (el ? KF_CAPACITY : KF_NO_TURN);
    }
    if (!go) return;
    const size_t fb = (size_t)s * a.cap;
    const myslam_keypoint* kps = k.newKps + (size_t)s * k.kpCap;
    for (int i = t; i < m; i += TRK_NT) {                    // every start point is the feature's own pixel (:350-352)
        const float x = kps[i].x, y = kps[i].y;
        a.kfP0[(fb + i) * 2] = x; a.kfP0[(fb + i) * 2 + 1] = y;
        a.kfNxt[(fb + i) * 2] = x; a.kfNxt[(fb + i) * 2 + 1] = y;
    }
}

// ---- init tail: rules c - g, one block per stream.  Everything is built in scratch and in the output arrays; the state is written last ----
__global__ __launch_bounds__(TRK_NT) void k_init_tail(TrkArgs a, KfArgs k, int initGood) {
    __shared__ int s_w[TRK_NW];
    const int s = blockIdx.x, t = threadIdx.x;
    TrkState& st = a.st[s];
    const int code = a.kfCode[s];
    const int m = clamped_count(k.nNew, s, k.kpCap);
    if (code == KF_NO_TURN) { refuse(k, s, st, MYSLAM_TRACKER_NO_TURN, st.next_frame_id - 1, m, 0); return; }
    const int frameId = st.next_frame_id;                    // the Frame that GrabStereoImage constructed
    if (code != KF_GO) { refuse(k, s, st, MYSLAM_ERR_CAPACITY, frameId, m, 0); return; }
    const size_t fb = (size_t)s * a.cap, lb = (size_t)s * a.lmCap;
    const int64_t nextMp = a.ids[(size_t)s * 3 + 2];
    // rule d (triangulation in feature order, slot = rank among the successes), 256 features at a time
    int nTri = 0, nRight = 0;
    for (int base = 0; base < m; base += TRK_NT) {
        const int i = base + t;
        bool rok = false, tri = false;
        double X[3] = {0, 0, 0};
        if (i < m) {
            rok = a.kfSt[fb + i] != 0;
            tri = triangulate_feature(a, k.baseline, fb + i, rok, X);            // mvpFeaturesRight[i] != nullptr (:394)
        }
        int tt, tr;
        const int rt = block_rank<TRK_NW>(tri, s_w, tt);
        (void)block_rank<TRK_NW>(rok, s_w, tr);
        if (i < m) {
            const int slot = tri ? nTri + rt : -1;
            a.kfSlot[fb + i] = slot;
            const int64_t id = tri ? nextMp + slot : -1;
            if (!tri) { X[0] = 0; X[1] = 0; X[2] = 0; }
            if (tri && slot < a.lmCap) {                     // (beyond lmCap the init is refused below); the key-frame's pose is I: pos = X itself
                a.kfId[lb + slot] = id; a.kfOutl[lb + slot] = 0;
                for (int r = 0; r < 3; r++) a.kfPos[(lb + slot) * 3 + r] = X[r];
            }
            write_feature_row(a, k, fb, i, id, X, rok);
        }
        nTri += tt; nRight += tr;
    }
    if (nRight < initGood) {                                 // uniform.  StereoInit returns false (:285-287): only the Frame's id was spent
        refuse(k, s, st, MYSLAM_TRACKER_INIT_RETRY, frameId, m, nRight);
        if (t == 0) st.next_frame_id = frameId + 1;
        return;
    }
    if (nTri > a.lmCap) { refuse(k, s, st, MYSLAM_ERR_CAPACITY, frameId, m, nRight); return; }
    __syncthreads();                                         // kfSlot, kfPos, kfId are complete
    // ---- commit ----
    for (int i = t; i < m; i += TRK_NT) {
        a.lm[fb + i] = a.kfSlot[fb + i];
        a.xy[(fb + i) * 2] = a.kfP0[(fb + i) * 2]; a.xy[(fb + i) * 2 + 1] = a.kfP0[(fb + i) * 2 + 1];
    }
    commit_landmarks(a, lb, nTri);
    if (t != 0) return;
    const double ident[7] = {0, 0, 0, 1, 0, 0, 0};
    adopt_keyframe(a, k, s, ident, frameId, m, nRight, nTri, m, nTri, 0);
    for (int c = 0; c < 16; c++) st.rel_motion[c] = (c % 5 == 0) ? 1.0 : 0.0;
    st.next_frame_id = frameId + 1; st.status = TRK_GOOD; st.idsValid = 1;
}

}  // namespace myslam_hip

using namespace myslam_hip;

struct myslam_tracker {
    hipStream_t stream = nullptr;
    myslam_lk* lk = nullptr;
    int S = 0, rows = 0, cols = 0, cap = 0, lmCap = 0, levels = 0;
    size_t pyrBytes = 0;
    TrkArgs a{};
    uint8_t* d_pyr = nullptr;
    int32_t* d_selLeft = nullptr;          // StereoInit: the buffer the left image's levels go to (a.kfSel names the right image's)
    BufSet mem;                            // owns every block that `a`, d_pyr and d_selLeft name
    std::vector<char> hasImage;
};

static int trk_alloc_all(myslam_tracker* h) {
    TrkArgs& a = h->a;
    const size_t S = h->S, F = S * h->cap, L = S * h->lmCap;
    int rc = 0;
    auto own = [&](auto*& p, size_t n) { return h->mem.own(p, n); };
    if ((rc = own(a.st, S)) || (rc = own(a.xy, F * 2)) || (rc = own(a.lm, F)) || (rc = own(a.lmPos, L * 3)) || (rc = own(a.lmOutl, L)) ||
        (rc = own(a.outlList, F * 2)) || (rc = own(a.img, 2 * a.imgSel)) || (rc = own(h->d_pyr, 2 * S * h->pyrBytes)) ||
        (rc = own(a.sel, S)) || (rc = own(a.counts, S)) || (rc = own(a.p0, F * 2)) || (rc = own(a.p1, F * 2)) || (rc = own(a.nxt, F * 2)) ||
        (rc = own(a.lkSt, F)) || (rc = own(a.curXy, F * 2)) || (rc = own(a.curLm, F)) || (rc = own(a.curPo, F)) || (rc = own(a.curN, S)) ||
        (rc = own(a.poPose, S * 7)) || (rc = own(a.poPts, F * 3)) || (rc = own(a.poObs, F * 2)) || (rc = own(a.poCounts, S)) ||
        (rc = own(a.poOutl, F)) || (rc = own(a.poInl, S)) || (rc = own(a.poStatus, S)) ||
        (rc = own(a.lmId, L)) || (rc = own(a.ids, S * 3)) || (rc = own(a.kfSel, S)) || (rc = own(a.kfCounts, S)) || (rc = own(a.kfCode, S)) ||
        (rc = own(a.kfP0, F * 2)) || (rc = own(a.kfNxt, F * 2)) || (rc = own(a.kfSt, F)) || (rc = own(a.kfXyz, F * 3)) || (rc = own(a.kfTok, F)) ||
        (rc = own(a.kfSlot, F)) || (rc = own(a.kfFirst, L)) || (rc = own(a.kfMap, L)) || (rc = own(a.kfPos, L * 3)) || (rc = own(a.kfOutl, L)) ||
        (rc = own(a.kfId, L)) || (rc = own(h->d_selLeft, S)))
        return rc;
    std::vector<TrkState> init(S);
    memset(init.data(), 0, S * sizeof(TrkState));
    for (TrkState& st : init) { st.frozen = 1; st.status = TRK_INITING; }
    // (every other buffer is written before it is read: tables by set_frame, scratch by the step's own kernels)
    const std::vector<int32_t> zeros(S, 0);
    if ((rc = upload_table(a.st, init.data(), S * sizeof(TrkState))) || (rc = upload_table(a.counts, zeros.data(), S * sizeof(int32_t)))) return rc;
    const std::vector<int64_t> zeros64(S * 3, 0);
    if ((rc = upload_table(a.kfCounts, zeros.data(), S * sizeof(int32_t))) || (rc = upload_table(a.ids, zeros64.data(), S * 3 * sizeof(int64_t)))) return rc;
    return MYSLAM_OK;
}

// a batch of S images, `step` bytes between rows and `stride` between images, does not hold rows x cols each
static bool image_args_bad(const myslam_tracker* h, int step, size_t stride) { return step < h->cols || stride < (size_t)(h->rows - 1) * step + h->cols; }
// stream s's state as the device has it once the handle's stream has drained (synchronous)
static int trk_fetch_state(myslam_tracker* h, int s, TrkState& hs) { return copy_sync(&hs, h->a.st + s, sizeof(TrkState), hipMemcpyDeviceToHost, h->stream); }
// grid of the kernels that copy images: per stream, block 0 for the rules and one block per TRK_COPY_ROWS rows (copy_image_rows)
static dim3 trk_copy_grid(const myslam_tracker* h) { return dim3(1 + (h->rows + TRK_COPY_ROWS - 1) / TRK_COPY_ROWS, h->S); }

// the arguments myslam_tracker_keyframe_batch and myslam_tracker_init_batch share -> k; false when one of them is invalid
static bool kf_args(const myslam_tracker* h, const uint8_t* d_right, int step, size_t stride, const myslam_keypoint* d_new_kps, const int32_t* d_n_new, int kp_cap,
                    double baseline, int64_t* d_new_kf_id, double* d_new_kf_pose, int64_t* d_feat_mp_id, double* d_feat_mp_pos, float* d_feat_uv,
                    int32_t* d_feat_tag, uint8_t* d_feat_flags, int32_t* d_n_feat, int64_t* d_outlier_mp_id, int32_t* d_n_outlier_mp, float* d_right_xy,
                    uint8_t* d_right_ok, int32_t* d_report, KfArgs& k) {
    if (!h || !d_right || !d_new_kps || !d_n_new || !d_new_kf_id || !d_new_kf_pose || !d_feat_mp_id || !d_feat_mp_pos || !d_feat_uv || !d_feat_tag ||
        !d_feat_flags || !d_n_feat || !d_outlier_mp_id || !d_n_outlier_mp || !d_right_xy || !d_right_ok || !d_report || image_args_bad(h, step, stride) || kp_cap < 1)
        return false;
    k = KfArgs{d_right, step, stride, d_new_kps, d_n_new, kp_cap, baseline, d_new_kf_id, d_new_kf_pose, d_feat_mp_id, d_feat_mp_pos, d_feat_uv, d_feat_tag,
               d_feat_flags, d_n_feat, d_outlier_mp_id, d_n_outlier_mp, d_right_xy, d_right_ok, d_report};
    return true;
}

// head -> pyramid levels -> LK from the left image's buffer into the right image's -> tail: a key-frame turn (d_left null: the left image and
// its levels are the last step's, buffer `slot`) or StereoInit (d_left: its levels go to buffer `slot` first) (:358-361)
static int trk_run_turn(myslam_tracker* h, const KfArgs& k, const uint8_t* d_left, int init_good) {
    const TrkArgs& a = h->a;
    hipStream_t st = h->stream;
    const int S = h->S;
    const size_t pyrSel = (size_t)S * h->pyrBytes;
    if (d_left) hipLaunchKernelGGL(k_init_head, trk_copy_grid(h), dim3(TRK_NT), 0, st, a, k, d_left, h->d_selLeft);
    else hipLaunchKernelGGL(k_kf_head, trk_copy_grid(h), dim3(TRK_NT), 0, st, a, k);
    MYSLAM_HIP_CHECK(hipGetLastError());
    int rc;
    if (d_left && (rc = lk_bank_pyramid(h->lk, d_left, k.step, k.stride, h->d_pyr, S, h->d_selLeft, pyrSel))) return rc;
    if ((rc = lk_bank_pyramid(h->lk, k.right, k.step, k.stride, h->d_pyr, S, a.kfSel, pyrSel))) return rc;
    if ((rc = lk_bank_track(h->lk, a.img, h->cols, a.imgBytes, h->d_pyr, S, a.kfSel, a.imgSel, pyrSel, a.kfP0, a.kfNxt, a.kfCounts, h->cap, a.kfSt))) return rc;
    if (d_left) hipLaunchKernelGGL(k_init_tail, dim3(S), dim3(TRK_NT), 0, st, a, k, init_good);
    else hipLaunchKernelGGL(k_kf_tail, dim3(S), dim3(TRK_NT), 0, st, a, k);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

extern "C" {

int myslam_tracker_create(myslam_tracker** out, int streams, int rows, int cols, int cap, int landmark_cap, double fx, double fy, double cx, double cy,
                          int tracking_good, int tracking_bad, int win, int max_level, int max_iters, float eps, float min_eig_threshold) {
    if (!out || streams < 1 || rows < 1 || cols < 1 || cap < 1 || cap > 4096 || landmark_cap < 1) return MYSLAM_ERR_INVALID;
    myslam_lk* lk = nullptr;
    int rc = myslam_lk_create(&lk, win, max_level, max_iters, eps, min_eig_threshold);
    if (rc) return rc;
    myslam_tracker* h = new myslam_tracker();
    h->lk = lk; h->S = streams; h->rows = rows; h->cols = cols; h->cap = cap; h->lmCap = landmark_cap;
    h->hasImage.assign(streams, 0);
    lk_bank_plan(lk, rows, cols, &h->pyrBytes, &h->levels);
    TrkArgs& a = h->a;
    a.S = streams; a.cap = cap; a.lmCap = landmark_cap; a.rows = rows; a.cols = cols;
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.good = tracking_good; a.bad = tracking_bad;
    a.imgBytes = ((size_t)rows * cols + 255) & ~(size_t)255; a.imgSel = (size_t)streams * a.imgBytes;
    if ((rc = trk_alloc_all(h))) { myslam_tracker_destroy(h); return rc; }
    *out = h;
    return MYSLAM_OK;
}

int myslam_tracker_destroy(myslam_tracker* h) {
    if (!h) return MYSLAM_ERR_INVALID;
    (void)hipStreamSynchronize(h->stream);
    if (h->lk) (void)myslam_lk_destroy(h->lk);
    delete h;
    return MYSLAM_OK;
}

int myslam_tracker_set_stream(myslam_tracker* h, void* s) {
    if (!h) return MYSLAM_ERR_INVALID;
    MYSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    h->stream = (hipStream_t)s;
    return myslam_lk_set_stream(h->lk, s);
}

int myslam_tracker_launches_per_step(const myslam_tracker* h) {
    return h ? 5 + h->levels : MYSLAM_ERR_INVALID;
}

int myslam_tracker_set_frame(myslam_tracker* h, int s, const float* feat_xy, const int32_t* feat_landmark, int n_feat, const double* landmark_pos,
                             const uint8_t* landmark_outlier, int n_landmarks, const double* ref_pose7, int ref_frame_id, const double* last_rel16,
                             const double* rel_motion16, int next_frame_id, int status, int kf_every, const uint8_t* prev_image, int image_step) {
    if (!h || s < 0 || s >= h->S || n_feat < 0 || n_landmarks < 0 || (n_feat > 0 && (!feat_xy || !feat_landmark)) ||
        (n_landmarks > 0 && (!landmark_pos || !landmark_outlier)) || !ref_pose7 || !last_rel16 || !rel_motion16 || (prev_image && image_step < h->cols))
        return MYSLAM_ERR_INVALID;
    if (!prev_image && !h->hasImage[s]) return MYSLAM_ERR_INVALID;
    const bool fits = n_feat <= h->cap && n_landmarks <= h->lmCap;
    if (fits)
        for (int i = 0; i < n_feat; i++) if (feat_landmark[i] < -1 || feat_landmark[i] >= n_landmarks) return MYSLAM_ERR_INVALID;
    hipStream_t st = h->stream;
    TrkArgs& a = h->a;
    TrkState hs;
    if (int rc = trk_fetch_state(h, s, hs)) return rc;
    memcpy(hs.ref_pose, ref_pose7, sizeof(double) * 7); memcpy(hs.last_rel, last_rel16, sizeof(double) * 16); memcpy(hs.rel_motion, rel_motion16, sizeof(double) * 16);
    hs.ref_frame_id = ref_frame_id; hs.next_frame_id = next_frame_id; hs.status = status; hs.kf_every = kf_every;
    hs.frozen = 0; hs.n_outl = 0; hs.overflow = fits ? 0 : 1;
    hs.why = TRK_WHY_NONE; hs.idsValid = 0;  // the landmark table is new: its ids are the caller's to give again (myslam_tracker_set_ids)
    hs.n_feat = fits ? n_feat : 0; hs.n_lm = fits ? n_landmarks : 0;
    if (fits) {
        const size_t fb = (size_t)s * h->cap, lb = (size_t)s * h->lmCap;
        if (n_feat) {
            MYSLAM_HIP_CHECK(hipMemcpyAsync(a.xy + fb * 2, feat_xy, sizeof(float) * 2 * n_feat, hipMemcpyHostToDevice, st));
            MYSLAM_HIP_CHECK(hipMemcpyAsync(a.lm + fb, feat_landmark, sizeof(int32_t) * n_feat, hipMemcpyHostToDevice, st));
        }
        if (n_landmarks) {
            MYSLAM_HIP_CHECK(hipMemcpyAsync(a.lmPos + lb * 3, landmark_pos, sizeof(double) * 3 * n_landmarks, hipMemcpyHostToDevice, st));
            MYSLAM_HIP_CHECK(hipMemcpyAsync(a.lmOutl + lb, landmark_outlier, (size_t)n_landmarks, hipMemcpyHostToDevice, st));
        }
    }
    std::vector<uint8_t> packed;
    if (prev_image) {                        // one contiguous copy, then the levels above 0 of this one image
        packed.resize((size_t)h->rows * h->cols);
        for (int r = 0; r < h->rows; r++) memcpy(packed.data() + (size_t)r * h->cols, prev_image + (size_t)r * image_step, h->cols);
        uint8_t* d_img = a.img + (size_t)hs.slot * a.imgSel + (size_t)s * a.imgBytes;
        MYSLAM_HIP_CHECK(hipMemcpyAsync(d_img, packed.data(), packed.size(), hipMemcpyHostToDevice, st));
        if (int rc = lk_bank_pyramid(h->lk, d_img, h->cols, a.imgBytes, h->d_pyr + ((size_t)hs.slot * h->S + s) * h->pyrBytes, 1, nullptr, 0)) return rc;
        h->hasImage[s] = 1;
    }
    MYSLAM_HIP_CHECK(hipMemcpyAsync(a.st + s, &hs, sizeof(TrkState), hipMemcpyHostToDevice, st));
    MYSLAM_HIP_CHECK(hipStreamSynchronize(st));
    return fits ? MYSLAM_OK : MYSLAM_ERR_CAPACITY;
}

int myslam_tracker_get_frame(myslam_tracker* h, int s, float* feat_xy, int32_t* feat_landmark, int* n_feat, double* landmark_pos,
                             uint8_t* landmark_outlier, int* n_landmarks, double* ref_pose7, int* ref_frame_id, double* last_rel16, double* rel_motion16,
                             int* next_frame_id, int* status, int* kf_every, int* frozen, int32_t* outlier_landmarks, int* n_outlier_landmarks,
                             uint8_t* prev_image, int image_step) {
    if (!h || s < 0 || s >= h->S || (prev_image && image_step < h->cols)) return MYSLAM_ERR_INVALID;
    hipStream_t st = h->stream;
    TrkArgs& a = h->a;
    TrkState hs;
    if (int rc = trk_fetch_state(h, s, hs)) return rc;
    const size_t fb = (size_t)s * h->cap, lb = (size_t)s * h->lmCap;
    if (feat_xy && hs.n_feat) MYSLAM_HIP_CHECK(hipMemcpyAsync(feat_xy, a.xy + fb * 2, sizeof(float) * 2 * hs.n_feat, hipMemcpyDeviceToHost, st));
    if (feat_landmark && hs.n_feat) MYSLAM_HIP_CHECK(hipMemcpyAsync(feat_landmark, a.lm + fb, sizeof(int32_t) * hs.n_feat, hipMemcpyDeviceToHost, st));
    if (landmark_pos && hs.n_lm) MYSLAM_HIP_CHECK(hipMemcpyAsync(landmark_pos, a.lmPos + lb * 3, sizeof(double) * 3 * hs.n_lm, hipMemcpyDeviceToHost, st));
    if (landmark_outlier && hs.n_lm) MYSLAM_HIP_CHECK(hipMemcpyAsync(landmark_outlier, a.lmOutl + lb, (size_t)hs.n_lm, hipMemcpyDeviceToHost, st));
    if (outlier_landmarks && hs.n_outl)
        MYSLAM_HIP_CHECK(hipMemcpyAsync(outlier_landmarks, a.outlList + fb * 2, sizeof(int32_t) * hs.n_outl, hipMemcpyDeviceToHost, st));
    std::vector<uint8_t> packed;
    if (prev_image) {
        if (!h->hasImage[s]) return MYSLAM_ERR_INVALID;
        packed.resize((size_t)h->rows * h->cols);
        MYSLAM_HIP_CHECK(hipMemcpyAsync(packed.data(), a.img + (size_t)hs.slot * a.imgSel + (size_t)s * a.imgBytes, packed.size(), hipMemcpyDeviceToHost, st));
    }
    MYSLAM_HIP_CHECK(hipStreamSynchronize(st));
    if (prev_image)
        for (int r = 0; r < h->rows; r++) memcpy(prev_image + (size_t)r * image_step, packed.data() + (size_t)r * h->cols, h->cols);
    if (n_feat) *n_feat = hs.n_feat;
    if (n_landmarks) *n_landmarks = hs.n_lm;
    if (ref_pose7) memcpy(ref_pose7, hs.ref_pose, sizeof(double) * 7);
    if (ref_frame_id) *ref_frame_id = hs.ref_frame_id;
    if (last_rel16) memcpy(last_rel16, hs.last_rel, sizeof(double) * 16);
    if (rel_motion16) memcpy(rel_motion16, hs.rel_motion, sizeof(double) * 16);
    if (next_frame_id) *next_frame_id = hs.next_frame_id;
    if (status) *status = hs.status;
    if (kf_every) *kf_every = hs.kf_every;
    if (frozen) *frozen = hs.frozen;
    if (n_outlier_landmarks) *n_outlier_landmarks = hs.n_outl;
    return MYSLAM_OK;
}

int myslam_tracker_step_batch(myslam_tracker* h, const uint8_t* d_left, int step, size_t stride, myslam_tracker_result* d_results) {
    if (!h || !d_left || image_args_bad(h, step, stride) || !d_results) return MYSLAM_ERR_INVALID;
    TrkArgs a = h->a;
    a.left = d_left; a.step = step; a.stride = stride; a.res = d_results;
    hipStream_t st = h->stream;
    const int S = h->S;
    const size_t pyrSel = (size_t)S * h->pyrBytes;
    hipLaunchKernelGGL(k_trk_head, trk_copy_grid(h), dim3(TRK_NT), 0, st, a);
    MYSLAM_HIP_CHECK(hipGetLastError());
    int rc;
    if ((rc = lk_bank_pyramid(h->lk, d_left, step, stride, h->d_pyr, S, a.sel, pyrSel))) return rc;
    if ((rc = lk_bank_track(h->lk, a.img, h->cols, a.imgBytes, h->d_pyr, S, a.sel, a.imgSel, pyrSel, a.p0, a.nxt, a.counts, h->cap, a.lkSt))) return rc;
    hipLaunchKernelGGL(k_trk_compact, dim3(S), dim3(TRK_NT), 0, st, a);
    MYSLAM_HIP_CHECK(hipGetLastError());
    if ((rc = pose_only_bank_launch(a.poPose, a.poPts, a.poObs, a.poCounts, S, h->cap, a.fx, a.fy, a.cx, a.cy, 5.991, 4, 10, a.poOutl, a.poInl, a.poStatus, st)))
        return rc;
    hipLaunchKernelGGL(k_trk_tail, dim3(S), dim3(TRK_NT), 0, st, a);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_tracker_debug_last_step(myslam_tracker* h, int s, float* p0, float* p1, float* tracked, uint8_t* lk_status, int* n) {
    if (!h || s < 0 || s >= h->S || !n) return MYSLAM_ERR_INVALID;
    hipStream_t st = h->stream;
    const TrkArgs& a = h->a;
    int32_t cnt = 0;
    int rc = copy_sync(&cnt, a.counts + s, sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (rc) return rc;
    const size_t fb = (size_t)s * h->cap;
    if (cnt > 0) {
        if (p0) MYSLAM_HIP_CHECK(hipMemcpyAsync(p0, a.p0 + fb * 2, sizeof(float) * 2 * cnt, hipMemcpyDeviceToHost, st));
        if (p1) MYSLAM_HIP_CHECK(hipMemcpyAsync(p1, a.p1 + fb * 2, sizeof(float) * 2 * cnt, hipMemcpyDeviceToHost, st));
        if (tracked) MYSLAM_HIP_CHECK(hipMemcpyAsync(tracked, a.nxt + fb * 2, sizeof(float) * 2 * cnt, hipMemcpyDeviceToHost, st));
        if (lk_status) MYSLAM_HIP_CHECK(hipMemcpyAsync(lk_status, a.lkSt + fb, (size_t)cnt, hipMemcpyDeviceToHost, st));
        MYSLAM_HIP_CHECK(hipStreamSynchronize(st));
    }
    *n = cnt;
    return MYSLAM_OK;
}

// ---- key-frame turns ----
int myslam_tracker_set_ids(myslam_tracker* h, int s, const int64_t* landmark_id, int n_landmarks, int64_t ref_kf_id, int64_t next_kf_id, int64_t next_mp_id) {
    if (!h || s < 0 || s >= h->S || n_landmarks < 0 || (n_landmarks > 0 && !landmark_id) || ref_kf_id < 0 || next_kf_id < 0 || next_mp_id < 0)
        return MYSLAM_ERR_INVALID;
    hipStream_t st = h->stream;
    TrkArgs& a = h->a;
    TrkState hs;
    if (int rc = trk_fetch_state(h, s, hs)) return rc;
    if (n_landmarks != hs.n_lm) return MYSLAM_ERR_INVALID;
    for (int l = 0; l < n_landmarks; l++) if (landmark_id[l] < 0 || landmark_id[l] >= next_mp_id) return MYSLAM_ERR_INVALID;
    const int64_t ids[3] = {ref_kf_id, next_kf_id, next_mp_id};
    const int32_t one = 1;
    if (n_landmarks) MYSLAM_HIP_CHECK(hipMemcpyAsync(a.lmId + (size_t)s * h->lmCap, landmark_id, sizeof(int64_t) * n_landmarks, hipMemcpyHostToDevice, st));
    MYSLAM_HIP_CHECK(hipMemcpyAsync(a.ids + (size_t)s * 3, ids, sizeof(ids), hipMemcpyHostToDevice, st));
    MYSLAM_HIP_CHECK(hipMemcpyAsync(&a.st[s].idsValid, &one, sizeof(one), hipMemcpyHostToDevice, st));
    MYSLAM_HIP_CHECK(hipStreamSynchronize(st));
    return MYSLAM_OK;
}

int myslam_tracker_get_ids(myslam_tracker* h, int s, int64_t* landmark_id, int* n_landmarks, int64_t* ref_kf_id, int64_t* next_kf_id, int64_t* next_mp_id,
                           int* valid) {
    if (!h || s < 0 || s >= h->S) return MYSLAM_ERR_INVALID;
    hipStream_t st = h->stream;
    TrkArgs& a = h->a;
    TrkState hs;
    if (int rc = trk_fetch_state(h, s, hs)) return rc;
    int64_t ids[3];
    if (landmark_id && hs.n_lm)
        MYSLAM_HIP_CHECK(hipMemcpyAsync(landmark_id, a.lmId + (size_t)s * h->lmCap, sizeof(int64_t) * hs.n_lm, hipMemcpyDeviceToHost, st));
    if (int rc = copy_sync(ids, a.ids + (size_t)s * 3, sizeof(ids), hipMemcpyDeviceToHost, st)) return rc;
    if (n_landmarks) *n_landmarks = hs.n_lm;
    if (ref_kf_id) *ref_kf_id = ids[0];
    if (next_kf_id) *next_kf_id = ids[1];
    if (next_mp_id) *next_mp_id = ids[2];
    if (valid) *valid = hs.idsValid;
    return MYSLAM_OK;
}

int myslam_tracker_keyframe_masks(myslam_tracker* h, uint8_t* d_masks, int step, size_t stride) {
    if (!h || !d_masks || image_args_bad(h, step, stride)) return MYSLAM_ERR_INVALID;
    if ((size_t)MASK_ROWS * h->cols > 65536) return MYSLAM_ERR_UNSUPPORTED;           // one block's band of the mask lives in LDS
    hipLaunchKernelGGL(k_kf_masks, dim3((h->rows + MASK_ROWS - 1) / MASK_ROWS, h->S), dim3(TRK_NT), (size_t)MASK_ROWS * h->cols, h->stream, h->a, d_masks, step,
                       stride);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_tracker_keyframe_launches(const myslam_tracker* h) {
    return h ? 3 + h->levels : MYSLAM_ERR_INVALID;
}

int myslam_tracker_keyframe_batch(myslam_tracker* h, const uint8_t* d_right, int step, size_t stride, const myslam_keypoint* d_new_kps,
                                  const int32_t* d_n_new, int kp_cap, double baseline, int64_t* d_new_kf_id, double* d_new_kf_pose, int64_t* d_feat_mp_id,
                                  double* d_feat_mp_pos, float* d_feat_uv, int32_t* d_feat_tag, uint8_t* d_feat_flags, int32_t* d_n_feat,
                                  int64_t* d_outlier_mp_id, int32_t* d_n_outlier_mp, float* d_right_xy, uint8_t* d_right_ok, int32_t* d_report) {
    KfArgs k;
    if (!kf_args(h, d_right, step, stride, d_new_kps, d_n_new, kp_cap, baseline, d_new_kf_id, d_new_kf_pose, d_feat_mp_id, d_feat_mp_pos, d_feat_uv, d_feat_tag,
                 d_feat_flags, d_n_feat, d_outlier_mp_id, d_n_outlier_mp, d_right_xy, d_right_ok, d_report, k))
        return MYSLAM_ERR_INVALID;
    return trk_run_turn(h, k, nullptr, 0);
}

// ---- StereoInit ----
int myslam_tracker_reset_stream(myslam_tracker* h, int s, int next_frame_id, int64_t next_kf_id, int64_t next_mp_id, int kf_every) {
    if (!h || s < 0 || s >= h->S || next_frame_id < 0 || next_kf_id < 0 || next_mp_id < 0 || kf_every < 0) return MYSLAM_ERR_INVALID;
    hipStream_t st = h->stream;
    TrkArgs& a = h->a;
    TrkState hs;
    if (int rc = trk_fetch_state(h, s, hs)) return rc;
    const int slot = hs.slot;                // the two image buffers keep their roles
    memset(&hs, 0, sizeof(hs));
    hs.ref_pose[3] = 1.0;
    for (int c = 0; c < 16; c += 5) hs.last_rel[c] = hs.rel_motion[c] = 1.0;
    hs.next_frame_id = next_frame_id; hs.status = TRK_INITING; hs.frozen = 1; hs.kf_every = kf_every; hs.slot = slot;
    const int64_t ids[3] = {0, next_kf_id, next_mp_id};
    MYSLAM_HIP_CHECK(hipMemcpyAsync(a.ids + (size_t)s * 3, ids, sizeof(ids), hipMemcpyHostToDevice, st));
    MYSLAM_HIP_CHECK(hipMemcpyAsync(a.st + s, &hs, sizeof(TrkState), hipMemcpyHostToDevice, st));
    MYSLAM_HIP_CHECK(hipStreamSynchronize(st));
    return MYSLAM_OK;
}

int myslam_tracker_init_masks(myslam_tracker* h, uint8_t* d_masks, int step, size_t stride) {
    if (!h || !d_masks || image_args_bad(h, step, stride)) return MYSLAM_ERR_INVALID;
    hipLaunchKernelGGL(k_init_masks, dim3((h->rows + MASK_ROWS - 1) / MASK_ROWS, h->S), dim3(TRK_NT), 0, h->stream, h->a, d_masks, step, stride);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_tracker_init_launches(const myslam_tracker* h) {
    return h ? 3 + 2 * h->levels : MYSLAM_ERR_INVALID;
}

int myslam_tracker_init_batch(myslam_tracker* h, const uint8_t* d_left, const uint8_t* d_right, int step, size_t stride, const myslam_keypoint* d_new_kps,
                              const int32_t* d_n_new, int kp_cap, double baseline, int init_good, int64_t* d_new_kf_id, double* d_new_kf_pose,
                              int64_t* d_feat_mp_id, double* d_feat_mp_pos, float* d_feat_uv, int32_t* d_feat_tag, uint8_t* d_feat_flags, int32_t* d_n_feat,
                              int64_t* d_outlier_mp_id, int32_t* d_n_outlier_mp, float* d_right_xy, uint8_t* d_right_ok, int32_t* d_report) {
    KfArgs k;
    if (!d_left || !kf_args(h, d_right, step, stride, d_new_kps, d_n_new, kp_cap, baseline, d_new_kf_id, d_new_kf_pose, d_feat_mp_id, d_feat_mp_pos, d_feat_uv,
                            d_feat_tag, d_feat_flags, d_n_feat, d_outlier_mp_id, d_n_outlier_mp, d_right_xy, d_right_ok, d_report, k))
        return MYSLAM_ERR_INVALID;
    return trk_run_turn(h, k, d_left, init_good);
}

int myslam_tracker_debug_last_turn(myslam_tracker* h, int s, float* left_xy, float* right_xy, uint8_t* right_ok, double* tri_xyz, uint8_t* tri_ok, int* n) {
    if (!h || s < 0 || s >= h->S || !n) return MYSLAM_ERR_INVALID;
    hipStream_t st = h->stream;
    const TrkArgs& a = h->a;
    int32_t cnt = 0;
    int rc = copy_sync(&cnt, a.kfCounts + s, sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (rc) return rc;
    const size_t fb = (size_t)s * h->cap;
    if (cnt > 0) {
        if (left_xy) MYSLAM_HIP_CHECK(hipMemcpyAsync(left_xy, a.kfP0 + fb * 2, sizeof(float) * 2 * cnt, hipMemcpyDeviceToHost, st));
        if (right_xy) MYSLAM_HIP_CHECK(hipMemcpyAsync(right_xy, a.kfNxt + fb * 2, sizeof(float) * 2 * cnt, hipMemcpyDeviceToHost, st));
        if (right_ok) MYSLAM_HIP_CHECK(hipMemcpyAsync(right_ok, a.kfSt + fb, (size_t)cnt, hipMemcpyDeviceToHost, st));
        if (tri_xyz) MYSLAM_HIP_CHECK(hipMemcpyAsync(tri_xyz, a.kfXyz + fb * 3, sizeof(double) * 3 * cnt, hipMemcpyDeviceToHost, st));
        if (tri_ok) MYSLAM_HIP_CHECK(hipMemcpyAsync(tri_ok, a.kfTok + fb, (size_t)cnt, hipMemcpyDeviceToHost, st));
        MYSLAM_HIP_CHECK(hipStreamSynchronize(st));
    }
    *n = cnt;
    return MYSLAM_OK;
}

int myslam_tracker_debug_freeze(myslam_tracker* h, int s, int why) {
    if (!h || s < 0 || s >= h->S || why < TRK_WHY_KEYFRAME || why > TRK_WHY_CAPACITY) return MYSLAM_ERR_INVALID;
    const int32_t w[2] = {1, why};
    hipStream_t st = h->stream;
    MYSLAM_HIP_CHECK(hipMemcpyAsync(&h->a.st[s].frozen, &w[0], sizeof(int32_t), hipMemcpyHostToDevice, st));
    MYSLAM_HIP_CHECK(hipMemcpyAsync(&h->a.st[s].why, &w[1], sizeof(int32_t), hipMemcpyHostToDevice, st));
    MYSLAM_HIP_CHECK(hipStreamSynchronize(st));
    return MYSLAM_OK;
}

int myslam_tracker_update_from_map_batch(myslam_tracker* h, const int64_t* d_kf_id, const double* d_kf_pose, const int32_t* d_n_kf, int kf_cap,
                                         const int64_t* d_mp_id, const double* d_mp_pos, const uint8_t* d_mp_outlier, const int32_t* d_n_mp, int mp_cap) {
    return tracker_update_from_map_launch(h, d_kf_id, d_kf_pose, d_n_kf, kf_cap, d_mp_id, d_mp_pos, d_mp_outlier, d_n_mp, mp_cap, nullptr);
}

}  // extern "C"

void myslam_hip::tracker_shape(const myslam_tracker* h, hipStream_t* stream, int* streams, int* cap) { *stream = h->stream; *streams = h->S; *cap = h->cap; }

int myslam_hip::tracker_update_from_map_launch(myslam_tracker* h, const int64_t* d_kf_id, const double* d_kf_pose, const int32_t* d_n_kf, int kf_cap,
                                               const int64_t* d_mp_id, const double* d_mp_pos, const uint8_t* d_mp_outlier, const int32_t* d_n_mp, int mp_cap,
                                               const int32_t* d_gate) {
    if (!h || !d_kf_id || !d_kf_pose || !d_n_kf || kf_cap < 1 || !d_mp_id || !d_mp_pos || !d_mp_outlier || !d_n_mp || mp_cap < 1) return MYSLAM_ERR_INVALID;
    const BeTablesRead g{d_kf_id, d_kf_pose, d_n_kf, d_mp_id, d_mp_pos, d_mp_outlier, d_n_mp, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, kf_cap, mp_cap, 0};
    hipLaunchKernelGGL(k_kf_update, dim3(h->S), dim3(TRK_NT), 0, h->stream, h->a, g, d_gate);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

extern "C" {

int myslam_tracker_clear_links_batch(myslam_tracker* h, const int64_t* d_kf_id, const int32_t* d_tag, const int32_t* d_n, int list_cap, int32_t* d_n_cleared) {
    if (!h || !d_kf_id || !d_tag || !d_n || list_cap <= 0) return MYSLAM_ERR_INVALID;
    hipLaunchKernelGGL(k_trk_clear_links, dim3(h->S), dim3(TRK_NT), 0, h->stream, h->a, d_kf_id, d_tag, d_n, list_cap, d_n_cleared);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_tracker_relink_batch(myslam_tracker* h, const int64_t* d_kf_id, const int32_t* d_tag, const int32_t* d_slot, const int32_t* d_n, int list_cap,
                                const myslam_map* map, int32_t* d_n_relinked, int32_t* d_status) {
    if (!h || !d_kf_id || !d_tag || !d_slot || !d_n || list_cap <= 0 || !map || !d_status) return MYSLAM_ERR_INVALID;
    myslam_map_tables mv;
    if (myslam_map_view(map, &mv) != MYSLAM_OK) return MYSLAM_ERR_INVALID;
    if (h->S > mv.max_batch) return MYSLAM_ERR_INVALID;                       // item s of the map is stream s
    const TrkRelink r{d_kf_id, d_tag, d_slot, d_n, list_cap, mv.mp_id, mv.mp_pos, mv.mp_state, mv.n_mp, mv.point_cap, d_n_relinked, d_status};
    hipLaunchKernelGGL(k_trk_relink, dim3(h->S), dim3(TRK_NT), 0, h->stream, h->a, r);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_tracker_set_image_batch(myslam_tracker* h, const uint8_t* d_imgs, int step, size_t stride, const uint8_t* d_select) {
    if (!h || !d_imgs || !d_select || image_args_bad(h, step, stride)) return MYSLAM_ERR_INVALID;
    const TrkArgs& a = h->a;
    hipLaunchKernelGGL(k_kf_set_image, trk_copy_grid(h), dim3(TRK_NT), 0, h->stream, a, d_imgs, step, stride,
                       d_select);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return lk_bank_pyramid(h->lk, d_imgs, step, stride, h->d_pyr, h->S, a.kfSel, (size_t)h->S * h->pyrBytes);
}

}  // extern "C"
