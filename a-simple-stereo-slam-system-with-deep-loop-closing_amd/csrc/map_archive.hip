// map_archive.hip — Map::mmAllKeyFrames / mmAllMapPoints (reference src/map.cpp: InsertKeyFrame, InsertMapPoint, RemoveMapPoint, AddOutlierMapPoint,
// RemoveAllOutlierMapPoints) and KeyFrame::mpLastKF / mRelativePoseToLastKF (include/myslam/keyframe.h, set in src/frontend.cpp:424-447) as device
// tables per stream, laid out as the tables myslam_loop_correct_batch reads (src/loopclosing.cpp:560-562, :568-602, :612-641).
//   k_map_update         one workgroup per map, after each back-end call: appends what is new in the back end's tables, keeps the erased / outlier state
//                        of every point, refreshes poses, positions and first observers, and remembers which archive slot each back-end row had;
//   k_map_loop_inputs    the per-loop index inputs of myslam_loop_correct_batch;
//   k_map_write_backend  the corrected poses and positions back into the back end's rows;
//   k_map_feature_slots  map-point id -> archive slot per feature (myslam_loop_store_put_batch's d_feat_landmark);
//   k_map_filter_landmarks  the links of a gathered table to points erased since (one workgroup per item, a block scan for its count);
//   k_map_relink         the points a re-link plan merged away are erased (state 2), one workgroup per item.
// Ids ascend in every table, so a row is found by binary search (sorted_rows.h) and a new row's slot is a closed form: no scans, no atomics; an item's bytes depend
// neither on its slot nor on its neighbours.  The edge measurement uses se3_chain.h (chain.py's arithmetic, built with -ffp-contract=off).
// See include/myslam_hip.h for the contract.
#include "dev_tables.h"
#include "se3_chain.h"

namespace myslam_hip {

constexpr int MA_NT = 256;
constexpr int MA_MAX_BE_KF = MYSLAM_BA_MAX_WINDOW_POSES;

struct MaTables {                       // the archive, strided by the caps; snap: archive slot of every back-end map-point row as of the last update
    int64_t* kf_id; double* kf_pose; int32_t* n_kf;
    int32_t* edge_v0; int32_t* edge_v1; double* meas; int32_t* n_edges;
    int64_t* mp_id; double* mp_pos; int32_t* mp_first_kf; uint8_t* mp_state; int32_t* n_mp;
    int32_t* snap; int32_t* n_snap;
    // what keeps the first observer exact once key-frames leave the window (a row with obs_kf = -1 no longer says whose it is):
    int32_t* gone_kf;                   // per point: lowest archive row among its observers that left the window, -1 = none
    uint16_t* win_mask;                 // per point: bit k = it had a row on row k of the back end's key-frame table at the last update
    int32_t* win_kf; int32_t* n_win;    // per item: archive row of every row of that key-frame table (MA_MAX_BE_KF slots), and their number
    int kf_cap, edge_cap, point_cap, be_mp_cap;
    struct Item {
        int64_t* kf_id; double* kf_pose; int32_t* edge_v0; int32_t* edge_v1; double* meas;
        int64_t* mp_id; double* mp_pos; int32_t* mp_first_kf; uint8_t* mp_state; int32_t* snap;
        int32_t* gone_kf; uint16_t* win_mask; int32_t* win_kf;
    };
    __device__ __forceinline__ Item item(int b) const {
        const size_t k = (size_t)b * kf_cap, e = (size_t)b * edge_cap, p = (size_t)b * point_cap;
        return {kf_id + k, kf_pose + k * 7, edge_v0 + e, edge_v1 + e, meas + e * 7, mp_id + p, mp_pos + p * 3, mp_first_kf + p, mp_state + p,
                snap + (size_t)b * be_mp_cap, gone_kf + p, win_mask + p, win_kf + (size_t)b * MA_MAX_BE_KF};
    }
};

// The back end's tables as myslam_backend_* leaves them are dev_tables.h's view (BeTablesRead; BeTablesPose where poses and positions go back), with
// nullptr for every column a call does not take: no kernel here reads mp_outlier, obs_uv or obs_tag.

struct MaUpdateIn {
    int mode; const int32_t* be_status; const int64_t* outlier_id; const int32_t* n_outlier; int outlier_cap; const uint8_t* mp_report;
    const double* solve_pts; const int32_t* solve_slot;     // myslam_map_attach_solve: the solve's positions by landmark slot, the slot of every INPUT row
};

__global__ __launch_bounds__(MA_NT) void k_map_update(MaTables A, BeTablesRead B, MaUpdateIn U, int32_t* status) {
    __shared__ int s_bad;
    __shared__ int s_kfrow[MA_MAX_BE_KF];                                   // archive row of every back-end key-frame row
    __shared__ int s_prev[MA_MAX_BE_KF];                                    // the same at the last update, and which of those rows have left since
    __shared__ unsigned s_left;
    const int b = blockIdx.x, t = threadIdx.x;
    const int bst = U.be_status[b];
    const bool ins = U.mode == MYSLAM_MAP_AFTER_INSERT;
    if (bst != 0) {                                                         // a refused insert; EMPTY or an error: the reference returns before the removal
        if (t == 0) status[b] = MYSLAM_MAP_SKIPPED;
        return;
    }
    const int nk = B.n_kf[b], nm = B.n_mp[b], no = B.n_obs[b];
    const int aK = A.n_kf[b], aE = A.n_edges[b], aM = A.n_mp[b], nsnap = A.n_snap[b], nwin = A.n_win[b];
    const int nx = (ins && U.n_outlier) ? U.n_outlier[b] : 0;
    if (nk < 0 || nk > B.kf_cap || nm < 0 || nm > B.mp_cap || no < 0 || no > B.obs_cap || nx < 0 || nx > U.outlier_cap || aK < 0 || aK > A.kf_cap ||
        aE < 0 || aE > A.edge_cap || aM < 0 || aM > A.point_cap || nsnap < 0 || nsnap > A.be_mp_cap || nwin < 0 || nwin > MA_MAX_BE_KF) {                        // uniform
        if (t == 0) status[b] = MYSLAM_ERR_INVALID;
        return;
    }
    const auto a = A.item(b);
    const auto be = B.item(b);

    // ---- decide: where every back-end row lives in the archive, what is new ----
    const int64_t last_kf = aK ? a.kf_id[aK - 1] : INT64_MIN, last_mp = aM ? a.mp_id[aM - 1] : INT64_MIN;
    const int k0 = aK ? lower_row(be.kf_id, nk, last_kf + 1) : 0;            // back-end key-frame rows from k0 on are above the archive's last id
    const int m0 = aM ? lower_row(be.mp_id, nm, last_mp + 1) : 0;
    const int newK = nk - k0, newM = nm - m0;
    if (t == 0) { s_bad = 0; s_left = 0u; }
    if (t < nwin) s_prev[t] = a.win_kf[t];
    __syncthreads();
    bool bad = false;
    if (t < nk) {
        const int r = t < k0 ? find_row(a.kf_id, aK, be.kf_id[t]) : aK + (t - k0);
        s_kfrow[t] = r;
        bad |= r < 0;                                                       // a key-frame id below the archive's last that it never saw
    }
    for (int m = t; m < m0; m += MA_NT) bad |= find_row(a.mp_id, aM, be.mp_id[m]) < 0;      // an unarchived id below the archive's last
    if (!ins) bad |= newK > 0 || newM > 0 || nm > nsnap;                    // an optimise adds nothing
    if (bad) s_bad = 1;
    __syncthreads();
    if (s_bad) { if (t == 0) status[b] = MYSLAM_ERR_INVALID; return; }
    const int newE = newK - ((aK == 0 && newK > 0) ? 1 : 0);                // every appended row but the archive's first gets an edge
    if (aK + newK > A.kf_cap || aE + newE > A.edge_cap || aM + newM > A.point_cap) {          // uniform
        if (t == 0) status[b] = MYSLAM_ERR_CAPACITY;
        return;
    }

    // ---- from here on the item is written ----
    if (ins) {
        // InsertKeyFrame (map.cpp), mpLastKF / mRelativePoseToLastKF (frontend.cpp:424-447): meas = p7(T(new) * T(prev)^-1), prev = the archive's pose
        if (t < newK) {
            const int r = aK + t;
            const double* pn = be.kf_pose + 7 * (k0 + t);
            a.kf_id[r] = be.kf_id[k0 + t];
            for (int k = 0; k < 7; k++) a.kf_pose[7 * r + k] = pn[k];
            if (r > 0) {
                const double* pp = t == 0 ? a.kf_pose + 7 * (aK - 1) : be.kf_pose + 7 * (k0 + t - 1);
                double Tn[16], Tp[16], Ti[16], Tm[16], m7[7];
                se3_T_of(pn, Tn); se3_T_of(pp, Tp); se3_inv(Tp, Ti); se3_mm(Tn, Ti, Tm); se3_p7_of(Tm, m7);
                const int e = aE + (r - 1) - (aK > 0 ? aK - 1 : 0);
                a.edge_v0[e] = r; a.edge_v1[e] = r - 1;
                for (int k = 0; k < 7; k++) a.meas[7 * e + k] = m7[k];
            }
        }
        // InsertMapPoint: ids above the archive's last, in the table's order
        for (int j = t; j < newM; j += MA_NT) {
            const int s = aM + j;
            a.mp_id[s] = be.mp_id[m0 + j]; a.mp_state[s] = 0; a.mp_first_kf[s] = -1; a.gone_kf[s] = -1; a.win_mask[s] = 0;
        }
        __syncthreads();                                                    // the outlier ids may name a row appended above; t == 0's pose of row aK - 1 is read
        // AddOutlierMapPoint (map.cpp): alive points only
        for (int j = t; j < nx; j += MA_NT) {
            const int s = find_row(a.mp_id, aM + newM, U.outlier_id[(size_t)b * U.outlier_cap + j]);
            if (s >= 0 && a.mp_state[s] == 0) a.mp_state[s] = 1;
        }
    } else {
        // RemoveAllOutlierMapPoints (map.cpp): the optimiser's erased rows by INPUT row = the snapshot's row, then the whole outlier list
        for (int m = t; m < nsnap; m += MA_NT)
            if (U.mp_report[(size_t)b * B.mp_cap + m] == 2) {
                const int s = a.snap[m];
                if (s >= 0 && s < aM) a.mp_state[s] = 2;
            }
        // SetPos reaches every vertex (backend.cpp:259-261) before RemoveOldActiveMapPoints (map.cpp:126-140): a point that leaves the table alive with
        // this optimise takes the solve's position, which the compacted table no longer holds
        if (U.solve_pts)
            for (int m = t; m < nsnap; m += MA_NT)
                if (U.mp_report[(size_t)b * B.mp_cap + m] == 1) {
                    const int s = a.snap[m], slot = U.solve_slot[(size_t)b * B.mp_cap + m];
                    if (s >= 0 && s < aM && slot >= 0 && slot < B.mp_cap) {
                        const double* p = U.solve_pts + ((size_t)b * B.mp_cap + slot) * 3;
                        a.mp_pos[3 * s] = p[0]; a.mp_pos[3 * s + 1] = p[1]; a.mp_pos[3 * s + 2] = p[2];
                    }
                }
        __syncthreads();
        for (int s = t; s < aM; s += MA_NT)
            if (a.mp_state[s] == 1) a.mp_state[s] = 2;
    }
    __syncthreads();

    // ---- observers that left the window since the last update: the points of the table as it was then (the old snapshot) that had a row on them ----
    if (t < nwin) {
        bool here = false;
        for (int k = 0; k < nk; k++) here |= s_kfrow[k] == s_prev[t];
        if (!here) atomicOr(&s_left, 1u << t);                              // LDS
    }
    __syncthreads();
    const unsigned left = s_left;
    for (int m = t; m < nsnap; m += MA_NT) {
        const int s = a.snap[m];
        if (s < 0 || s >= aM) continue;
        int g = a.gone_kf[s];
        for (unsigned w = left & a.win_mask[s]; w; w &= w - 1) {
            const int row = s_prev[__ffs(w) - 1];
            g = g < 0 ? row : min(g, row);
        }
        if (g >= 0) { a.gone_kf[s] = g; a.mp_first_kf[s] = g; }            // a point that is leaving keeps only such rows: the lowest of them is its front
    }
    __syncthreads();

    // ---- refresh: poses, positions, first observers; the snapshot ----
    for (int i = t; i < 7 * nk; i += MA_NT) a.kf_pose[7 * s_kfrow[i / 7] + i % 7] = be.kf_pose[i];
    for (int m = t; m < nm; m += MA_NT) {
        const int s = m < m0 ? lower_row(a.mp_id, aM, be.mp_id[m]) : aM + (m - m0);
        a.mp_pos[3 * s] = be.mp_pos[3 * m]; a.mp_pos[3 * s + 1] = be.mp_pos[3 * m + 1]; a.mp_pos[3 * s + 2] = be.mp_pos[3 * m + 2];
        // GetObservations().front()->mpKF: both observation lists are in key-frame order, so the front is the lowest archive row among the rows whose
        // key-frame is in the window (the first of them) and the observers that left it
        int first = a.gone_kf[s];
        unsigned mask = 0;
        for (int r = lower_row(be.obs_mp, no, m); r < no && be.obs_mp[r] == m; r++) {
            const int k = be.obs_kf[r];
            if (k < 0 || k >= nk) continue;
            if (!mask) first = first < 0 ? s_kfrow[k] : min(first, s_kfrow[k]);
            mask |= 1u << k;
        }
        if (first >= 0) a.mp_first_kf[s] = first;
        a.win_mask[s] = (uint16_t)mask;
        a.snap[m] = s;
    }
    if (t < nk) a.win_kf[t] = s_kfrow[t];
    if (t == 0) {
        A.n_kf[b] = aK + newK; A.n_edges[b] = aE + newE; A.n_mp[b] = aM + newM; A.n_snap[b] = nm; A.n_win[b] = nk;
        status[b] = MYSLAM_MAP_UPDATED;
    }
}

struct MaLoopIn { const int64_t* cur_kf_id; const uint64_t* loop_kf_id; const int32_t* detect_status; int active_cap; };
struct MaLoopOut { int32_t* active; int32_t* n_active; int32_t* cur; int32_t* loop; int32_t* first_active; int32_t* first_kf; int32_t* n_points; };

// grid (point_cap / MA_NT rounded up, batch): block (c, b) writes the point rows [c MA_NT, (c + 1) MA_NT) of item b, block (0, b) also the key-frame side
__global__ __launch_bounds__(MA_NT) void k_map_loop_inputs(MaTables A, BeTablesRead B, MaLoopIn I, MaLoopOut O) {
    const int b = blockIdx.y, c = blockIdx.x, t = threadIdx.x;
    const int64_t cur_id = I.cur_kf_id[b];
    const int aK = clamped_count(A.n_kf, b, A.kf_cap), aM = clamped_count(A.n_mp, b, A.point_cap);
    const int nk = min(clamped_count(B.n_kf, b, B.kf_cap), I.active_cap), nm = clamped_count(B.n_mp, b, B.mp_cap), no = clamped_count(B.n_obs, b, B.obs_cap);
    if (cur_id < 0) {                                                       // no key-frame this turn: myslam_loop_correct_batch skips the item on its verify status
        if (c == 0 && t == 0) { O.n_active[b] = 0; O.cur[b] = -1; O.loop[b] = -1; O.n_points[b] = 0; }
        return;
    }
    const auto a = A.item(b);
    const auto be = B.item(b);
    if (c == 0 && t < nk) O.active[(size_t)b * I.active_cap + t] = find_row(a.kf_id, aK, be.kf_id[t]);       // GetActiveKeyFrames(), :560
    if (c == 0 && t == 0) {
        O.n_active[b] = nk; O.n_points[b] = aM;
        O.cur[b] = find_row(a.kf_id, aK, cur_id);
        const uint64_t lid = I.loop_kf_id[b];
        O.loop[b] = (I.detect_status[b] == MYSLAM_LOOP_DETECT_CANDIDATE && lid <= (uint64_t)INT64_MAX) ? find_row(a.kf_id, aK, (int64_t)lid) : -1;
    }
    const int s = c * MA_NT + t;
    if (s < aM) {
        int fa = -1;
        const int m = find_row(be.mp_id, nm, a.mp_id[s]);
        if (m >= 0)                                                         // GetActiveObservations().front(): the first ACTIVE row of the segment
            for (int r = lower_row(be.obs_mp, no, m); r < no && be.obs_mp[r] == m; r++)
                if (be.obs_flags[r] & MYSLAM_BACKEND_OBS_ACTIVE) { fa = be.obs_kf[r]; break; }
        O.first_active[(size_t)b * A.point_cap + s] = fa;
        O.first_kf[(size_t)b * A.point_cap + s] = a.mp_state[s] == 2 ? -1 : a.mp_first_kf[s];     // :625-629: an erased point is skipped
    }
}

__global__ __launch_bounds__(MA_NT) void k_map_write_backend(MaTables A, BeTablesPose B, const uint8_t* select) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (select && !select[b]) return;
    const int aK = clamped_count(A.n_kf, b, A.kf_cap), aM = clamped_count(A.n_mp, b, A.point_cap);
    const int nk = clamped_count(B.n_kf, b, B.kf_cap), nm = clamped_count(B.n_mp, b, B.mp_cap);
    const auto a = A.item(b);
    const auto be = B.item(b);
    for (int i = t; i < 7 * nk; i += MA_NT) {
        const int r = find_row(a.kf_id, aK, be.kf_id[i / 7]);
        if (r >= 0) be.kf_pose[i] = a.kf_pose[7 * r + i % 7];
    }
    for (int m = t; m < nm; m += MA_NT) {
        const int s = find_row(a.mp_id, aM, be.mp_id[m]);
        double* dst = be.mp_pos + 3 * m;
        if (s >= 0) { dst[0] = a.mp_pos[3 * s]; dst[1] = a.mp_pos[3 * s + 1]; dst[2] = a.mp_pos[3 * s + 2]; }
    }
}

__global__ __launch_bounds__(MA_NT) void k_map_feature_slots(MaTables A, const int64_t* feat_mp_id, const int32_t* n_feat, int feat_cap, int32_t* feat_landmark) {
    const int b = blockIdx.y, f = blockIdx.x * MA_NT + threadIdx.x;
    const int nf = clamped_count(n_feat, b, feat_cap);
    if (f >= nf) return;
    const int aM = clamped_count(A.n_mp, b, A.point_cap);
    const auto a = A.item(b);
    const int64_t id = feat_mp_id[(size_t)b * feat_cap + f];
    const int s = id < 0 ? -1 : find_row(a.mp_id, aM, id);
    feat_landmark[(size_t)b * feat_cap + f] = (s >= 0 && a.mp_state[s] != 2) ? s : -1;
}

// One workgroup per item over the whole row of a gathered feature -> landmark table (the matcher indexes it by class_id < feat_cap, without a count):
// an entry that names an erased point becomes -1, as mpMapPoint.lock() of ComputeCorrectPose (src/loopclosing.cpp:218-237) finds it once
// Map::RemoveAllOutlierMapPoints (src/map.cpp:166-175) dropped the point.  Every other value keeps its bits.
__global__ __launch_bounds__(MA_NT) void k_map_filter_landmarks(MaTables A, int32_t* feat_landmark, int feat_cap, int32_t* n_dropped) {
    __shared__ int s_w[MA_NT / WAVE];
    const int b = blockIdx.x, t = threadIdx.x;
    const int aM = clamped_count(A.n_mp, b, A.point_cap);
    const uint8_t* const state = A.mp_state + (size_t)b * A.point_cap;
    int32_t* const row = feat_landmark + (size_t)b * feat_cap;
    int dropped = 0;
    for (int base = 0; base < feat_cap; base += MA_NT) {                    // uniform
        const int f = base + t;
        bool drop = false;
        if (f < feat_cap) {
            const int e = row[f];
            drop = e >= 0 && e < aM && state[e] == 2;
            if (drop) row[f] = -1;
        }
        int tot;
        (void)block_rank<MA_NT / WAVE>(drop, s_w, tot);
        dropped += tot;
    }
    if (t == 0 && n_dropped) n_dropped[b] = dropped;
}

// One workgroup per item: Map::RemoveMapPoint (src/map.cpp:144-155) for every point the re-link plan merged away (src/loopclosing.cpp:526).  The
// list is validated whole before the first state is written; targets keep their state, no position is touched.
__global__ __launch_bounds__(MA_NT) void k_map_relink(MaTables A, const int32_t* merge, const int32_t* n_merge, int merge_cap, const int32_t* plan_status,
                                                      int32_t* status) {
    __shared__ int s_bad;
    const int b = blockIdx.x, t = threadIdx.x;
    if (plan_status[b] != MYSLAM_RELINK_DONE) {                             // uniform: skipped or refused, nothing was merged
        if (t == 0) status[b] = MYSLAM_MAP_SKIPPED;
        return;
    }
    const int n = n_merge[b], aM = A.n_mp[b];
    const int32_t* const list = merge + (size_t)b * merge_cap * 2;
    uint8_t* const state = A.mp_state + (size_t)b * A.point_cap;
    if (t == 0) s_bad = 0;
    __syncthreads();
    bool bad = n < 0 || n > merge_cap || aM < 0 || aM > A.point_cap;
    if (!bad)
        for (int i = t; i < n; i += MA_NT) {
            const int from = list[2 * i], to = list[2 * i + 1];
            bad |= from < 0 || from >= aM || to < 0 || to >= aM || from == to;
        }
    if (bad) s_bad = 1;
    __syncthreads();
    if (s_bad) {                                                            // uniform; every byte kept
        if (t == 0) status[b] = MYSLAM_ERR_INVALID;
        return;
    }
    for (int i = t; i < n; i += MA_NT) state[list[2 * i]] = 2;
    if (t == 0) status[b] = MYSLAM_MAP_UPDATED;
}

}  // namespace myslam_hip

using namespace myslam_hip;

struct myslam_map {
    int max_batch = 0;
    hipStream_t stream = nullptr;
    MaTables t{};
    BufSet mem;                         // owns every block that `t` names
    const double* solve_pts = nullptr;  // myslam_map_attach_solve: the back end's, not owned
    const int32_t* solve_slot = nullptr;
};

// host <-> one item's rows, complete on return, on the calling thread's non-blocking stream (common.h); the caller has waited for the handle's stream
static int ma_copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    if (!dst || !src || bytes == 0) return MYSLAM_OK;
    const hipStream_t st = host_call_stream();
    if (!st) return MYSLAM_ERR_HIP;
    return copy_sync(dst, src, bytes, kind, st);
}

static bool ma_backend_args_bad(const myslam_map* h, int be_kf_cap, int be_mp_cap) {
    return be_kf_cap < 1 || be_kf_cap > MA_MAX_BE_KF || be_mp_cap != h->t.be_mp_cap;
}

extern "C" {

int myslam_map_create(myslam_map** out, int max_batch, int kf_cap, int edge_cap, int point_cap, int backend_mp_cap) {
    if (!out || max_batch < 1 || max_batch > 65535 || kf_cap < 1 || edge_cap < 1 || point_cap < 1 || backend_mp_cap < 1) return MYSLAM_ERR_INVALID;
    if (kf_cap > (1 << 24) || edge_cap > (1 << 24) || point_cap > (1 << 26) || backend_mp_cap > (1 << 24)) return MYSLAM_ERR_CAPACITY;
    if (need_device()) return MYSLAM_ERR_HIP;
    myslam_map* h = new myslam_map();
    h->max_batch = max_batch;
    MaTables& t = h->t;
    t.kf_cap = kf_cap; t.edge_cap = edge_cap; t.point_cap = point_cap; t.be_mp_cap = backend_mp_cap;
    const size_t B = (size_t)max_batch, K = (size_t)kf_cap, E = (size_t)edge_cap, P = (size_t)point_cap, M = (size_t)backend_mp_cap;
    auto own = [&](auto*& p, size_t n) { return h->mem.own(p, n, MYSLAM_ERR_CAPACITY); };
    int rc;
    if ((rc = own(t.kf_id, B * K)) || (rc = own(t.kf_pose, B * K * 7)) || (rc = own(t.n_kf, B)) || (rc = own(t.edge_v0, B * E)) || (rc = own(t.edge_v1, B * E)) ||
        (rc = own(t.meas, B * E * 7)) || (rc = own(t.n_edges, B)) || (rc = own(t.mp_id, B * P)) || (rc = own(t.mp_pos, B * P * 3)) ||
        (rc = own(t.mp_first_kf, B * P)) || (rc = own(t.mp_state, B * P)) || (rc = own(t.n_mp, B)) || (rc = own(t.snap, B * M)) || (rc = own(t.n_snap, B)) ||
        (rc = own(t.gone_kf, B * P)) || (rc = own(t.win_mask, B * P)) || (rc = own(t.win_kf, B * MA_MAX_BE_KF)) || (rc = own(t.n_win, B))) {
        delete h;
        return rc;
    }
    const std::vector<int32_t> zeros(B, 0);                                 // every map starts empty
    for (int32_t* p : {t.n_kf, t.n_edges, t.n_mp, t.n_snap, t.n_win})
        if ((rc = upload_table(p, zeros.data(), B * sizeof(int32_t)))) { delete h; return rc; }
    *out = h;
    return MYSLAM_OK;
}

int myslam_map_destroy(myslam_map* h) {
    if (!h) return MYSLAM_ERR_INVALID;
    (void)hipStreamSynchronize(h->stream);
    delete h;
    return MYSLAM_OK;
}

int myslam_map_set_stream(myslam_map* h, void* hip_stream) {
    if (!h) return MYSLAM_ERR_INVALID;
    h->stream = (hipStream_t)hip_stream;
    return MYSLAM_OK;
}

int myslam_map_view(const myslam_map* h, myslam_map_tables* out) {
    if (!h || !out) return MYSLAM_ERR_INVALID;
    const MaTables& t = h->t;
    *out = {t.kf_id, t.kf_pose, t.n_kf, t.edge_v0, t.edge_v1, t.meas, t.n_edges, t.mp_id, t.mp_pos, t.mp_first_kf, t.mp_state, t.n_mp,
            h->max_batch, t.kf_cap, t.edge_cap, t.point_cap, t.be_mp_cap};
    return MYSLAM_OK;
}

int myslam_map_launches_per_update(const myslam_map* h) { return h ? 1 : MYSLAM_ERR_INVALID; }

int myslam_map_attach_solve(myslam_map* h, const double* d_solve_points, const int32_t* d_solve_mp_slot) {
    if (!h || (d_solve_points == nullptr) != (d_solve_mp_slot == nullptr)) return MYSLAM_ERR_INVALID;
    h->solve_pts = d_solve_points; h->solve_slot = d_solve_mp_slot;
    return MYSLAM_OK;
}

int myslam_map_load(myslam_map* h, int item, const int64_t* kf_id, const double* kf_pose, int n_kf, const int32_t* edge_v0, const int32_t* edge_v1,
                    const double* meas, int n_edges, const int64_t* mp_id, const double* mp_pos, const int32_t* mp_first_kf, const uint8_t* mp_state, int n_mp,
                    const int32_t* snapshot, int n_snapshot, const int32_t* mp_gone_kf, const uint16_t* mp_win_mask, const int32_t* win_kf, int n_win) {
    if (!h || item < 0 || item >= h->max_batch) return MYSLAM_ERR_INVALID;
    const MaTables& t = h->t;
    if (n_kf < 0 || n_edges < 0 || n_mp < 0 || n_snapshot < 0 || n_win < 0) return MYSLAM_ERR_INVALID;
    if (n_kf > t.kf_cap || n_edges > t.edge_cap || n_mp > t.point_cap || n_snapshot > t.be_mp_cap || n_win > MA_MAX_BE_KF) return MYSLAM_ERR_CAPACITY;
    if ((n_kf && (!kf_id || !kf_pose)) || (n_edges && (!edge_v0 || !edge_v1 || !meas)) || (n_mp && (!mp_id || !mp_pos || !mp_first_kf || !mp_state)) ||
        (n_snapshot && !snapshot) || (n_win && !win_kf))
        return MYSLAM_ERR_INVALID;
    for (int i = 1; i < n_kf; i++) if (kf_id[i - 1] >= kf_id[i]) return MYSLAM_ERR_INVALID;
    for (int i = 1; i < n_mp; i++) if (mp_id[i - 1] >= mp_id[i]) return MYSLAM_ERR_INVALID;
    for (int e = 0; e < n_edges; e++)
        if (edge_v0[e] < 0 || edge_v0[e] >= n_kf || edge_v1[e] < 0 || edge_v1[e] >= n_kf || edge_v0[e] == edge_v1[e]) return MYSLAM_ERR_INVALID;
    for (int i = 0; i < n_mp; i++) if (mp_first_kf[i] < -1 || mp_first_kf[i] >= n_kf || mp_state[i] > 2) return MYSLAM_ERR_INVALID;
    for (int i = 0; i < n_snapshot; i++) if (snapshot[i] < 0 || snapshot[i] >= n_mp) return MYSLAM_ERR_INVALID;
    for (int i = 0; i < n_win; i++) if (win_kf[i] < 0 || win_kf[i] >= n_kf) return MYSLAM_ERR_INVALID;
    for (int i = 0; i < n_mp && mp_gone_kf; i++) if (mp_gone_kf[i] < -1 || mp_gone_kf[i] >= n_kf) return MYSLAM_ERR_INVALID;
    for (int i = 0; i < n_mp && mp_win_mask; i++) if (mp_win_mask[i] >> n_win) return MYSLAM_ERR_INVALID;
    const std::vector<int32_t> no_gone(mp_gone_kf ? 0 : n_mp, -1);          // NULL: no observer has left, no row in the window
    const std::vector<uint16_t> no_mask(mp_win_mask ? 0 : n_mp, 0);
    if (stream_is_capturing(h->stream)) return MYSLAM_ERR_UNSUPPORTED;
    MYSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    const size_t b = (size_t)item, K = (size_t)t.kf_cap, E = (size_t)t.edge_cap, P = (size_t)t.point_cap, M = (size_t)t.be_mp_cap;
    const int32_t counts[5] = {n_kf, n_edges, n_mp, n_snapshot, n_win};
    const auto up = [](void* dst, const void* src, size_t bytes) { return ma_copy(dst, src, bytes, hipMemcpyHostToDevice); };
    int rc;
    if ((rc = up(t.kf_id + b * K, kf_id, n_kf * sizeof(int64_t))) || (rc = up(t.kf_pose + b * K * 7, kf_pose, n_kf * 7 * sizeof(double))) ||
        (rc = up(t.edge_v0 + b * E, edge_v0, n_edges * sizeof(int32_t))) || (rc = up(t.edge_v1 + b * E, edge_v1, n_edges * sizeof(int32_t))) ||
        (rc = up(t.meas + b * E * 7, meas, n_edges * 7 * sizeof(double))) || (rc = up(t.mp_id + b * P, mp_id, n_mp * sizeof(int64_t))) ||
        (rc = up(t.mp_pos + b * P * 3, mp_pos, n_mp * 3 * sizeof(double))) || (rc = up(t.mp_first_kf + b * P, mp_first_kf, n_mp * sizeof(int32_t))) ||
        (rc = up(t.mp_state + b * P, mp_state, n_mp)) || (rc = up(t.snap + b * M, snapshot, n_snapshot * sizeof(int32_t))) ||
        (rc = up(t.n_kf + b, &counts[0], 4)) || (rc = up(t.n_edges + b, &counts[1], 4)) || (rc = up(t.n_mp + b, &counts[2], 4)) ||
        (rc = up(t.n_snap + b, &counts[3], 4)) || (rc = up(t.gone_kf + b * P, mp_gone_kf ? mp_gone_kf : no_gone.data(), n_mp * sizeof(int32_t))) ||
        (rc = up(t.win_mask + b * P, mp_win_mask ? mp_win_mask : no_mask.data(), n_mp * sizeof(uint16_t))) ||
        (rc = up(t.win_kf + b * MA_MAX_BE_KF, win_kf, n_win * sizeof(int32_t))) || (rc = up(t.n_win + b, &counts[4], 4)))
        return rc;
    return MYSLAM_OK;
}

int myslam_map_get(myslam_map* h, int item, int64_t* kf_id, double* kf_pose, int* n_kf, int32_t* edge_v0, int32_t* edge_v1, double* meas, int* n_edges,
                   int64_t* mp_id, double* mp_pos, int32_t* mp_first_kf, uint8_t* mp_state, int* n_mp, int32_t* snapshot, int* n_snapshot,
                   int32_t* mp_gone_kf, uint16_t* mp_win_mask, int32_t* win_kf, int* n_win) {
    if (!h || item < 0 || item >= h->max_batch) return MYSLAM_ERR_INVALID;
    if (stream_is_capturing(h->stream)) return MYSLAM_ERR_UNSUPPORTED;
    MYSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    const MaTables& t = h->t;
    const size_t b = (size_t)item, K = (size_t)t.kf_cap, E = (size_t)t.edge_cap, P = (size_t)t.point_cap, M = (size_t)t.be_mp_cap;
    int32_t c[5];
    const auto down = [](void* dst, const void* src, size_t bytes) { return ma_copy(dst, src, bytes, hipMemcpyDeviceToHost); };
    int rc;
    if ((rc = down(&c[0], t.n_kf + b, 4)) || (rc = down(&c[1], t.n_edges + b, 4)) || (rc = down(&c[2], t.n_mp + b, 4)) || (rc = down(&c[3], t.n_snap + b, 4)) ||
        (rc = down(&c[4], t.n_win + b, 4)))
        return rc;
    const size_t nK = (size_t)clamped_count(c[0], t.kf_cap), nE = (size_t)clamped_count(c[1], t.edge_cap);
    const size_t nP = (size_t)clamped_count(c[2], t.point_cap), nS = (size_t)clamped_count(c[3], t.be_mp_cap);
    const size_t nW = (size_t)clamped_count(c[4], MA_MAX_BE_KF);
    if ((rc = down(kf_id, t.kf_id + b * K, nK * sizeof(int64_t))) || (rc = down(kf_pose, t.kf_pose + b * K * 7, nK * 7 * sizeof(double))) ||
        (rc = down(edge_v0, t.edge_v0 + b * E, nE * sizeof(int32_t))) || (rc = down(edge_v1, t.edge_v1 + b * E, nE * sizeof(int32_t))) ||
        (rc = down(meas, t.meas + b * E * 7, nE * 7 * sizeof(double))) || (rc = down(mp_id, t.mp_id + b * P, nP * sizeof(int64_t))) ||
        (rc = down(mp_pos, t.mp_pos + b * P * 3, nP * 3 * sizeof(double))) || (rc = down(mp_first_kf, t.mp_first_kf + b * P, nP * sizeof(int32_t))) ||
        (rc = down(mp_state, t.mp_state + b * P, nP)) || (rc = down(snapshot, t.snap + b * M, nS * sizeof(int32_t))) ||
        (rc = down(mp_gone_kf, t.gone_kf + b * P, nP * sizeof(int32_t))) || (rc = down(mp_win_mask, t.win_mask + b * P, nP * sizeof(uint16_t))) ||
        (rc = down(win_kf, t.win_kf + b * MA_MAX_BE_KF, nW * sizeof(int32_t))))
        return rc;
    if (n_kf) *n_kf = c[0];
    if (n_edges) *n_edges = c[1];
    if (n_mp) *n_mp = c[2];
    if (n_snapshot) *n_snapshot = c[3];
    if (n_win) *n_win = c[4];
    return MYSLAM_OK;
}

int myslam_map_update_batch(myslam_map* h, int mode, const int64_t* d_kf_id, const double* d_kf_pose, const int32_t* d_n_kf, int be_kf_cap,
                            const int64_t* d_mp_id, const double* d_mp_pos, const int32_t* d_n_mp, int be_mp_cap, const int32_t* d_obs_mp,
                            const int32_t* d_obs_kf, const uint8_t* d_obs_flags, const int32_t* d_n_obs, int be_obs_cap, const int32_t* d_backend_status,
                            const int64_t* d_outlier_mp_id, const int32_t* d_n_outlier_mp, int outlier_cap, const uint8_t* d_mp_report, int batch,
                            int32_t* d_status) {
    if (!h || batch < 0 || (mode != MYSLAM_MAP_AFTER_INSERT && mode != MYSLAM_MAP_AFTER_OPTIMIZE && mode != MYSLAM_MAP_AFTER_RELINK)) return MYSLAM_ERR_INVALID;
    if (mode == MYSLAM_MAP_AFTER_RELINK) {      // the re-link neither makes a key-frame nor a point: an insert's update without an outlier list
        mode = MYSLAM_MAP_AFTER_INSERT; d_n_outlier_mp = nullptr;
    }
    if (!d_kf_id || !d_kf_pose || !d_n_kf || !d_mp_id || !d_mp_pos || !d_n_mp || !d_obs_mp || !d_obs_kf || !d_obs_flags || !d_n_obs || !d_backend_status ||
        !d_status || be_obs_cap < 1 || ma_backend_args_bad(h, be_kf_cap, be_mp_cap))
        return MYSLAM_ERR_INVALID;
    if (mode == MYSLAM_MAP_AFTER_OPTIMIZE && !d_mp_report) return MYSLAM_ERR_INVALID;
    if (mode == MYSLAM_MAP_AFTER_INSERT && d_n_outlier_mp && (!d_outlier_mp_id || outlier_cap < 0)) return MYSLAM_ERR_INVALID;
    if (batch > h->max_batch) return MYSLAM_ERR_CAPACITY;
    if (batch == 0) return MYSLAM_OK;
    const bool ins = mode == MYSLAM_MAP_AFTER_INSERT;
    const BeTablesRead B{d_kf_id, d_kf_pose, d_n_kf, d_mp_id, d_mp_pos, nullptr, d_n_mp, d_obs_mp, d_obs_kf, d_obs_flags, nullptr, nullptr, d_n_obs,
                         be_kf_cap, be_mp_cap, be_obs_cap};
    const MaUpdateIn U{mode, d_backend_status, ins ? d_outlier_mp_id : nullptr, ins ? d_n_outlier_mp : nullptr, (ins && d_n_outlier_mp) ? outlier_cap : 0,
                       d_mp_report, ins ? nullptr : h->solve_pts, ins ? nullptr : h->solve_slot};
    hipLaunchKernelGGL(k_map_update, dim3(batch), dim3(MA_NT), 0, h->stream, h->t, B, U, d_status);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_map_loop_inputs_batch(myslam_map* h, const int64_t* d_kf_id, const int32_t* d_n_kf, int be_kf_cap, const int64_t* d_mp_id, const int32_t* d_n_mp,
                                 int be_mp_cap, const int32_t* d_obs_mp, const int32_t* d_obs_kf, const uint8_t* d_obs_flags, const int32_t* d_n_obs,
                                 int be_obs_cap, const int64_t* d_cur_kf_id, const uint64_t* d_loop_kf_id, const int32_t* d_detect_status, int active_cap,
                                 int batch, int32_t* d_active, int32_t* d_n_active, int32_t* d_cur, int32_t* d_loop, int32_t* d_first_active,
                                 int32_t* d_first_kf, int32_t* d_n_points) {
    if (!h || batch < 0) return MYSLAM_ERR_INVALID;
    if (!d_kf_id || !d_n_kf || !d_mp_id || !d_n_mp || !d_obs_mp || !d_obs_kf || !d_obs_flags || !d_n_obs || !d_cur_kf_id || !d_loop_kf_id || !d_detect_status ||
        !d_active || !d_n_active || !d_cur || !d_loop || !d_first_active || !d_first_kf || !d_n_points || be_obs_cap < 1 ||
        ma_backend_args_bad(h, be_kf_cap, be_mp_cap) || active_cap < be_kf_cap)
        return MYSLAM_ERR_INVALID;
    if (batch > h->max_batch) return MYSLAM_ERR_CAPACITY;
    if (batch == 0) return MYSLAM_OK;
    const BeTablesRead B{d_kf_id, nullptr, d_n_kf, d_mp_id, nullptr, nullptr, d_n_mp, d_obs_mp, d_obs_kf, d_obs_flags, nullptr, nullptr, d_n_obs,
                         be_kf_cap, be_mp_cap, be_obs_cap};
    const MaLoopIn I{d_cur_kf_id, d_loop_kf_id, d_detect_status, active_cap};
    const MaLoopOut O{d_active, d_n_active, d_cur, d_loop, d_first_active, d_first_kf, d_n_points};
    hipLaunchKernelGGL(k_map_loop_inputs, dim3((h->t.point_cap + MA_NT - 1) / MA_NT, batch), dim3(MA_NT), 0, h->stream, h->t, B, I, O);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_map_write_backend_batch(myslam_map* h, const int64_t* d_kf_id, double* d_kf_pose, const int32_t* d_n_kf, int be_kf_cap, const int64_t* d_mp_id,
                                   double* d_mp_pos, const int32_t* d_n_mp, int be_mp_cap, const uint8_t* d_select, int batch) {
    if (!h || batch < 0 || !d_kf_id || !d_kf_pose || !d_n_kf || !d_mp_id || !d_mp_pos || !d_n_mp || ma_backend_args_bad(h, be_kf_cap, be_mp_cap))
        return MYSLAM_ERR_INVALID;
    if (batch > h->max_batch) return MYSLAM_ERR_CAPACITY;
    if (batch == 0) return MYSLAM_OK;
    const BeTablesPose B{d_kf_id, d_kf_pose, d_n_kf, d_mp_id, d_mp_pos, nullptr, d_n_mp, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                         be_kf_cap, be_mp_cap, 0};
    hipLaunchKernelGGL(k_map_write_backend, dim3(batch), dim3(MA_NT), 0, h->stream, h->t, B, d_select);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_map_feature_slots_batch(myslam_map* h, const int64_t* d_feat_mp_id, const int32_t* d_n_feat, int feat_cap, int batch, int32_t* d_feat_landmark) {
    if (!h || batch < 0 || !d_feat_mp_id || !d_n_feat || !d_feat_landmark || feat_cap < 1) return MYSLAM_ERR_INVALID;
    if (batch > h->max_batch) return MYSLAM_ERR_CAPACITY;
    if (batch == 0) return MYSLAM_OK;
    hipLaunchKernelGGL(k_map_feature_slots, dim3((feat_cap + MA_NT - 1) / MA_NT, batch), dim3(MA_NT), 0, h->stream, h->t, d_feat_mp_id, d_n_feat, feat_cap,
                       d_feat_landmark);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_map_filter_landmarks_batch(myslam_map* h, int32_t* d_feat_landmark, int feat_cap, int batch, int32_t* d_n_dropped) {
    if (!h || batch < 0 || !d_feat_landmark || feat_cap < 1) return MYSLAM_ERR_INVALID;
    if (batch > h->max_batch) return MYSLAM_ERR_CAPACITY;
    if (batch == 0) return MYSLAM_OK;
    hipLaunchKernelGGL(k_map_filter_landmarks, dim3(batch), dim3(MA_NT), 0, h->stream, h->t, d_feat_landmark, feat_cap, d_n_dropped);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_map_relink_batch(myslam_map* h, const int32_t* d_merge, const int32_t* d_n_merge, int merge_cap, const int32_t* d_plan_status, int batch,
                            int32_t* d_status) {
    if (!h || batch < 0 || !d_merge || !d_n_merge || !d_plan_status || !d_status || merge_cap < 1) return MYSLAM_ERR_INVALID;
    if (batch > h->max_batch) return MYSLAM_ERR_CAPACITY;
    if (batch == 0) return MYSLAM_OK;
    hipLaunchKernelGGL(k_map_relink, dim3(batch), dim3(MA_NT), 0, h->stream, h->t, d_merge, d_n_merge, merge_cap, d_plan_status, d_status);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

}  // extern "C"
