// backend.hip — Backend::OptimizeActiveMap (reference src/backend.cpp:126-266) for a batch of active maps that live in device tables.
// Three dependent launches on the handle's stream, one workgroup per map in each:
//   k_backend_flatten     the graph-build rules of :139-206 in the orders of myslam_ba_flatten_window (pose slot = key-frame row, landmark slots in
//                         map-point row order, edges grouped by landmark in row order), and the validation of the tables;
//   k_ba_optimize         the solve of :208-243 (ba.hip, through backend_launch.h) on the handle's flat windows;
//   k_backend_write_back  :234-266 with Map::RemoveAllOutlierMapPoints / RemoveOldActiveMapPoints (src/map.cpp:126-175): outlier edges leave the
//                         observation table, emptied map points become outliers, poses and positions are stored, the map-point and observation
//                         tables are compacted in place; the (key-frame id, feature tag) of every removed edge is listed in the handle's buffers
//                         (myslam_backend_culled_view), for the loop store and the tracker, which hold those features too.
// Every order is fixed by the tables, so positions come from block-wide exclusive scans (block_rank / block_exsum of dev_tables.h, whose two
// barriers the in-place compactions of the write-back stand on): no global atomics, and an item's bytes depend neither on its slot nor on its
// neighbours.  See include/myslam_hip.h for the contract.
// k_backend_insert is Map::InsertKeyFrame (src/map.cpp:17-48 with KeyFrame::CreateKF's AddObservation loop, RemoveOldActiveKeyframe and
// RemoveOldActiveMapPoints) on the same tables: one launch, one workgroup per map, the same scans; the tables are rebuilt from a copy the handle holds.
// Every argument struct is a set of batch arrays strided by the caps; its item(b, ...) is the one place that states each stride and returns the
// pointers of map b (arrays with one element per map are indexed by b where they are used).  The caller's tables are dev_tables.h's BeTables /
// InsTables, rows are found with its lower_row / upper_row.  be_tables_bad is the one validation of the tables.
#include "backend_launch.h"
#include "dev_tables.h"
#include "pg_shared.h"

namespace myslam_hip {

constexpr int BE_NT = 512, BE_NW = BE_NT / WAVE;
constexpr int BE_ACTIVE = MYSLAM_BACKEND_OBS_ACTIVE, BE_OUTLIER = MYSLAM_BACKEND_OBS_OUTLIER;

struct BeWork {                         // the handle's buffers of optimise, strided by the same caps
    double* poses; double* pts; int32_t* ep; int32_t* el; double* obs; uint8_t* fixed; int32_t* sizes;       // the flat windows (k_ba_optimize's arguments)
    int32_t* pt_src; int32_t* edge_src;
    int32_t* eidx;                      // obs_cap + 1 per item: edges before row r; row r is an edge iff eidx[r + 1] > eidx[r]
    int32_t* mp_slot;                   // landmark slot of a map-point row, -1 = none
    int32_t* mp_new;                    // row of a map point after the compaction, -1 = it left the table
    int32_t* st;                        // the flatten's verdict: 0 = solve this item, else the item's final status (doubles as the solve's skip flag)
    double* chi2; uint8_t* out; int32_t* rounds; int32_t* nout; int32_t* solve_st;
    struct Item {
        double* poses; double* pts; int32_t* ep; int32_t* el; double* obs; uint8_t* fixed; int32_t* sizes;
        int32_t* pt_src; int32_t* edge_src; int32_t* eidx; int32_t* mp_slot; int32_t* mp_new; double* chi2; uint8_t* out;
    };
    __device__ __forceinline__ Item item(int b, int kf_cap, int mp_cap, int obs_cap) const {
        const size_t k = (size_t)b * kf_cap, m = (size_t)b * mp_cap, o = (size_t)b * obs_cap;
        return {poses + k * 7, pts + m * 3, ep + o, el + o, obs + o * 2, fixed + m, sizes + 3 * (size_t)b,
                pt_src + m, edge_src + o, eidx + (size_t)b * (obs_cap + 1), mp_slot + m, mp_new + m, chi2 + o, out + o};
    }
};

struct BeOut {
    uint8_t* obs_report; uint8_t* mp_report; int32_t* new_outlier_mp; int32_t* n_new_outlier_mp; double* obs_chi2;
    int32_t* rounds; int32_t* n_outlier_edges; int32_t* status;
    int64_t* culled_kf_id; int32_t* culled_tag; int32_t* n_culled;         // the handle's: the features whose edge the solve removed (myslam_backend_culled_view)
    struct Item { uint8_t* obs_report; uint8_t* mp_report; int32_t* new_outlier_mp; double* obs_chi2; int64_t* culled_kf_id; int32_t* culled_tag; };
    __device__ __forceinline__ Item item(int b, int mp_cap, int obs_cap) const {
        const size_t m = (size_t)b * mp_cap, o = (size_t)b * obs_cap;
        return {obs_report + o, mp_report + m, new_outlier_mp + m, obs_chi2 + o, culled_kf_id + o, culled_tag + o};
    }
};

struct InsIn {                          // the new key-frame of every item; n_prior / n_outlier NULL = none
    const int64_t* new_kf_id; const double* new_kf_pose;
    const int64_t* feat_mp_id; const double* feat_mp_pos; const float* feat_uv; const int32_t* feat_tag; const uint8_t* feat_flags;
    const int32_t* n_feat; int feat_cap;
    const int64_t* prior_mp_id; const int64_t* prior_kf_id; const float* prior_uv; const int32_t* prior_tag; const uint8_t* prior_flags;
    const int32_t* n_prior; int prior_cap;
    const int64_t* outlier_mp_id; const int32_t* n_outlier; int outlier_cap;
    int window; double min_dis_th;
    struct Item {
        const double* new_pose;
        const int64_t* fid; const double* fpos; const float* fuv; const int32_t* ftag; const uint8_t* fflags;
        const int64_t* pid; const int64_t* pkf; const float* puv; const int32_t* ptag; const uint8_t* pflags;
        const int64_t* xid;
    };
    // np, nx: the item's prior and outlier counts; a group whose count is 0 (its arrays may be NULL) is nullptr
    __device__ __forceinline__ Item item(int b, int np, int nx) const {
        const size_t f = (size_t)b * feat_cap, p = (size_t)b * prior_cap;
        return {new_kf_pose + (size_t)b * 7, feat_mp_id + f, feat_mp_pos + f * 3, feat_uv + f * 2, feat_tag + f, feat_flags + f,
                np ? prior_mp_id + p : nullptr, np ? prior_kf_id + p : nullptr, np ? prior_uv + p * 2 : nullptr, np ? prior_tag + p : nullptr,
                np ? prior_flags + p : nullptr, nx ? outlier_mp_id + (size_t)b * outlier_cap : nullptr};
    }
};

struct InsWork {                        // the handle's staging of insert, strided by the caps
    int64_t* mp_id; double* mp_pos; uint8_t* mp_outlier;                                         // the tables as they came in (outlier ids applied)
    int32_t* obs_mp; int32_t* obs_kf; uint8_t* obs_flags; float* obs_uv; int32_t* obs_tag;
    int64_t* vid; int32_t* vft;         // obs_cap: ids / indices of the features that name a map point, in feature order
    int64_t* sid; int32_t* sfeat;       // obs_cap: the same sorted by (id, feature index)
    int32_t* dcum;                      // obs_cap + 1: distinct ids that are new to the table among sorted features before s
    int32_t* pcum;                      // obs_cap + 1: prior rows that enter the table before prior row p
    int32_t* dmp; int32_t* drows;       // mp_cap + 1: map points / their rows that leave, before input row m
    int32_t* mp_fin; int32_t* mp_shift; // mp_cap: final row of an input map point (-1 = it leaves); what its observation rows move by
    using Item = InsWork;               // the same fields, of one map
    __device__ __forceinline__ Item item(int b, int mp_cap, int obs_cap) const {
        const size_t m = (size_t)b * mp_cap, o = (size_t)b * obs_cap, m1 = (size_t)b * (mp_cap + 1), o1 = (size_t)b * (obs_cap + 1);
        return {mp_id + m, mp_pos + m * 3, mp_outlier + m, obs_mp + o, obs_kf + o, obs_flags + o, obs_uv + o * 2, obs_tag + o,
                vid + o, vft + o, sid + o, sfeat + o, dcum + o1, pcum + o1, dmp + m1, drows + m1, mp_fin + m, mp_shift + m};
    }
};

struct InsOut {
    int32_t* feat_row; int32_t* mp_new_row; int64_t* removed_kf_id; int32_t* removed_kf_row; double* dis; int32_t* status;
    struct Item { int32_t* feat_row; int32_t* mp_new_row; double* dis; };
    __device__ __forceinline__ Item item(int b, int feat_cap, int mp_cap, int kf_cap) const {
        return {feat_row + (size_t)b * feat_cap, mp_new_row + (size_t)b * mp_cap, dis + (size_t)b * kf_cap};
    }
};

// The rules every operator's tables obey, over counts that are within the caps: key-frame ids ascending, row fields in range and grouped by map
// point, ACTIVE implies a key-frame (the assert of backend.cpp:187), map-point ids ascending.  -> this thread's `bad`; the block ORs them.
// COPY: the same pass stages the map-point and observation tables in `copy` (a compile-time switch: behind a run-time one the item's pointers
// live in scratch memory); without it `copy` is not looked at.
template <bool COPY, class TablesItem>
__device__ __forceinline__ bool be_tables_bad(const TablesItem& tb, int nk, int nm, int no, const InsWork::Item& copy) {
    const int t = threadIdx.x;
    bool bad = false;
    for (int i = t + 1; i < nk; i += BE_NT) bad |= tb.kf_id[i - 1] >= tb.kf_id[i];
    for (int r = t; r < no; r += BE_NT) {
        const int m = tb.obs_mp[r], k = tb.obs_kf[r];
        const uint8_t fl = tb.obs_flags[r];
        bad |= m < 0 || m >= nm || (r > 0 && tb.obs_mp[r - 1] > m) || k < -1 || k >= nk;
        bad |= (fl & BE_ACTIVE) && k < 0;
        if (COPY) {
            copy.obs_mp[r] = m; copy.obs_kf[r] = k; copy.obs_flags[r] = fl;
            copy.obs_uv[2 * r] = tb.obs_uv[2 * r]; copy.obs_uv[2 * r + 1] = tb.obs_uv[2 * r + 1]; copy.obs_tag[r] = tb.obs_tag[r];
        }
    }
    for (int m = t; m < nm; m += BE_NT) {
        bad |= m > 0 && tb.mp_id[m - 1] >= tb.mp_id[m];
        if (COPY) {
            copy.mp_id[m] = tb.mp_id[m]; copy.mp_outlier[m] = tb.mp_outlier[m];
            copy.mp_pos[3 * m] = tb.mp_pos[3 * m]; copy.mp_pos[3 * m + 1] = tb.mp_pos[3 * m + 1]; copy.mp_pos[3 * m + 2] = tb.mp_pos[3 * m + 2];
        }
    }
    return bad;
}

// gate (NULL = every item runs): an item whose entry is not 0 leaves with MYSLAM_MAPPER_IDLE before any of its tables is read (mapper.hip)
__global__ __launch_bounds__(BE_NT) void k_backend_flatten(BeTables T, BeWork W, const int32_t* gate) {
    __shared__ int s_w[BE_NW];
    __shared__ int s_bad;
    const int b = blockIdx.x, t = threadIdx.x;
    if (gate && gate[b] != 0) {                                             // uniform: the solve skips on W.st, the write-back zeroes the reports
        if (t == 0) { W.st[b] = MYSLAM_MAPPER_IDLE; int32_t* const sz = W.sizes + 3 * (size_t)b; sz[0] = 0; sz[1] = 0; sz[2] = 0; }
        return;
    }
    const int nk = T.n_kf[b], nm = T.n_mp[b], no = T.n_obs[b];
    const auto w = W.item(b, T.kf_cap, T.mp_cap, T.obs_cap);
    auto refuse = [&](int st) {                                             // nothing to solve: the item's final status, an empty window
        if (t == 0) { W.st[b] = st; w.sizes[0] = 0; w.sizes[1] = 0; w.sizes[2] = 0; }
    };
    if (nk < 0 || nk > T.kf_cap || nm < 0 || nm > T.mp_cap || no < 0 || no > T.obs_cap) { refuse(MYSLAM_ERR_INVALID); return; }      // uniform
    const auto tb = T.item(b);

    // ---- validation ----
    if (t == 0) s_bad = 0;
    __syncthreads();
    bool bad = be_tables_bad<false>(tb, nk, nm, no, InsWork::Item{});
    for (int m = t; m < nm; m += BE_NT)
        if (!tb.mp_outlier[m]) {                                            // an active map point without observations (:175 would dereference front())
            const int s = lower_row(tb.obs_mp, no, m);
            bad |= s >= no || tb.obs_mp[s] != m;
        }
    if (bad) s_bad = 1;
    __syncthreads();
    if (s_bad) { refuse(MYSLAM_ERR_INVALID); return; }

    // ---- edges: ACTIVE && !OUTLIER rows of map points that are no outliers (:163, :183-189), in row order ----
    int E = 0;
    for (int base = 0; base < no; base += BE_NT) {
        const int r = base + t;
        bool e = false;
        if (r < no) e = (tb.obs_flags[r] & (BE_ACTIVE | BE_OUTLIER)) == BE_ACTIVE && !tb.mp_outlier[tb.obs_mp[r]];
        int tot;
        const int k = E + block_rank<BE_NW>(e, s_w, tot);
        if (r < no) w.eidx[r] = k;
        if (e) {
            w.ep[k] = tb.obs_kf[r]; w.edge_src[k] = r;
            w.obs[2 * k] = (double)tb.obs_uv[2 * r]; w.obs[2 * k + 1] = (double)tb.obs_uv[2 * r + 1];      // toVec2, :196
        }
        E += tot;
    }
    if (E == 0) { refuse(MYSLAM_BACKEND_EMPTY); return; }                   // nothing to optimise: the caller's early return
    if (t == 0) w.eidx[no] = E;
    __syncthreads();

    // ---- landmark slots: map points with at least one edge, in row order; fixed = the first observer has left the window (:175-177) ----
    int L = 0;
    for (int base = 0; base < nm; base += BE_NT) {
        const int m = base + t;
        bool has = false;
        int s = 0;
        if (m < nm && !tb.mp_outlier[m]) {
            s = lower_row(tb.obs_mp, no, m);
            has = w.eidx[lower_row(tb.obs_mp, no, m + 1)] > w.eidx[s];
        }
        int tot;
        const int slot = L + block_rank<BE_NW>(has, s_w, tot);
        if (m < nm) w.mp_slot[m] = has ? slot : -1;
        if (has) {
            w.pt_src[slot] = m;
            w.fixed[slot] = tb.obs_kf[s] < 0 ? 1 : 0;
            w.pts[3 * slot] = tb.mp_pos[3 * m]; w.pts[3 * slot + 1] = tb.mp_pos[3 * m + 1]; w.pts[3 * slot + 2] = tb.mp_pos[3 * m + 2];
        }
        L += tot;
    }
    __syncthreads();
    for (int k = t; k < E; k += BE_NT) w.el[k] = w.mp_slot[tb.obs_mp[w.edge_src[k]]];
    for (int i = t; i < 7 * nk; i += BE_NT) w.poses[i] = tb.kf_pose[i];
    if (t == 0) { w.sizes[0] = nk; w.sizes[1] = L; w.sizes[2] = E; W.st[b] = 0; }
}

__global__ __launch_bounds__(BE_NT) void k_backend_write_back(BeTables T, BeWork W, BeOut O) {
    __shared__ int s_w[BE_NW];
    const int b = blockIdx.x, t = threadIdx.x;
    const int nk = T.n_kf[b], nm = T.n_mp[b], no = T.n_obs[b];
    const auto o = O.item(b, T.mp_cap, T.obs_cap);
    int st = W.st[b];
    if (st == 0) st = W.solve_st[b];
    if (st != 0) {                                                          // refused or empty: the tables keep every byte, the reports are zero
        const int cm = clamped_count(nm, T.mp_cap), co = clamped_count(no, T.obs_cap);
        for (int r = t; r < co; r += BE_NT) { o.obs_report[r] = 0; o.obs_chi2[r] = 0.0; }
        for (int m = t; m < cm; m += BE_NT) o.mp_report[m] = 0;
        if (t == 0) { O.rounds[b] = 0; O.n_outlier_edges[b] = 0; O.n_new_outlier_mp[b] = 0; O.n_culled[b] = 0; O.status[b] = st; }
        return;
    }
    const auto tb = T.item(b);
    const auto w = W.item(b, T.kf_cap, T.mp_cap, T.obs_cap);

    for (int i = t; i < 7 * nk; i += BE_NT) tb.kf_pose[i] = w.poses[i];     // :256-258

    // ---- map points, in ascending chunks: a chunk is read, the block meets in block_rank, then the chunk is written at or below where it stood ----
    int n_keep = 0, n_new = 0;
    for (int base = 0; base < nm; base += BE_NT) {
        const int m = base + t;
        bool keep = false, newout = false;
        int64_t id = 0;
        double p0 = 0, p1 = 0, p2 = 0;
        if (m < nm) {
            const int s = lower_row(tb.obs_mp, no, m), e = lower_row(tb.obs_mp, no, m + 1);
            int nrem = 0, nact = 0;
            for (int k = w.eidx[s]; k < w.eidx[e]; k++) nrem += w.out[k] ? 1 : 0;                 // :237-241: the edge's row leaves both lists
            for (int r = s; r < e; r++) nact += tb.obs_flags[r] & BE_ACTIVE;
            const bool old = tb.mp_outlier[m] != 0;
            newout = !old && nrem == e - s;                                                       // :243-246: no observation left
            const bool leaves = nact - nrem == 0;                                                 // map.cpp:132
            const int rep = (old || newout) ? 2 : (leaves ? 1 : 0);
            o.mp_report[m] = (uint8_t)rep;
            keep = rep == 0;
            id = tb.mp_id[m];
            const int slot = w.mp_slot[m];
            const double* src = slot >= 0 ? w.pts + 3 * slot : tb.mp_pos + 3 * m;                 // :259-261
            p0 = src[0]; p1 = src[1]; p2 = src[2];
        }
        int tot, ntot;
        const int dst = n_keep + block_rank<BE_NW>(keep, s_w, tot);
        const int nd = n_new + block_rank<BE_NW>(newout, s_w, ntot);
        if (m < nm) w.mp_new[m] = keep ? dst : -1;
        if (keep) { tb.mp_id[dst] = id; tb.mp_pos[3 * dst] = p0; tb.mp_pos[3 * dst + 1] = p1; tb.mp_pos[3 * dst + 2] = p2; tb.mp_outlier[dst] = 0; }
        if (newout) o.new_outlier_mp[nd] = m;
        n_keep += tot; n_new += ntot;
    }
    __syncthreads();

    // ---- observation rows, the same way; the removed edges' (key-frame id, feature tag) are listed in row order (:236-247 reset that feature) ----
    int n_rows = 0, n_cull = 0;
    for (int base = 0; base < no; base += BE_NT) {
        const int r = base + t;
        bool keep = false, rem = false;
        int m2 = 0, kf = 0, tag = 0;
        uint8_t fl = 0;
        float u = 0, v = 0;
        if (r < no) {
            const int k = w.eidx[r];
            const bool edge = w.eidx[r + 1] > k;
            rem = edge && w.out[k];
            m2 = w.mp_new[tb.obs_mp[r]];
            keep = m2 >= 0 && !rem;
            o.obs_report[r] = rem ? 1 : (m2 < 0 ? 2 : 0);
            o.obs_chi2[r] = edge ? w.chi2[k] : -1.0;
            kf = tb.obs_kf[r]; tag = tb.obs_tag[r]; u = tb.obs_uv[2 * r]; v = tb.obs_uv[2 * r + 1];
            fl = tb.obs_flags[r];
            if (edge) fl &= (uint8_t)~BE_OUTLIER;                                                 // :249
        }
        int tot, ctot;
        const int dst = n_rows + block_rank<BE_NW>(keep, s_w, tot);
        const int cd = n_cull + block_rank<BE_NW>(rem, s_w, ctot);
        if (keep) {
            tb.obs_mp[dst] = m2; tb.obs_kf[dst] = kf; tb.obs_flags[dst] = fl; tb.obs_uv[2 * dst] = u; tb.obs_uv[2 * dst + 1] = v; tb.obs_tag[dst] = tag;
        }
        if (rem) { o.culled_kf_id[cd] = kf >= 0 ? tb.kf_id[kf] : -1; o.culled_tag[cd] = tag; }     // an edge row is ACTIVE: kf >= 0 (be_tables_bad)
        n_rows += tot; n_cull += ctot;
    }
    if (t == 0) {
        T.n_mp[b] = n_keep; T.n_obs[b] = n_rows;
        O.n_new_outlier_mp[b] = n_new; O.n_culled[b] = n_cull; O.rounds[b] = W.rounds[b]; O.n_outlier_edges[b] = W.nout[b]; O.status[b] = MYSLAM_BACKEND_DONE;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// Map::InsertKeyFrame for a batch of maps (myslam_backend_insert_keyframe_batch)
// One workgroup per map.  Everything is decided from the inputs and the staged copy before the first byte of a table is written; every position is a
// closed form of binary searches and block scans:
//   merged map-point row  = rows of the table below the id + distinct new ids below it
//   merged observation row = the segment's old position + feature rows of smaller ids + prior rows that entered before it
// minus what RemoveOldActiveMapPoints takes out below it.  The rank sort of the features is quadratic in their number (a key-frame has hundreds).
// gate: as k_backend_flatten's
__global__ __launch_bounds__(BE_NT) void k_backend_insert(InsTables T, InsIn I, InsWork W, InsOut O, const int32_t* gate) {
    __shared__ int s_w[BE_NW];
    __shared__ int s_bad, s_victim;
    __shared__ long long s_kfid[MYSLAM_BA_MAX_WINDOW_POSES + 1];
    __shared__ double s_dis[MYSLAM_BA_MAX_WINDOW_POSES];
    const int b = blockIdx.x, t = threadIdx.x;
    const int nk = T.n_kf[b], nm = T.n_mp[b], no = T.n_obs[b], nf = I.n_feat[b];
    const int np = I.n_prior ? I.n_prior[b] : 0, nx = I.n_outlier ? I.n_outlier[b] : 0;
    const auto o = O.item(b, I.feat_cap, T.mp_cap, T.kf_cap);
    auto refuse = [&](int st) {                                             // the tables keep every byte; the reports say "nothing"
        const int cf = clamped_count(nf, I.feat_cap), cm = clamped_count(nm, T.mp_cap);
        for (int f = t; f < cf; f += BE_NT) o.feat_row[f] = -1;
        for (int m = t; m < cm; m += BE_NT) o.mp_new_row[m] = -1;
        if (t < T.kf_cap) o.dis[t] = -1.0;
        if (t == 0) { O.removed_kf_id[b] = -1; O.removed_kf_row[b] = -1; O.status[b] = st; }
    };
    if (gate && gate[b] != 0) { refuse(MYSLAM_MAPPER_IDLE); return; }      // uniform: only the counts were read
    if (nk < 0 || nk > T.kf_cap || nm < 0 || nm > T.mp_cap || no < 0 || no > T.obs_cap || nf < 0 || nf > I.feat_cap || np < 0 || np > I.prior_cap ||
        nx < 0 || nx > I.outlier_cap || I.window < 1) {                     // uniform
        refuse(MYSLAM_ERR_INVALID);
        return;
    }
    const auto tb = T.item(b);
    const auto in = I.item(b, np, nx);
    const auto w = W.item(b, T.mp_cap, T.obs_cap);      // w.mp_id ... w.obs_tag: the copy the tables are rebuilt from
    const int64_t new_id = I.new_kf_id[b];

    // ---- validation, and the copy the tables are rebuilt from ----
    if (t == 0) { s_bad = 0; s_victim = -1; }
    if (t <= nk) s_kfid[t] = t < nk ? tb.kf_id[t] : new_id;
    __syncthreads();
    bool bad = be_tables_bad<true>(tb, nk, nm, no, w);
    if (t == 0 && nk > 0) bad |= new_id <= tb.kf_id[nk - 1];                // mnKFId comes from a counter (keyframe.cpp:24)
    for (int f = t; f < nf; f += BE_NT) bad |= in.fid[f] < -1 || (in.fflags[f] & ~BE_OUTLIER);
    for (int p = t; p < np; p += BE_NT) bad |= (p > 0 && in.pid[p - 1] > in.pid[p]) || (in.pflags[p] & ~BE_OUTLIER);  // ACTIVE is one of the other bits
    if (bad) s_bad = 1;
    __syncthreads();
    if (s_bad) { refuse(MYSLAM_ERR_INVALID); return; }

    // ---- Map::AddOutlierMapPoint (map.cpp:159-164) on the copy: ids that are not in the table are ignored ----
    for (int j = t; j < nx; j += BE_NT) {
        const int m = lower_row(w.mp_id, nm, in.xid[j]);
        if (m < nm && w.mp_id[m] == in.xid[j]) w.mp_outlier[m] = 1;
    }

    // ---- the features that name a map point, sorted by (id, feature index): the rows AddObservation / AddActiveObservation push back ----
    int nv = 0;
    for (int base = 0; base < nf; base += BE_NT) {
        const int f = base + t;
        const bool v = f < nf && in.fid[f] >= 0;
        int tot;
        const int k = nv + block_rank<BE_NW>(v, s_w, tot);
        if (v) { w.vid[k] = in.fid[f]; w.vft[k] = f; }
        nv += tot;
    }
    __syncthreads();
    for (int k = t; k < nv; k += BE_NT) {
        const int64_t id = w.vid[k];
        int r = 0;
        for (int j = 0; j < nv; j++) { const int64_t oid = w.vid[j]; r += (oid < id || (oid == id && j < k)) ? 1 : 0; }
        w.sid[r] = id; w.sfeat[r] = w.vft[k];
    }
    __syncthreads();
    int nu = 0;                                                             // distinct ids that are not in the table: InsertActiveMapPoint adds a row
    for (int base = 0; base < nv; base += BE_NT) {
        const int s = base + t;
        bool fn = false;
        if (s < nv && (s == 0 || w.sid[s - 1] != w.sid[s])) {
            const int m = lower_row(w.mp_id, nm, w.sid[s]);
            fn = !(m < nm && w.mp_id[m] == w.sid[s]);
        }
        int tot;
        const int k = nu + block_rank<BE_NW>(fn, s_w, tot);
        if (s < nv) w.dcum[s] = k;
        nu += tot;
    }
    if (t == 0) w.dcum[nv] = nu;
    int npu = 0;                                                            // prior rows of those ids
    for (int base = 0; base < np; base += BE_NT) {
        const int p = base + t;
        bool u = false;
        if (p < np) {
            const int64_t id = in.pid[p];
            const int m = lower_row(w.mp_id, nm, id), g = lower_row(w.sid, nv, id);
            u = g < nv && w.sid[g] == id && !(m < nm && w.mp_id[m] == id);
        }
        int tot;
        const int k = npu + block_rank<BE_NW>(u, s_w, tot);
        if (p < np) w.pcum[p] = k;
        npu += tot;
    }
    if (t == 0) w.pcum[np] = npu;
    if (nk + 1 > T.kf_cap || nm + nu > T.mp_cap || no + nv + npu > T.obs_cap) { refuse(MYSLAM_ERR_CAPACITY); return; }          // uniform

    // ---- RemoveOldActiveKeyframe's choice (map.cpp:83-107) ----
    const bool removal = nk + 1 > I.window;                                 // map.cpp:44
    if (removal && t < nk) {
        double d[6];
        pg_log(pg_mul(pg_load(tb.kf_pose + 7 * t), pg_inv(pg_load(in.new_pose))), d);
        double s = 0;
        for (int k = 0; k < 6; k++) s += d[k] * d[k];
        s_dis[t] = sqrt(s);
    }
    __syncthreads();
    if (removal && t == 0) {
        double maxDis = 0, minDis = 9999;
        long long maxId = 0, minId = 0;
        for (int i = 0; i < nk; i++) {
            const double d = s_dis[i];
            if (d > maxDis) { maxDis = d; maxId = s_kfid[i]; }
            else if (d < minDis) { minDis = d; minId = s_kfid[i]; }
        }
        const long long gone = minDis < I.min_dis_th ? minId : maxId;
        int v = -1;
        for (int i = 0; i < nk; i++) v = s_kfid[i] == gone ? i : v;         // .at(): an id that is no key-frame of the table throws
        s_victim = v;
    }
    __syncthreads();
    const int victim = s_victim;
    if (removal && victim < 0) { refuse(MYSLAM_ERR_INVALID); return; }

    // ---- RemoveOldActiveMapPoints (map.cpp:126-140): an input map point no feature names and whose ACTIVE rows were all the victim's ----
    int ndm = 0, ndr = 0;
    for (int base = 0; base < nm; base += BE_NT) {
        const int m = base + t;
        bool dead = false;
        int len = 0, g = 0;
        if (m < nm) {
            const int64_t id = w.mp_id[m];
            g = lower_row(w.sid, nv, id);
            if (removal && !(g < nv && w.sid[g] == id)) {
                const int s0 = lower_row(w.obs_mp, no, m), e0 = lower_row(w.obs_mp, no, m + 1);
                bool act = false;
                for (int r = s0; r < e0; r++) act |= (w.obs_flags[r] & BE_ACTIVE) && w.obs_kf[r] != victim;
                dead = !act; len = e0 - s0;
            }
        }
        int tot, rtot;
        const int dm = ndm + block_rank<BE_NW>(dead, s_w, tot);
        const int dr = ndr + block_exsum<BE_NW>(dead ? len : 0, s_w, rtot);
        if (m < nm) {
            w.dmp[m] = dm; w.drows[m] = dr;
            w.mp_fin[m] = dead ? -1 : m + w.dcum[g] - dm;
            w.mp_shift[m] = g + w.pcum[lower_row(in.pid, np, w.mp_id[m])] - dr;
        }
        ndm += tot; ndr += rtot;
    }
    if (t == 0) { w.dmp[nm] = ndm; w.drows[nm] = ndr; }

    // ---- the key-frame table: the victim's row leaves, the new row is the last ----
    long long kid = 0;
    double kp[7];
    if (t <= nk) {
        kid = s_kfid[t];
        const double* src = t < nk ? tb.kf_pose + 7 * t : in.new_pose;
        for (int k = 0; k < 7; k++) kp[k] = src[k];
    }
    __syncthreads();                                                        // everything above is decided and stored; from here on the tables are written
    if (t <= nk && t != victim) {
        const int dst = t - ((removal && t > victim) ? 1 : 0);
        tb.kf_id[dst] = kid;
        for (int k = 0; k < 7; k++) tb.kf_pose[7 * dst + k] = kp[k];
    }
    const int new_kf_row = removal ? nk - 1 : nk;
    auto kf_row_after = [&](int k) { return !removal || k < victim ? k : (k == victim ? -1 : k - 1); };

    // ---- map points: the input rows that stay, then the new ids (position from the first feature naming them) ----
    for (int m = t; m < nm; m += BE_NT) {
        const int dst = w.mp_fin[m];
        o.mp_new_row[m] = dst;
        if (dst >= 0 && dst < T.mp_cap) {
            tb.mp_id[dst] = w.mp_id[m]; tb.mp_outlier[dst] = w.mp_outlier[m];
            tb.mp_pos[3 * dst] = w.mp_pos[3 * m]; tb.mp_pos[3 * dst + 1] = w.mp_pos[3 * m + 1]; tb.mp_pos[3 * dst + 2] = w.mp_pos[3 * m + 2];
        }
    }
    for (int f = t; f < nf; f += BE_NT) if (in.fid[f] < 0) o.feat_row[f] = -1;
    for (int s = t; s < nv; s += BE_NT) {
        const int64_t id = w.sid[s];
        const int f = w.sfeat[s];
        const int lm = lower_row(w.mp_id, nm, id), g = lower_row(w.sid, nv, id);
        const bool in_table = lm < nm && w.mp_id[lm] == id;
        const int um = lm + (in_table ? 1 : 0);
        const int mrow = lm + w.dcum[g] - w.dmp[lm];
        if (!in_table && g == s && (unsigned)mrow < (unsigned)T.mp_cap) {
            tb.mp_id[mrow] = id; tb.mp_outlier[mrow] = 0;
            tb.mp_pos[3 * mrow] = in.fpos[3 * f]; tb.mp_pos[3 * mrow + 1] = in.fpos[3 * f + 1]; tb.mp_pos[3 * mrow + 2] = in.fpos[3 * f + 2];
        }
        // the feature's row: behind the segment's old rows (or its prior rows), in feature order
        const int dst = lower_row(w.obs_mp, no, um) + w.pcum[upper_row(in.pid, np, id)] + s - w.drows[um];
        if ((unsigned)dst >= (unsigned)T.obs_cap) continue;            // cannot happen: the merged count passed the capacity check
        tb.obs_mp[dst] = mrow; tb.obs_kf[dst] = new_kf_row; tb.obs_flags[dst] = (uint8_t)(BE_ACTIVE | (in.fflags[f] & BE_OUTLIER));
        tb.obs_uv[2 * dst] = in.fuv[2 * f]; tb.obs_uv[2 * dst + 1] = in.fuv[2 * f + 1]; tb.obs_tag[dst] = in.ftag[f];
        o.feat_row[f] = dst;
    }
    // ---- the input observation rows: RemoveActiveObservation on the victim's, key-frame rows renumbered ----
    for (int r = t; r < no; r += BE_NT) {
        const int m = w.obs_mp[r], mrow = w.mp_fin[m];
        if (mrow < 0) continue;
        const int dst = r + w.mp_shift[m], k = w.obs_kf[r];
        if ((unsigned)dst >= (unsigned)T.obs_cap) continue;
        uint8_t fl = w.obs_flags[r];
        if (removal && k == victim) fl &= (uint8_t)~BE_ACTIVE;
        tb.obs_mp[dst] = mrow; tb.obs_kf[dst] = k < 0 ? -1 : kf_row_after(k); tb.obs_flags[dst] = fl;
        tb.obs_uv[2 * dst] = w.obs_uv[2 * r]; tb.obs_uv[2 * dst + 1] = w.obs_uv[2 * r + 1]; tb.obs_tag[dst] = w.obs_tag[r];
    }
    // ---- GetObservations() of a map point that comes back: never ACTIVE, key-frame resolved against the final table ----
    for (int p = t; p < np; p += BE_NT) {
        if (w.pcum[p + 1] == w.pcum[p]) continue;
        const int64_t id = in.pid[p];
        const int lm = lower_row(w.mp_id, nm, id), g = lower_row(w.sid, nv, id);
        const int dst = lower_row(w.obs_mp, no, lm) + g + w.pcum[p] - w.drows[lm];
        if ((unsigned)dst >= (unsigned)T.obs_cap) continue;
        int k = -1;
        for (int i = 0; i <= nk; i++) k = s_kfid[i] == in.pkf[p] ? i : k;
        tb.obs_mp[dst] = lm + w.dcum[g] - w.dmp[lm]; tb.obs_kf[dst] = k < 0 ? -1 : (k == nk ? new_kf_row : kf_row_after(k)); tb.obs_flags[dst] = in.pflags[p];
        tb.obs_uv[2 * dst] = in.puv[2 * p]; tb.obs_uv[2 * dst + 1] = in.puv[2 * p + 1]; tb.obs_tag[dst] = in.ptag[p];
    }
    if (t < T.kf_cap) o.dis[t] = (removal && t < nk) ? s_dis[t] : -1.0;
    if (t == 0) {
        T.n_kf[b] = new_kf_row + 1; T.n_mp[b] = nm + nu - ndm; T.n_obs[b] = no + nv + npu - ndr;
        O.removed_kf_id[b] = removal ? (int64_t)s_kfid[victim] : -1; O.removed_kf_row[b] = victim; O.status[b] = MYSLAM_OK;
    }
}

// k_backend_relink: LoopLocalFusion's re-linking (src/loopclosing.cpp:521-527) on the tables, from the rows myslam_relink_stage_batch staged.  A merged
// point leaves with all its rows (Map::RemoveMapPoint, src/map.cpp:144-155); a point the rows end on that is in the table gets them at the END of its
// segment, each at the place the stage gave it, ACTIVE cleared (AddObservation alone runs), OUTLIER kept, its key-frame found by id.  The tables are
// rebuilt from the handle's copy, as the insert does; everything is decided before anything is written.
__global__ __launch_bounds__(BE_NT) void k_backend_relink(InsTables T, InsWork W, myslam_relink_lists R, const int32_t* stage_status, int32_t* mp_new_row,
                                                          int32_t* status) {
    __shared__ int s_w[BE_NW];
    __shared__ int s_bad;
    const int b = blockIdx.x, t = threadIdx.x;
    const int nk = T.n_kf[b], nm = T.n_mp[b], no = T.n_obs[b];
    int32_t* const new_row = mp_new_row + (size_t)b * T.mp_cap;
    auto refuse = [&](int st) {                                             // the tables keep every byte
        for (int m = t; m < clamped_count(nm, T.mp_cap); m += BE_NT) new_row[m] = -1;
        if (t == 0) status[b] = st;
    };
    const int ss = stage_status[b];
    if (ss != 0) { refuse(ss); return; }                                    // uniform: skipped, or the stage's refusal
    const int nmg = R.n_staged_merges[b], nst = R.n_rows[b];
    if (nk < 0 || nk > T.kf_cap || nm < 0 || nm > T.mp_cap || no < 0 || no > T.obs_cap || nmg < 0 || nmg > R.out_cap || nst < 0 || nst > R.stage_cap ||
        R.table_mp[b] != nm || R.table_rows[b] != no) {                     // uniform: the rows were not staged for this table
        refuse(MYSLAM_ERR_INVALID);
        return;
    }
    const auto tb = T.item(b);
    const auto w = W.item(b, T.mp_cap, T.obs_cap);
    int32_t* const old_off = w.dmp; int32_t* const new_off = w.drows;      // mp_cap + 1 each
    int32_t* const fin = w.mp_fin; int32_t* const add = w.mp_shift;        // final row of an input point (-1: it leaves); the rows it receives
    const int64_t* const mg_from = R.merge_from_id + (size_t)b * R.out_cap;
    const int64_t* const mg_root = R.merge_root_id + (size_t)b * R.out_cap;
    const int32_t* const mg_rows = R.merge_rows + (size_t)b * R.out_cap;
    const size_t sb = (size_t)b * R.stage_cap;
    if (t == 0) s_bad = 0;
    __syncthreads();
    bool bad = be_tables_bad<true>(tb, nk, nm, no, w);
    for (int m = t; m < nm; m += BE_NT) { fin[m] = 0; add[m] = 0; }
    if (bad) s_bad = 1;
    __syncthreads();
    if (s_bad) { refuse(MYSLAM_ERR_INVALID); return; }
    for (int r = t; r <= no; r += BE_NT) {                                  // where every segment starts (obs_mp is in range and non-decreasing)
        const int prev = r ? w.obs_mp[r - 1] : -1, cur = r < no ? w.obs_mp[r] : nm;
        for (int m = prev + 1; m <= cur; m++) old_off[m] = r;
    }
    __syncthreads();
    if (t == 0)
        for (int i = 0; i < nmg; i++) {
            const int fr = find_row(w.mp_id, nm, mg_from[i]), rr = find_row(w.mp_id, nm, mg_root[i]);
            if (fr >= 0) { fin[fr] = -1; if (old_off[fr + 1] - old_off[fr] != mg_rows[i]) s_bad = 1; }
            if (rr >= 0) add[rr] += mg_rows[i];
        }
    __syncthreads();
    int n_rows = 0, n_pts = 0;
    for (int m0 = 0; m0 < nm; m0 += BE_NT) {                                // uniform: the new places, in the table's order
        const int m = m0 + t;
        const bool keep = m < nm && fin[m] == 0;
        if (m < nm && !keep && add[m]) s_bad = 1;                           // rows never end on a point that was merged away
        const int len = keep ? old_off[m + 1] - old_off[m] + add[m] : 0;
        int tot, totp;
        const int pos = n_rows + block_exsum<BE_NW>(len, s_w, tot);
        const int row = n_pts + block_rank<BE_NW>(keep, s_w, totp);
        if (m < nm) { new_off[m] = pos; fin[m] = keep ? row : -1; }
        n_rows += tot; n_pts += totp;
    }
    for (int d = t; d < nst; d += BE_NT) {                                  // a staged row stands behind the rows its point had, within what it receives
        const int rr = find_row(w.mp_id, nm, R.row_root_id[sb + d]);
        if (rr < 0) continue;
        const int place = R.row_place[sb + d], len = old_off[rr + 1] - old_off[rr];
        if (place < len || place >= len + add[rr] || (R.row_flags[sb + d] & ~BE_OUTLIER)) s_bad = 1;
    }
    __syncthreads();
    if (s_bad || n_rows > T.obs_cap) { refuse(s_bad ? MYSLAM_ERR_INVALID : MYSLAM_ERR_CAPACITY); return; }      // uniform
    // ---- from here on the item is written ----
    for (int r = t; r < no; r += BE_NT) {
        const int m = w.obs_mp[r];
        if (fin[m] < 0) continue;
        const int q = new_off[m] + (r - old_off[m]);
        tb.obs_mp[q] = fin[m]; tb.obs_kf[q] = w.obs_kf[r]; tb.obs_flags[q] = w.obs_flags[r];
        tb.obs_uv[2 * q] = w.obs_uv[2 * r]; tb.obs_uv[2 * q + 1] = w.obs_uv[2 * r + 1]; tb.obs_tag[q] = w.obs_tag[r];
    }
    for (int d = t; d < nst; d += BE_NT) {
        const int rr = find_row(w.mp_id, nm, R.row_root_id[sb + d]);
        if (rr < 0) continue;
        const int q = new_off[rr] + R.row_place[sb + d];
        tb.obs_mp[q] = fin[rr]; tb.obs_kf[q] = find_row(tb.kf_id, nk, R.row_kf_id[sb + d]); tb.obs_flags[q] = R.row_flags[sb + d] & BE_OUTLIER;
        tb.obs_uv[2 * q] = R.row_uv[2 * (sb + d)]; tb.obs_uv[2 * q + 1] = R.row_uv[2 * (sb + d) + 1]; tb.obs_tag[q] = R.row_tag[sb + d];
    }
    for (int m = t; m < nm; m += BE_NT) {
        const int q = fin[m];
        new_row[m] = q;
        if (q < 0) continue;
        tb.mp_id[q] = w.mp_id[m]; tb.mp_outlier[q] = w.mp_outlier[m];
        tb.mp_pos[3 * q] = w.mp_pos[3 * m]; tb.mp_pos[3 * q + 1] = w.mp_pos[3 * m + 1]; tb.mp_pos[3 * q + 2] = w.mp_pos[3 * m + 2];
    }
    if (t == 0) { T.n_mp[b] = n_pts; T.n_obs[b] = n_rows; status[b] = MYSLAM_OK; }
}

}  // namespace myslam_hip

using namespace myslam_hip;

struct myslam_backend {
    int max_batch = 0, kf_cap = 0, mp_cap = 0, obs_cap = 0;
    hipStream_t stream = nullptr;
    size_t wstride = 0;
    Buf<double> scratch;                // the solve's
    BeWork w{};                         // optimise's buffers, which debug_flat / debug_solved read after any later call ...
    InsWork iw{};                       // ... so insert's staging shares none of them
    int64_t* culled_kf_id = nullptr; int32_t* culled_tag = nullptr; int32_t* n_culled = nullptr;    // the write-back's list of culled features
    BufSet mem;                         // owns every block that `w` and `iw` name, and the culled list
};

extern "C" {

int myslam_backend_destroy(myslam_backend* h) {
    if (!h) return MYSLAM_ERR_INVALID;
    (void)hipStreamSynchronize(h->stream);
    delete h;
    return MYSLAM_OK;
}

int myslam_backend_create(myslam_backend** out, int max_batch, int kf_cap, int mp_cap, int obs_cap) {
    if (!out || max_batch < 1 || max_batch > 65535 || kf_cap < 1 || mp_cap < 1 || obs_cap < 1) return MYSLAM_ERR_INVALID;
    if (kf_cap > MYSLAM_BA_MAX_WINDOW_POSES) return MYSLAM_ERR_UNSUPPORTED;
    if (mp_cap > (1 << 24) || obs_cap > (1 << 24)) return MYSLAM_ERR_CAPACITY;
    if (need_device()) return MYSLAM_ERR_HIP;
    myslam_backend* h = new myslam_backend();
    h->max_batch = max_batch; h->kf_cap = kf_cap; h->mp_cap = mp_cap; h->obs_cap = obs_cap;
    h->wstride = ba_active_map_scratch_doubles(mp_cap, obs_cap);
    const size_t B = (size_t)max_batch, K = (size_t)kf_cap, M = (size_t)mp_cap, N = (size_t)obs_cap;
    BeWork& w = h->w;
    InsWork& iw = h->iw;
    auto own = [&](auto*& p, size_t n) { return h->mem.own(p, n, MYSLAM_ERR_CAPACITY); };
    int rc;
    if ((rc = h->scratch.renew(B * h->wstride, MYSLAM_ERR_CAPACITY)) ||
        (rc = own(w.poses, B * K * 7)) || (rc = own(w.pts, B * M * 3)) || (rc = own(w.ep, B * N)) || (rc = own(w.el, B * N)) ||
        (rc = own(w.obs, B * N * 2)) || (rc = own(w.fixed, B * M)) || (rc = own(w.sizes, B * 3)) || (rc = own(w.pt_src, B * M)) ||
        (rc = own(w.edge_src, B * N)) || (rc = own(w.eidx, B * (N + 1))) || (rc = own(w.mp_slot, B * M)) || (rc = own(w.mp_new, B * M)) ||
        (rc = own(w.st, B)) || (rc = own(w.chi2, B * N)) || (rc = own(w.out, B * N)) || (rc = own(w.rounds, B)) || (rc = own(w.nout, B)) ||
        (rc = own(w.solve_st, B)) ||
        (rc = own(iw.mp_id, B * M)) || (rc = own(iw.mp_pos, B * M * 3)) || (rc = own(iw.mp_outlier, B * M)) || (rc = own(iw.obs_mp, B * N)) ||
        (rc = own(iw.obs_kf, B * N)) || (rc = own(iw.obs_flags, B * N)) || (rc = own(iw.obs_uv, B * N * 2)) || (rc = own(iw.obs_tag, B * N)) ||
        (rc = own(iw.vid, B * N)) || (rc = own(iw.vft, B * N)) || (rc = own(iw.sid, B * N)) || (rc = own(iw.sfeat, B * N)) ||
        (rc = own(iw.dcum, B * (N + 1))) || (rc = own(iw.pcum, B * (N + 1))) || (rc = own(iw.dmp, B * (M + 1))) ||
        (rc = own(iw.drows, B * (M + 1))) || (rc = own(iw.mp_fin, B * M)) || (rc = own(iw.mp_shift, B * M)) ||
        (rc = own(h->culled_kf_id, B * N)) || (rc = own(h->culled_tag, B * N)) || (rc = own(h->n_culled, B))) {
        delete h;
        return rc;
    }
    // debug_flat before the first call reports empty windows
    const std::vector<int32_t> zeros(B * 3, 0);
    if ((rc = upload_table(w.sizes, zeros.data(), zeros.size() * sizeof(int32_t))) ||
        (rc = upload_table(h->n_culled, zeros.data(), B * sizeof(int32_t)))) {             // culled_view before the first call: empty lists
        delete h;
        return rc;
    }
    *out = h;
    return MYSLAM_OK;
}

int myslam_backend_set_stream(myslam_backend* h, void* hip_stream) {
    if (!h) return MYSLAM_ERR_INVALID;
    h->stream = (hipStream_t)hip_stream;
    return MYSLAM_OK;
}

int myslam_backend_launches_per_call(const myslam_backend* h) { return h ? 3 : MYSLAM_ERR_INVALID; }

int myslam_backend_solve_view(const myslam_backend* h, const double** d_points, const int32_t** d_mp_slot) {
    if (!h || !d_points || !d_mp_slot) return MYSLAM_ERR_INVALID;
    *d_points = h->w.pts; *d_mp_slot = h->w.mp_slot;
    return MYSLAM_OK;
}

int myslam_backend_culled_view(const myslam_backend* h, const int64_t** d_kf_id, const int32_t** d_tag, const int32_t** d_n_culled) {
    if (!h || !d_kf_id || !d_tag || !d_n_culled) return MYSLAM_ERR_INVALID;
    *d_kf_id = h->culled_kf_id; *d_tag = h->culled_tag; *d_n_culled = h->n_culled;
    return MYSLAM_OK;
}

int myslam_backend_optimize_batch(myslam_backend* h, const int64_t* d_kf_id, double* d_kf_pose, const int32_t* d_n_kf, int64_t* d_mp_id, double* d_mp_pos,
                                  uint8_t* d_mp_outlier, int32_t* d_n_mp, int32_t* d_obs_mp, int32_t* d_obs_kf, uint8_t* d_obs_flags, float* d_obs_uv,
                                  int32_t* d_obs_tag, int32_t* d_n_obs, int batch, double fx, double fy, double cx, double cy, double huber_delta,
                                  double chi2_th, int max_rounds, int iters_per_round, uint8_t* d_obs_report, uint8_t* d_mp_report,
                                  int32_t* d_new_outlier_mp, int32_t* d_n_new_outlier_mp, double* d_obs_chi2, int32_t* d_rounds,
                                  int32_t* d_n_outlier_edges, int32_t* d_status) {
    return backend_optimize_launch(h, d_kf_id, d_kf_pose, d_n_kf, d_mp_id, d_mp_pos, d_mp_outlier, d_n_mp, d_obs_mp, d_obs_kf, d_obs_flags, d_obs_uv, d_obs_tag,
                                   d_n_obs, batch, fx, fy, cx, cy, huber_delta, chi2_th, max_rounds, iters_per_round, d_obs_report, d_mp_report,
                                   d_new_outlier_mp, d_n_new_outlier_mp, d_obs_chi2, d_rounds, d_n_outlier_edges, d_status, nullptr);
}

}  // extern "C"

int myslam_hip::backend_optimize_launch(myslam_backend* h, const int64_t* d_kf_id, double* d_kf_pose, const int32_t* d_n_kf, int64_t* d_mp_id, double* d_mp_pos,
                                        uint8_t* d_mp_outlier, int32_t* d_n_mp, int32_t* d_obs_mp, int32_t* d_obs_kf, uint8_t* d_obs_flags, float* d_obs_uv,
                                        int32_t* d_obs_tag, int32_t* d_n_obs, int batch, double fx, double fy, double cx, double cy, double huber_delta,
                                        double chi2_th, int max_rounds, int iters_per_round, uint8_t* d_obs_report, uint8_t* d_mp_report,
                                        int32_t* d_new_outlier_mp, int32_t* d_n_new_outlier_mp, double* d_obs_chi2, int32_t* d_rounds,
                                        int32_t* d_n_outlier_edges, int32_t* d_status, const int32_t* d_gate) {
    if (!h || batch < 0 || max_rounds < 1 || iters_per_round < 1) return MYSLAM_ERR_INVALID;
    if (batch > h->max_batch) return MYSLAM_ERR_CAPACITY;
    if (batch == 0) return MYSLAM_OK;
    if (!d_kf_id || !d_kf_pose || !d_n_kf || !d_mp_id || !d_mp_pos || !d_mp_outlier || !d_n_mp || !d_obs_mp || !d_obs_kf || !d_obs_flags || !d_obs_uv ||
        !d_obs_tag || !d_n_obs || !d_obs_report || !d_mp_report || !d_new_outlier_mp || !d_n_new_outlier_mp || !d_obs_chi2 || !d_rounds ||
        !d_n_outlier_edges || !d_status)
        return MYSLAM_ERR_INVALID;
    const BeTables T{d_kf_id, d_kf_pose, d_n_kf, d_mp_id, d_mp_pos, d_mp_outlier, d_n_mp, d_obs_mp, d_obs_kf, d_obs_flags, d_obs_uv, d_obs_tag, d_n_obs,
                     h->kf_cap, h->mp_cap, h->obs_cap};
    const BeWork& W = h->w;
    const BeOut O{d_obs_report, d_mp_report, d_new_outlier_mp, d_n_new_outlier_mp, d_obs_chi2, d_rounds, d_n_outlier_edges, d_status,
                  h->culled_kf_id, h->culled_tag, h->n_culled};
    hipLaunchKernelGGL(k_backend_flatten, dim3(batch), dim3(BE_NT), 0, h->stream, T, W, d_gate);
    MYSLAM_HIP_CHECK(hipGetLastError());
    const int rc = ba_active_map_launch(W.poses, W.pts, W.ep, W.el, W.obs, W.fixed, W.sizes, W.st, batch, h->kf_cap, h->mp_cap, h->obs_cap, fx, fy, cx, cy,
                                        huber_delta, chi2_th, max_rounds, iters_per_round, h->scratch, h->wstride, W.chi2, W.out, W.rounds, W.nout,
                                        W.solve_st, h->stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_backend_write_back, dim3(batch), dim3(BE_NT), 0, h->stream, T, W, O);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

extern "C" {

int myslam_backend_insert_launches_per_call(const myslam_backend* h) { return h ? 1 : MYSLAM_ERR_INVALID; }

int myslam_backend_insert_keyframe_batch(myslam_backend* h, int64_t* d_kf_id, double* d_kf_pose, int32_t* d_n_kf, int64_t* d_mp_id, double* d_mp_pos,
                                         uint8_t* d_mp_outlier, int32_t* d_n_mp, int32_t* d_obs_mp, int32_t* d_obs_kf, uint8_t* d_obs_flags,
                                         float* d_obs_uv, int32_t* d_obs_tag, int32_t* d_n_obs, const int64_t* d_new_kf_id, const double* d_new_kf_pose,
                                         const int64_t* d_feat_mp_id, const double* d_feat_mp_pos, const float* d_feat_uv, const int32_t* d_feat_tag,
                                         const uint8_t* d_feat_flags, const int32_t* d_n_feat, int feat_cap, const int64_t* d_prior_mp_id,
                                         const int64_t* d_prior_kf_id, const float* d_prior_uv, const int32_t* d_prior_tag, const uint8_t* d_prior_flags,
                                         const int32_t* d_n_prior, int prior_cap, const int64_t* d_outlier_mp_id, const int32_t* d_n_outlier_mp,
                                         int outlier_cap, int batch, int window, double min_dis_th, int32_t* d_feat_row, int32_t* d_mp_new_row,
                                         int64_t* d_removed_kf_id, int32_t* d_removed_kf_row, double* d_dis, int32_t* d_status) {
    return backend_insert_launch(h, d_kf_id, d_kf_pose, d_n_kf, d_mp_id, d_mp_pos, d_mp_outlier, d_n_mp, d_obs_mp, d_obs_kf, d_obs_flags, d_obs_uv, d_obs_tag, d_n_obs,
                                 d_new_kf_id, d_new_kf_pose, d_feat_mp_id, d_feat_mp_pos, d_feat_uv, d_feat_tag, d_feat_flags, d_n_feat, feat_cap, d_prior_mp_id,
                                 d_prior_kf_id, d_prior_uv, d_prior_tag, d_prior_flags, d_n_prior, prior_cap, d_outlier_mp_id, d_n_outlier_mp, outlier_cap, batch,
                                 window, min_dis_th, d_feat_row, d_mp_new_row, d_removed_kf_id, d_removed_kf_row, d_dis, d_status, nullptr);
}

}  // extern "C"

int myslam_hip::backend_insert_launch(myslam_backend* h, int64_t* d_kf_id, double* d_kf_pose, int32_t* d_n_kf, int64_t* d_mp_id, double* d_mp_pos,
                                         uint8_t* d_mp_outlier, int32_t* d_n_mp, int32_t* d_obs_mp, int32_t* d_obs_kf, uint8_t* d_obs_flags,
                                         float* d_obs_uv, int32_t* d_obs_tag, int32_t* d_n_obs, const int64_t* d_new_kf_id, const double* d_new_kf_pose,
                                         const int64_t* d_feat_mp_id, const double* d_feat_mp_pos, const float* d_feat_uv, const int32_t* d_feat_tag,
                                         const uint8_t* d_feat_flags, const int32_t* d_n_feat, int feat_cap, const int64_t* d_prior_mp_id,
                                         const int64_t* d_prior_kf_id, const float* d_prior_uv, const int32_t* d_prior_tag, const uint8_t* d_prior_flags,
                                         const int32_t* d_n_prior, int prior_cap, const int64_t* d_outlier_mp_id, const int32_t* d_n_outlier_mp,
                                         int outlier_cap, int batch, int window, double min_dis_th, int32_t* d_feat_row, int32_t* d_mp_new_row,
                                         int64_t* d_removed_kf_id, int32_t* d_removed_kf_row, double* d_dis, int32_t* d_status, const int32_t* d_gate) {
    if (!h || batch < 0 || feat_cap < 0) return MYSLAM_ERR_INVALID;
    if (!d_kf_id || !d_kf_pose || !d_n_kf || !d_mp_id || !d_mp_pos || !d_mp_outlier || !d_n_mp || !d_obs_mp || !d_obs_kf || !d_obs_flags || !d_obs_uv ||
        !d_obs_tag || !d_n_obs || !d_new_kf_id || !d_new_kf_pose || !d_feat_mp_id || !d_feat_mp_pos || !d_feat_uv || !d_feat_tag || !d_feat_flags ||
        !d_n_feat || !d_feat_row || !d_mp_new_row || !d_removed_kf_id || !d_removed_kf_row || !d_dis || !d_status)
        return MYSLAM_ERR_INVALID;
    // the optional inputs are given by their counts: with a count array, its tables are required
    if (d_n_prior && (prior_cap < 0 || !d_prior_mp_id || !d_prior_kf_id || !d_prior_uv || !d_prior_tag || !d_prior_flags)) return MYSLAM_ERR_INVALID;
    if (d_n_outlier_mp && (outlier_cap < 0 || !d_outlier_mp_id)) return MYSLAM_ERR_INVALID;
    if (batch > h->max_batch || feat_cap > h->obs_cap || (d_n_prior && prior_cap > h->obs_cap)) return MYSLAM_ERR_CAPACITY;
    if (batch == 0) return MYSLAM_OK;
    const InsTables T{d_kf_id, d_kf_pose, d_n_kf, d_mp_id, d_mp_pos, d_mp_outlier, d_n_mp, d_obs_mp, d_obs_kf, d_obs_flags, d_obs_uv, d_obs_tag, d_n_obs,
                      h->kf_cap, h->mp_cap, h->obs_cap};
    const InsIn I{d_new_kf_id, d_new_kf_pose, d_feat_mp_id, d_feat_mp_pos, d_feat_uv, d_feat_tag, d_feat_flags, d_n_feat, feat_cap,
                  d_prior_mp_id, d_prior_kf_id, d_prior_uv, d_prior_tag, d_prior_flags, d_n_prior, d_n_prior ? prior_cap : 0,
                  d_outlier_mp_id, d_n_outlier_mp, d_n_outlier_mp ? outlier_cap : 0, window, min_dis_th};
    const InsOut O{d_feat_row, d_mp_new_row, d_removed_kf_id, d_removed_kf_row, d_dis, d_status};
    hipLaunchKernelGGL(k_backend_insert, dim3(batch), dim3(BE_NT), 0, h->stream, T, I, h->iw, O, d_gate);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

extern "C" {

// device -> host, complete on return; on this thread's non-blocking stream, never the legacy stream (common.h).  The caller has waited for h->stream.
static int be_fetch(void* dst, const void* src, size_t bytes) {
    if (!dst || bytes == 0) return MYSLAM_OK;
    const hipStream_t st = host_call_stream();
    if (!st) return MYSLAM_ERR_HIP;
    return copy_sync(dst, src, bytes, hipMemcpyDeviceToHost, st);
}

int myslam_backend_debug_flat(myslam_backend* h, int item, int32_t* pose_src, int32_t* pt_src, int32_t* edge_pose, int32_t* edge_pt, double* edge_obs,
                              int32_t* edge_src, uint8_t* fixed, int32_t* sizes3) {
    if (!h || item < 0 || item >= h->max_batch || !sizes3) return MYSLAM_ERR_INVALID;
    MYSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    const size_t b = (size_t)item, M = (size_t)h->mp_cap, N = (size_t)h->obs_cap;
    const BeWork& w = h->w;
    int rc;
    if ((rc = be_fetch(sizes3, w.sizes + 3 * b, 3 * sizeof(int32_t)))) return rc;
    const size_t P = (size_t)sizes3[0], L = (size_t)sizes3[1], E = (size_t)sizes3[2];
    if (pose_src) for (size_t i = 0; i < P; i++) pose_src[i] = (int32_t)i;       // pose slot = key-frame row
    if ((rc = be_fetch(pt_src, w.pt_src + b * M, L * sizeof(int32_t))) || (rc = be_fetch(fixed, w.fixed + b * M, L)) ||
        (rc = be_fetch(edge_pose, w.ep + b * N, E * sizeof(int32_t))) || (rc = be_fetch(edge_pt, w.el + b * N, E * sizeof(int32_t))) ||
        (rc = be_fetch(edge_obs, w.obs + b * N * 2, E * 2 * sizeof(double))) || (rc = be_fetch(edge_src, w.edge_src + b * N, E * sizeof(int32_t))))
        return rc;
    return MYSLAM_OK;
}

int myslam_backend_debug_solved(myslam_backend* h, int item, double* poses, double* points, double* edge_chi2, uint8_t* edge_outlier,
                                int32_t* rounds_outliers2) {
    if (!h || item < 0 || item >= h->max_batch) return MYSLAM_ERR_INVALID;
    MYSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    const size_t b = (size_t)item, K = (size_t)h->kf_cap, M = (size_t)h->mp_cap, N = (size_t)h->obs_cap;
    const BeWork& w = h->w;
    int32_t sz[3];
    int rc;
    if ((rc = be_fetch(sz, w.sizes + 3 * b, sizeof(sz)))) return rc;
    const size_t P = (size_t)sz[0], L = (size_t)sz[1], E = (size_t)sz[2];
    if ((rc = be_fetch(poses, w.poses + b * K * 7, P * 7 * sizeof(double))) || (rc = be_fetch(points, w.pts + b * M * 3, L * 3 * sizeof(double))) ||
        (rc = be_fetch(edge_chi2, w.chi2 + b * N, E * sizeof(double))) || (rc = be_fetch(edge_outlier, w.out + b * N, E)))
        return rc;
    if (rounds_outliers2) {
        rounds_outliers2[0] = 0; rounds_outliers2[1] = 0;
        if (E && ((rc = be_fetch(rounds_outliers2, w.rounds + b, sizeof(int32_t))) || (rc = be_fetch(rounds_outliers2 + 1, w.nout + b, sizeof(int32_t)))))
            return rc;
    }
    return MYSLAM_OK;
}

int myslam_relink_backend_batch(myslam_backend* h, const myslam_relink* rl, int64_t* d_kf_id, double* d_kf_pose, int32_t* d_n_kf, int64_t* d_mp_id,
                                double* d_mp_pos, uint8_t* d_mp_outlier, int32_t* d_n_mp, int32_t* d_obs_mp, int32_t* d_obs_kf, uint8_t* d_obs_flags,
                                float* d_obs_uv, int32_t* d_obs_tag, int32_t* d_n_obs, const int32_t* d_stage_status, int batch, int32_t* d_mp_new_row,
                                int32_t* d_status) {
    if (!h || !rl || batch < 0 || !d_kf_id || !d_kf_pose || !d_n_kf || !d_mp_id || !d_mp_pos || !d_mp_outlier || !d_n_mp || !d_obs_mp || !d_obs_kf ||
        !d_obs_flags || !d_obs_uv || !d_obs_tag || !d_n_obs || !d_stage_status || !d_mp_new_row || !d_status)
        return MYSLAM_ERR_INVALID;
    myslam_relink_lists v;
    if (myslam_relink_view(rl, &v) != MYSLAM_OK) return MYSLAM_ERR_INVALID;
    if (batch > h->max_batch || batch > v.max_batch) return MYSLAM_ERR_CAPACITY;
    if (batch == 0) return MYSLAM_OK;
    const InsTables T{d_kf_id, d_kf_pose, d_n_kf, d_mp_id, d_mp_pos, d_mp_outlier, d_n_mp, d_obs_mp, d_obs_kf, d_obs_flags, d_obs_uv, d_obs_tag, d_n_obs,
                      h->kf_cap, h->mp_cap, h->obs_cap};
    hipLaunchKernelGGL(k_backend_relink, dim3(batch), dim3(BE_NT), 0, h->stream, T, h->iw, v, d_stage_status, d_mp_new_row, d_status);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

}  // extern "C"
