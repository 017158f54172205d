// obs_archive.hip — MapPoint::GetObservations() (reference src/mappoint.cpp:19-44) of every map point that is alive and NOT in the active set, per
// stream, on the device: the list the MapPoint object keeps while the point is outside Map::_mumpActiveMapPoints (src/map.cpp:126-140) and brings back
// when a feature of a new key-frame names it again (the prior rows of myslam_backend_insert_keyframe_batch).
//   k_obs_update      one workgroup per item, after each myslam_map_update_batch: stores the rows of every point that left the back end's table alive,
//                     drops the rows of every point that returned to it, and rebuilds the MIRROR (whole rows of the back end's table with the
//                     observer's mnKFId, which a table row with d_obs_kf = -1 no longer says);
//   k_obs_prior_rows  one workgroup per item, before the insert: the stored rows of every distinct stored point a feature names, ids ascending.
// Segments are bump-allocated in one of two pools of row_cap rows; a map-point slot of the map archive (myslam_map, ids ascending and append-only)
// holds (offset, count).  When an append would not fit, the live segments go to the other pool in slot order, in the same launch.  The mirror and the
// record of the table's points are double-buffered as well, so nothing is rebuilt in place; the mirror is rebuilt one thread per row, the searches of a
// point are made once and kept in work columns.  Ids ascend in every table (sorted_rows.h), positions come
// from block scans (dev_tables.h): no global atomics, and an item's bytes depend neither on its slot nor on its neighbours.  Integer code and copies.
// See include/myslam_hip.h for the contract.
#include <algorithm>
#include <vector>

#include "dev_mem.h"
#include "dev_tables.h"

namespace myslam_hip {

constexpr int OA_NT = 256;
constexpr int OA_NW = OA_NT / WAVE;

struct OaRows {                         // observation rows: observer's mnKFId, pixel, tag, flags (OUTLIER only)
    int64_t* kf; float* uv; int32_t* tag; uint8_t* flags;
    __device__ __forceinline__ OaRows at(size_t r) const { return {kf + r, uv + 2 * r, tag + r, flags + r}; }
    __device__ __forceinline__ void copy_from(int dst, const OaRows& s, int src) const {
        kf[dst] = s.kf[src]; uv[2 * dst] = s.uv[2 * src]; uv[2 * dst + 1] = s.uv[2 * src + 1]; tag[dst] = s.tag[src]; flags[dst] = s.flags[src];
    }
};

struct OaTables {
    OaRows pool[2];                     // max_batch x row_cap each; pcur[b] says which one holds item b's segments
    OaRows mir[2];                      // max_batch x be_obs_cap each: the rows of the back end's table as of the last update; mcur[b]
    int64_t* t_mp_id[2];                // max_batch x be_mp_cap: the ids of that table's map points
    int32_t* t_off[2];                  // max_batch x (be_mp_cap + 1): where each point's segment starts; [t_n_mp] = the row count
    int32_t* t_n_mp[2];
    int32_t* seg_off; int32_t* seg_cnt; // max_batch x point_cap, by the map archive's slot; count 0 = nothing stored
    uint8_t* named;                     // max_batch x point_cap: k_obs_prior_rows' marks, all 0 between launches
    int32_t* w_s; int32_t* w_p; int32_t* w_ls; int32_t* w_lk;             // max_batch x be_mp_cap each: k_obs_update's work columns, no state
    int32_t* pcur; int32_t* mcur; int32_t* used; int32_t* n_reclaim; int32_t* err;
    const int64_t* map_mp_id; const uint8_t* map_state; const int32_t* map_n_mp;        // the map archive's, not owned
    int point_cap, row_cap, be_mp_cap, be_obs_cap;
};

struct OaUpdateIn { int mode; const int32_t* be_status; const int32_t* map_status; const uint8_t* obs_report; };

// rows of the recorded segment [o0, o1) that stay in GetObservations(): all after an insert, those the optimiser did not remove after an optimise
__device__ __forceinline__ int oa_kept(const uint8_t* report, int o0, int o1) {
    if (!report) return o1 - o0;
    int k = 0;
    for (int r = o0; r < o1; r++) k += report[r] != 1;
    return k;
}

__global__ __launch_bounds__(OA_NT) void k_obs_update(OaTables A, BeTablesRead B, OaUpdateIn U, int32_t* status) {
    __shared__ int s_w[OA_NW];
    __shared__ int s_bad, s_keep, s_leave, s_back;
    const int b = blockIdx.x, t = threadIdx.x;
    const int err = A.err[b];
    if (err) {                                                              // stale until a load
        if (t == 0) status[b] = err;
        return;
    }
    const int ms = U.map_status[b];
    if (U.be_status[b] != 0 || ms == MYSLAM_MAP_SKIPPED) {
        if (t == 0) status[b] = MYSLAM_MAP_SKIPPED;
        return;
    }
    const bool ins = U.mode == MYSLAM_MAP_AFTER_INSERT;
    const int nk = B.n_kf[b], nm = B.n_mp[b], no = B.n_obs[b], aM = A.map_n_mp[b];
    const int mc = A.mcur[b] & 1, pc = A.pcur[b] & 1, used = A.used[b];
    const int pn = A.t_n_mp[mc][b];
    const int32_t* const po = A.t_off[mc] + (size_t)b * (A.be_mp_cap + 1);
    const int pno = (pn >= 0 && pn <= A.be_mp_cap) ? po[pn] : -1;
    if (ms != MYSLAM_MAP_UPDATED || nk < 1 || nk > B.kf_cap || nm < 0 || nm > B.mp_cap || no < 0 || no > B.obs_cap || aM < 0 || aM > A.point_cap ||
        pno < 0 || pno > A.be_obs_cap || used < 0 || used > A.row_cap) {    // uniform.  The map refused its update: the table moved on without us
        if (t == 0) { A.err[b] = MYSLAM_ERR_INVALID; status[b] = MYSLAM_ERR_INVALID; }
        return;
    }
    const auto be = B.item(b);
    const int64_t* const map_id = A.map_mp_id + (size_t)b * A.point_cap;
    const uint8_t* const state = A.map_state + (size_t)b * A.point_cap;
    int32_t* const seg_off = A.seg_off + (size_t)b * A.point_cap;
    int32_t* const seg_cnt = A.seg_cnt + (size_t)b * A.point_cap;
    const int64_t* const pid = A.t_mp_id[mc] + (size_t)b * A.be_mp_cap;
    const OaRows old_mir = A.mir[mc].at((size_t)b * A.be_obs_cap), new_mir = A.mir[mc ^ 1].at((size_t)b * A.be_obs_cap);
    const OaRows old_pool = A.pool[pc].at((size_t)b * A.row_cap);
    const uint8_t* const report = ins ? nullptr : U.obs_report + (size_t)b * B.obs_cap;    // by INPUT row = the recorded table's row
    const auto seg_ok = [&](int o0, int o1) { return o0 >= 0 && o0 <= o1 && o1 <= pno; };

    // The inactive copies of the mirror and the four work columns are scratch until the flip at the end: writing them decides nothing.
    int64_t* const nid = A.t_mp_id[mc ^ 1] + (size_t)b * A.be_mp_cap;
    int32_t* const noff = A.t_off[mc ^ 1] + (size_t)b * (A.be_mp_cap + 1);
    int32_t* const w_s = A.w_s + (size_t)b * A.be_mp_cap;                   // per table point: its slot in the map, its row in the recorded table (-1: new)
    int32_t* const w_p = A.w_p + (size_t)b * A.be_mp_cap;
    int32_t* const w_ls = A.w_ls + (size_t)b * A.be_mp_cap;                 // per recorded point: its slot if it leaves alive with rows (else -1), and how many
    int32_t* const w_lk = A.w_lk + (size_t)b * A.be_mp_cap;

    // ---- where each point's segment starts, one thread per row (row `no` closes the last): d_obs_mp must be in range and non-decreasing ----
    if (t == 0) { s_bad = 0; s_keep = 0; s_leave = 0; s_back = 0; }
    __syncthreads();
    bool bad = false;
    for (int r = t; r <= no; r += OA_NT) {
        const int prev = r ? be.obs_mp[r - 1] : -1, cur = r < no ? be.obs_mp[r] : nm;
        if (prev < -1 || cur < prev || cur > nm || (r < no && cur == nm)) { bad = true; continue; }
        for (int m = prev + 1; m <= cur; m++) noff[m] = r;                  // the points between two rows have none
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (s_bad) {                                                            // uniform
        if (t == 0) { A.err[b] = MYSLAM_ERR_INVALID; status[b] = MYSLAM_ERR_INVALID; }
        return;
    }

    // ---- decide ----
    int leave = 0, keep = 0, back = 0;
    for (int m = t; m < nm; m += OA_NT) {                                   // the table's points: their rows must continue what is recorded or stored
        const int64_t id = be.mp_id[m];
        const int s = find_row(map_id, aM, id), p = find_row(pid, pn, id);
        const int n0 = noff[m], len = noff[m + 1] - n0;
        w_s[m] = s; w_p[m] = p;
        if (s < 0) { bad = true; continue; }
        if (p >= 0) {
            const int o0 = po[p], o1 = po[p + 1];
            if (!seg_ok(o0, o1)) { bad = true; continue; }
            bad |= ins ? len < o1 - o0 : len != oa_kept(report, o0, o1);
        } else if (ins) {                                                   // NEW to the table: prior rows first, then the new key-frame's
            int lead = 0;
            while (lead < len && be.obs_kf[n0 + lead] != nk - 1) lead++;
            const int c = seg_cnt[s], o = seg_off[s];
            const bool live = c > 0 && state[s] != 2;
            bad |= lead != (live ? c : 0) || (live && (o < 0 || o > A.row_cap - c));
            if (live) back += c;                                            // it RETURNED: these rows are dead from now on
        } else {
            bad = true;                                                     // an optimise adds nothing
        }
    }
    for (int p = t; p < pn; p += OA_NT) {                                   // the recorded points that are gone and alive: their rows are stored
        int ls = -1, k = 0;
        if (find_row(be.mp_id, nm, pid[p]) < 0) {
            const int s = find_row(map_id, aM, pid[p]), o0 = po[p], o1 = po[p + 1];
            if (s < 0 || !seg_ok(o0, o1)) bad = true;
            else if (state[s] != 2 && (k = oa_kept(report, o0, o1)) > 0) ls = s;
        }
        w_ls[p] = ls; w_lk[p] = ls >= 0 ? k : 0;
        leave += ls >= 0 ? k : 0;
    }
    for (int s = t; s < aM; s += OA_NT) {                                   // what is stored and alive, the returning points included
        const int c = seg_cnt[s];
        if (c <= 0 || state[s] == 2) continue;
        const int o = seg_off[s];
        if (o < 0 || o > A.row_cap - c) { bad = true; continue; }
        keep += c;
    }
    if (bad) s_bad = 1;
    if (leave) atomicAdd(&s_leave, leave);                                  // LDS
    if (keep) atomicAdd(&s_keep, keep);
    if (back) atomicAdd(&s_back, back);
    __syncthreads();
    const int n_leave = s_leave, n_keep = s_keep - s_back;                  // live rows outside the table: capacity is theirs, whatever the pool holds
    if (s_bad || n_keep < 0 || n_keep + n_leave > A.row_cap) {              // uniform; sticky, every byte kept
        const int e = (s_bad || n_keep < 0) ? MYSLAM_ERR_INVALID : MYSLAM_ERR_CAPACITY;
        if (t == 0) { A.err[b] = e; status[b] = e; }
        return;
    }

    // ---- from here on the item is written: the other mirror (one thread per row), the free rows of the pool (or the other pool), the slots ----
    const int64_t new_kf = be.kf_id[nk - 1];                                // an insert's key-frame has the highest id
    for (int r = t; r < no; r += OA_NT) {
        const int m = be.obs_mp[r], p = w_p[m], n0 = noff[m], j = r - n0;
        int64_t kf = new_kf;
        if (p >= 0) {                                                       // the observer ids of the leading rows: the old mirror's, by rank
            const int o0 = po[p], old = po[p + 1] - o0;
            if (ins) {
                if (j < old) kf = old_mir.kf[o0 + j];
            } else {
                int src = o0 + j;
                if (noff[m + 1] - n0 != old) {                              // the optimiser took rows of this point: the j-th kept one
                    src = o0 - 1;
                    for (int k = -1; k < j;) { src++; k += report[src] != 1; }
                }
                kf = old_mir.kf[src];
            }
        } else {                                                            // a returning point's: the store's
            const int s = w_s[m], c = seg_cnt[s];
            if (c > 0 && state[s] != 2 && j < c) kf = old_pool.kf[seg_off[s] + j];
        }
        new_mir.kf[r] = kf;
        new_mir.uv[2 * r] = be.obs_uv[2 * r]; new_mir.uv[2 * r + 1] = be.obs_uv[2 * r + 1];
        new_mir.tag[r] = be.obs_tag[r]; new_mir.flags[r] = be.obs_flags[r] & MYSLAM_BACKEND_OBS_OUTLIER;
    }
    __syncthreads();
    for (int m = t; m < nm; m += OA_NT) {
        nid[m] = be.mp_id[m];
        if (w_p[m] < 0) seg_cnt[w_s[m]] = 0;                                // a point that returned: its stored rows are dead
    }
    if (t == 0) A.t_n_mp[mc ^ 1][b] = nm;
    __syncthreads();

    int base = used, npc = pc;
    if (used + n_leave > A.row_cap) {                                       // reclaim: the live segments to the other pool, in slot order
        const OaRows dst = A.pool[pc ^ 1].at((size_t)b * A.row_cap);
        base = 0; npc = pc ^ 1;
        for (int s0 = 0; s0 < aM; s0 += OA_NT) {                            // uniform
            const int s = s0 + t;
            const int c = (s < aM && seg_cnt[s] > 0 && state[s] != 2) ? seg_cnt[s] : 0;
            int tot;
            const int pos = base + block_exsum<OA_NW>(c, s_w, tot);
            if (c) {
                const int o = seg_off[s];
                for (int j = 0; j < c; j++) dst.copy_from(pos + j, old_pool, o + j);
                seg_off[s] = pos;
            }
            base += tot;
        }
    }
    const OaRows dst = A.pool[npc].at((size_t)b * A.row_cap);
    for (int p0 = 0; p0 < pn; p0 += OA_NT) {                                // uniform: the leaving points in the recorded table's order
        const int p = p0 + t;
        const int s = p < pn ? w_ls[p] : -1, k = s >= 0 ? w_lk[p] : 0;
        int tot;
        const int pos = base + block_exsum<OA_NW>(k, s_w, tot);
        if (k) {
            int w = pos;
            for (int r = po[p]; r < po[p + 1]; r++)
                if (!report || report[r] != 1) dst.copy_from(w++, old_mir, r);
            seg_off[s] = pos; seg_cnt[s] = k;
        }
        base += tot;
    }
    if (t == 0) {
        A.mcur[b] = mc ^ 1; A.pcur[b] = npc; A.used[b] = base;
        if (npc != pc) A.n_reclaim[b] += 1;
        status[b] = MYSLAM_MAP_UPDATED;
    }
}

struct OaPriorIn { const int64_t* feat_mp_id; const int32_t* n_feat; int feat_cap; const int64_t* be_mp_id; const int32_t* be_n_mp; int be_mp_cap; };
struct OaPriorOut { int64_t* mp_id; OaRows rows; int32_t* n; int cap; };

__global__ __launch_bounds__(OA_NT) void k_obs_prior_rows(OaTables A, OaPriorIn I, OaPriorOut O, int32_t* status) {
    __shared__ int s_w[OA_NW];
    __shared__ int s_bad, s_total, s_lo, s_hi;
    const int b = blockIdx.x, t = threadIdx.x;
    const int err = A.err[b];
    const int nf = I.n_feat[b], nm = I.be_n_mp[b], aM = A.map_n_mp[b];
    if (err || nf < 0 || nf > I.feat_cap || nm < 0 || nm > I.be_mp_cap || aM < 0 || aM > A.point_cap) {           // uniform
        if (t == 0) { O.n[b] = 0; status[b] = err ? err : MYSLAM_ERR_INVALID; }
        return;
    }
    const int64_t* const feat = I.feat_mp_id + (size_t)b * I.feat_cap;
    const int64_t* const be_id = I.be_mp_id + (size_t)b * I.be_mp_cap;
    const int64_t* const map_id = A.map_mp_id + (size_t)b * A.point_cap;
    const uint8_t* const state = A.map_state + (size_t)b * A.point_cap;
    const int32_t* const seg_off = A.seg_off + (size_t)b * A.point_cap;
    const int32_t* const seg_cnt = A.seg_cnt + (size_t)b * A.point_cap;
    uint8_t* const named = A.named + (size_t)b * A.point_cap;
    const OaRows pool = A.pool[A.pcur[b] & 1].at((size_t)b * A.row_cap);
    // the slot of a feature's point if it is stored, alive and outside the table, else -1
    const auto slot_of = [&](int f) {
        const int64_t id = feat[f];
        if (id < 0 || find_row(be_id, nm, id) >= 0) return -1;
        const int s = find_row(map_id, aM, id);
        return (s >= 0 && state[s] != 2 && seg_cnt[s] > 0) ? s : -1;
    };
    if (t == 0) { s_bad = 0; s_total = 0; s_lo = aM; s_hi = -1; }
    __syncthreads();
    for (int f = t; f < nf; f += OA_NT) {                                   // distinct ids: a mark per slot, whoever names it
        const int s = slot_of(f);
        if (s < 0) continue;
        named[s] = 1;
        atomicMin(&s_lo, s); atomicMax(&s_hi, s);                           // LDS
    }
    __syncthreads();
    const int lo = s_lo, hi = s_hi;
    int sum = 0;
    for (int s = lo + t; s <= hi; s += OA_NT)
        if (named[s]) {
            const int c = seg_cnt[s], o = seg_off[s];
            if (o < 0 || o > A.row_cap - c) s_bad = 1;
            sum += c;
        }
    if (sum) atomicAdd(&s_total, sum);
    __syncthreads();
    const int total = s_total;
    const bool fits = !s_bad && total <= O.cap;
    if (fits) {
        int64_t* const out_id = O.mp_id + (size_t)b * O.cap;
        const OaRows out = O.rows.at((size_t)b * O.cap);
        int base = 0;
        for (int s0 = lo; s0 <= hi; s0 += OA_NT) {                          // uniform: ids ascend with the slots
            const int s = s0 + t;
            const int c = (s <= hi && named[s]) ? seg_cnt[s] : 0;
            int tot;
            const int pos = base + block_exsum<OA_NW>(c, s_w, tot);
            for (int j = 0; j < c; j++) { out_id[pos + j] = map_id[s]; out.copy_from(pos + j, pool, seg_off[s] + j); }
            base += tot;
        }
    }
    __syncthreads();
    for (int s = lo + t; s <= hi; s += OA_NT) named[s] = 0;                 // the marks go, all within [lo, hi]: the next launch finds none
    if (t == 0) {
        O.n[b] = fits ? total : 0;
        status[b] = s_bad ? MYSLAM_ERR_INVALID : (fits ? MYSLAM_OK : MYSLAM_ERR_CAPACITY);
    }
}

// ---- RE-LINK (include/myslam_hip.h): LoopLocalFusion's moved rows (reference src/loopclosing.cpp:521-525) as far as this handle holds them ----
// k_relink_stage       reads the archive (nothing of it is written): GetObservations() of every merged point — the mirror's rows for a point of the
//                      table, the stored segment else — goes to the plan handle's staging with the place each row takes in the list of the point it
//                      ends on.  The final list of a point that stands is its own rows, then for every merge into it, in order, the whole list the
//                      merged point had by then; so a merged point's OWN rows stand at one place, which one lane finds with two passes over the merge
//                      list (sizes forwards, places backwards).  Both capacities (row_cap, the back end's obs_cap) are decided here.
// k_relink_obs_update  after the back end's tables and the map's states moved: the mirror follows the table (appended rows take their observer's id
//                      from the staging), a target outside the table has its list written afresh (stored rows, then the moved ones) by update rule 6.
// k_relink_first_kf    the front observer of every point in LIST order.
struct OaSeg { int p, n; };             // row of a point in the recorded table (-1: outside) and the rows of its list, n < 0: inconsistent

__device__ __forceinline__ OaSeg oa_own(const OaTables& A, int b, int mc, int pn, int pno, int s) {
    const int64_t* const pid = A.t_mp_id[mc] + (size_t)b * A.be_mp_cap;
    const int32_t* const po = A.t_off[mc] + (size_t)b * (A.be_mp_cap + 1);
    const int p = find_row(pid, pn, A.map_mp_id[(size_t)b * A.point_cap + s]);
    if (p >= 0) {
        const int o0 = po[p], o1 = po[p + 1];
        return {p, (o0 >= 0 && o0 <= o1 && o1 <= pno) ? o1 - o0 : -1};
    }
    const int c = A.seg_cnt[(size_t)b * A.point_cap + s], o = A.seg_off[(size_t)b * A.point_cap + s];
    return {-1, (c < 0 || (c > 0 && (o < 0 || o > A.row_cap - c))) ? -1 : c};
}

__global__ __launch_bounds__(OA_NT) void k_relink_stage(OaTables A, myslam_relink_lists R, const int32_t* plan_status, int32_t* status) {
    __shared__ int s_bad, s_live, s_code, s_total;
    const int b = blockIdx.x, t = threadIdx.x;
    const auto none = [&](int code) { if (t == 0) { R.n_rows[b] = 0; R.n_staged_merges[b] = 0; status[b] = code; } };
    const int err = A.err[b];
    if (err) { none(err); return; }
    if (plan_status[b] != MYSLAM_RELINK_DONE) { none(MYSLAM_RELINK_SKIPPED); return; }
    const int nmg = R.n_merge[b], aM = A.map_n_mp[b];
    const int mc = A.mcur[b] & 1, pc = A.pcur[b] & 1;
    const int pn = A.t_n_mp[mc][b];
    const int32_t* const po = A.t_off[mc] + (size_t)b * (A.be_mp_cap + 1);
    const int pno = (pn >= 0 && pn <= A.be_mp_cap) ? po[pn] : -1;
    if (nmg < 0 || nmg > R.out_cap || aM < 0 || aM > A.point_cap || pno < 0 || pno > A.be_obs_cap) { none(MYSLAM_ERR_INVALID); return; }      // uniform
    const int32_t* const merge = R.merge + (size_t)b * R.out_cap * 2;
    const int32_t* const target = R.target + (size_t)b * R.point_cap;
    const int64_t* const map_id = A.map_mp_id + (size_t)b * A.point_cap;
    const uint8_t* const state = A.map_state + (size_t)b * A.point_cap;
    const int32_t* const seg_off = A.seg_off + (size_t)b * A.point_cap;
    const int32_t* const seg_cnt = A.seg_cnt + (size_t)b * A.point_cap;
    const int64_t* const pid = A.t_mp_id[mc] + (size_t)b * A.be_mp_cap;
    int32_t* const wsz = R.work_size + (size_t)b * R.point_cap;
    int64_t* const mg_from = R.merge_from_id + (size_t)b * R.out_cap;
    int64_t* const mg_root = R.merge_root_id + (size_t)b * R.out_cap;
    int32_t* const mg_rows = R.merge_rows + (size_t)b * R.out_cap;
    int32_t* const mg_place = R.merge_place + (size_t)b * R.out_cap;
    if (t == 0) { s_bad = 0; s_live = 0; s_code = 0; s_total = 0; }
    __syncthreads();
    bool bad = false;
    for (int i = t; i < nmg; i += OA_NT) {                                  // every slot in range and alive, every merged point's end a point that stands
        const int x = merge[2 * i], y = merge[2 * i + 1];
        if (x < 0 || x >= aM || y < 0 || y >= aM || x == y || state[x] == 2 || state[y] == 2) { bad = true; continue; }
        const int r = target[x];
        if (r < 0 || r >= aM || target[r] != r || state[r] == 2) { bad = true; continue; }
        const OaSeg ox = oa_own(A, b, mc, pn, pno, x), oy = oa_own(A, b, mc, pn, pno, y);
        if (ox.n < 0 || oy.n < 0) { bad = true; continue; }
        wsz[x] = ox.n; wsz[y] = oy.n;                                       // (whoever writes a slot writes the same number)
        mg_from[i] = map_id[x]; mg_root[i] = map_id[r]; mg_rows[i] = ox.n;
    }
    int live = 0;
    for (int s = t; s < aM; s += OA_NT) {
        const int c = seg_cnt[s];
        if (c <= 0 || state[s] == 2) continue;
        if (seg_off[s] < 0 || seg_off[s] > A.row_cap - c) { bad = true; continue; }
        live += c;
    }
    if (bad) s_bad = 1;
    if (live) atomicAdd(&s_live, live);                                     // LDS
    __syncthreads();
    if (s_bad) { none(MYSLAM_ERR_INVALID); return; }                        // uniform
    if (t == 0) {
        for (int i = 0; i < nmg; i++) {                                     // sizes forwards: where the merged point's list starts in its target's
            const int x = merge[2 * i], y = merge[2 * i + 1];
            mg_place[i] = wsz[y]; wsz[y] += wsz[x];
        }
        long long n_table = pno, out_rows = s_live, total = 0;
        for (int i = nmg - 1; i >= 0; i--) {                                // places backwards: a target that was merged later has its own place by now
            const int x = merge[2 * i], y = merge[2 * i + 1];
            const int place = mg_place[i] + (target[y] == y ? 0 : wsz[y]);
            wsz[x] = place; mg_place[i] = place;
            const int c = mg_rows[i];
            const bool from_in = find_row(pid, pn, mg_from[i]) >= 0, root_in = find_row(pid, pn, mg_root[i]) >= 0;
            n_table += (root_in ? c : 0) - (from_in ? c : 0);
            out_rows += (root_in ? 0 : c) - (from_in ? 0 : c);
            total += c;
        }
        if (total > R.stage_cap || n_table > A.be_obs_cap || out_rows > A.row_cap) s_code = MYSLAM_ERR_CAPACITY;
        s_total = (int)(total > R.stage_cap ? 0 : total);
    }
    __syncthreads();
    if (s_code) { none(s_code); return; }                                   // uniform; nothing of any table was written
    const OaRows mir = A.mir[mc].at((size_t)b * A.be_obs_cap), pool = A.pool[pc].at((size_t)b * A.row_cap);
    const OaRows dst{R.row_kf_id + (size_t)b * R.stage_cap, R.row_uv + (size_t)b * R.stage_cap * 2, R.row_tag + (size_t)b * R.stage_cap,
                     R.row_flags + (size_t)b * R.stage_cap};
    int base = 0;
    for (int i = 0; i < nmg; i++) {                                         // uniform: the own rows of every merged point, merge by merge
        const int x = merge[2 * i], c = mg_rows[i];
        const int p = find_row(pid, pn, mg_from[i]);
        const int src0 = p >= 0 ? po[p] : seg_off[x];
        for (int j = t; j < c; j += OA_NT) {
            const size_t d = (size_t)base + j;
            dst.copy_from((int)d, p >= 0 ? mir : pool, src0 + j);
            R.row_root_id[(size_t)b * R.stage_cap + d] = mg_root[i]; R.row_slot[(size_t)b * R.stage_cap + d] = target[x];
            R.row_place[(size_t)b * R.stage_cap + d] = mg_place[i] + j;
        }
        base += c;
    }
    if (t == 0) { R.n_rows[b] = s_total; R.n_staged_merges[b] = nmg; R.table_mp[b] = pn; R.table_rows[b] = pno; status[b] = MYSLAM_RELINK_DONE; }
}

__global__ __launch_bounds__(OA_NT) void k_relink_obs_update(OaTables A, BeTablesRead B, myslam_relink_lists R, const int32_t* be_status, const int32_t* map_status,
                                                             int32_t* status) {
    __shared__ int s_w[OA_NW];
    __shared__ int s_bad, s_keep, s_new, s_lo, s_hi;
    const int b = blockIdx.x, t = threadIdx.x;
    const int err = A.err[b];
    if (err) { if (t == 0) status[b] = err; return; }
    const int ms = map_status[b];
    if (be_status[b] != 0 || ms == MYSLAM_MAP_SKIPPED) { if (t == 0) status[b] = MYSLAM_MAP_SKIPPED; return; }
    const int nk = B.n_kf[b], nm = B.n_mp[b], no = B.n_obs[b], aM = A.map_n_mp[b];
    const int mc = A.mcur[b] & 1, pc = A.pcur[b] & 1, used = A.used[b];
    const int pn = A.t_n_mp[mc][b];
    const int32_t* const po = A.t_off[mc] + (size_t)b * (A.be_mp_cap + 1);
    const int pno = (pn >= 0 && pn <= A.be_mp_cap) ? po[pn] : -1;
    const int nmg = R.n_staged_merges[b], nst = R.n_rows[b];
    if (ms != MYSLAM_MAP_UPDATED || nk < 1 || nk > B.kf_cap || nm < 0 || nm > B.mp_cap || no < 0 || no > B.obs_cap || aM < 0 || aM > A.point_cap || pno < 0 ||
        pno > A.be_obs_cap || used < 0 || used > A.row_cap || nmg < 0 || nmg > R.out_cap || nst < 0 || nst > R.stage_cap || R.table_mp[b] != pn ||
        R.table_rows[b] != pno) {                                           // uniform: the staging is not of this mirror
        if (t == 0) { A.err[b] = MYSLAM_ERR_INVALID; status[b] = MYSLAM_ERR_INVALID; }                          // sticky, every byte kept
        return;
    }
    const auto be = B.item(b);
    const int64_t* const map_id = A.map_mp_id + (size_t)b * A.point_cap;
    const uint8_t* const state = A.map_state + (size_t)b * A.point_cap;
    int32_t* const seg_off = A.seg_off + (size_t)b * A.point_cap;
    int32_t* const seg_cnt = A.seg_cnt + (size_t)b * A.point_cap;
    uint8_t* const named = A.named + (size_t)b * A.point_cap;
    const int64_t* const pid = A.t_mp_id[mc] + (size_t)b * A.be_mp_cap;
    const OaRows old_mir = A.mir[mc].at((size_t)b * A.be_obs_cap), new_mir = A.mir[mc ^ 1].at((size_t)b * A.be_obs_cap);
    const OaRows old_pool = A.pool[pc].at((size_t)b * A.row_cap);
    int64_t* const nid = A.t_mp_id[mc ^ 1] + (size_t)b * A.be_mp_cap;
    int32_t* const noff = A.t_off[mc ^ 1] + (size_t)b * (A.be_mp_cap + 1);
    int32_t* const w_p = A.w_p + (size_t)b * A.be_mp_cap;                   // per table point: its row in the recorded table, the rows it received
    int32_t* const w_add = A.w_lk + (size_t)b * A.be_mp_cap;
    int32_t* const wsz = R.work_size + (size_t)b * R.point_cap;             // per target outside the table: the rows it receives
    const int32_t* const merge = R.merge + (size_t)b * R.out_cap * 2;
    const int32_t* const target = R.target + (size_t)b * R.point_cap;
    const int64_t* const mg_root = R.merge_root_id + (size_t)b * R.out_cap;
    const int32_t* const mg_rows = R.merge_rows + (size_t)b * R.out_cap;
    const size_t sb = (size_t)b * R.stage_cap;
    if (t == 0) { s_bad = 0; s_keep = 0; s_new = 0; s_lo = aM; s_hi = -1; }
    __syncthreads();
    bool bad = false;
    for (int r = t; r <= no; r += OA_NT) {                                  // segment starts, as k_obs_update
        const int prev = r ? be.obs_mp[r - 1] : -1, cur = r < no ? be.obs_mp[r] : nm;
        if (prev < -1 || cur < prev || cur > nm || (r < no && cur == nm)) { bad = true; continue; }
        for (int m = prev + 1; m <= cur; m++) noff[m] = r;
    }
    for (int m = t; m < nm; m += OA_NT) w_add[m] = 0;
    for (int i = t; i < nmg; i += OA_NT) {                                  // the slots the merged rows end on
        const int x = merge[2 * i];
        const int r = (x >= 0 && x < aM) ? target[x] : -1;
        if (r < 0 || r >= aM || state[r] == 2) { bad = true; continue; }
        wsz[r] = 0;
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (s_bad) {                                                            // uniform
        if (t == 0) { A.err[b] = MYSLAM_ERR_INVALID; status[b] = MYSLAM_ERR_INVALID; }
        return;
    }
    if (t == 0)
        for (int i = 0; i < nmg; i++) {                                     // rows received, by table row or by slot
            const int rr = find_row(be.mp_id, nm, mg_root[i]);
            if (rr >= 0) w_add[rr] += mg_rows[i]; else wsz[target[merge[2 * i]]] += mg_rows[i];
        }
    __syncthreads();
    // ---- decide ----
    for (int m = t; m < nm; m += OA_NT) {                                   // every point of the table was in it, and holds what it held plus what it received
        const int p = find_row(pid, pn, be.mp_id[m]);
        w_p[m] = p;
        if (p < 0 || find_row(map_id, aM, be.mp_id[m]) < 0) { bad = true; continue; }
        const int o0 = po[p], o1 = po[p + 1];
        bad |= !(o0 >= 0 && o0 <= o1 && o1 <= pno) || noff[m + 1] - noff[m] != o1 - o0 + w_add[m];
    }
    for (int p = t; p < pn; p += OA_NT)                                     // a recorded point that is gone was merged away: erased by now
        if (find_row(be.mp_id, nm, pid[p]) < 0) { const int s = find_row(map_id, aM, pid[p]); bad |= s < 0 || state[s] != 2; }
    for (int i = t; i < nmg; i += OA_NT) {                                  // the targets outside the table: marked, whoever names them
        const int r = target[merge[2 * i]];
        if (find_row(be.mp_id, nm, mg_root[i]) >= 0 || wsz[r] <= 0) continue;
        named[r] = 1;
        atomicMin(&s_lo, r); atomicMax(&s_hi, r);                           // LDS
    }
    for (int d = t; d < nst; d += OA_NT) {                                  // a staged row of a table point stands behind the rows the point had
        const int rr = find_row(be.mp_id, nm, R.row_root_id[sb + d]);
        const int place = R.row_place[sb + d];
        if (rr < 0) {                                                       // of a point outside the table: behind its stored rows, within what it receives
            const int s = R.row_slot[sb + d];
            if (s < 0 || s >= aM || state[s] == 2) { bad = true; continue; }
            const int c = seg_cnt[s] > 0 ? seg_cnt[s] : 0;
            bad |= place < c || place - c >= wsz[s] || (R.row_flags[sb + d] & ~MYSLAM_BACKEND_OBS_OUTLIER);
            continue;
        }
        const int p = find_row(pid, pn, be.mp_id[rr]);
        bad |= p < 0 || place < po[p + 1] - po[p] || place >= noff[rr + 1] - noff[rr];
    }
    if (bad) s_bad = 1;
    __syncthreads();
    const int lo = s_lo, hi = s_hi;
    int keep = 0, fresh = 0;
    for (int s = t; s < aM; s += OA_NT) {
        const int c = (seg_cnt[s] > 0 && state[s] != 2) ? seg_cnt[s] : 0;
        if (c && (seg_off[s] < 0 || seg_off[s] > A.row_cap - c)) { s_bad = 1; continue; }
        if (s >= lo && s <= hi && named[s]) fresh += c + wsz[s]; else keep += c;
    }
    if (keep) atomicAdd(&s_keep, keep);
    if (fresh) atomicAdd(&s_new, fresh);
    __syncthreads();
    const int n_new = s_new;
    if (s_bad || s_keep + n_new > A.row_cap) {                              // uniform; sticky, every byte kept (the marks go)
        for (int s = lo + t; s <= hi; s += OA_NT) named[s] = 0;
        const int e = s_bad ? MYSLAM_ERR_INVALID : MYSLAM_ERR_CAPACITY;
        if (t == 0) { A.err[b] = e; status[b] = e; }
        return;
    }
    // ---- from here on the item is written: the other mirror, the free rows of the pool (or the other pool), the slots ----
    for (int r = t; r < no; r += OA_NT) {
        const int m = be.obs_mp[r], p = w_p[m], j = r - noff[m];
        if (j < po[p + 1] - po[p]) new_mir.kf[r] = old_mir.kf[po[p] + j];
        new_mir.uv[2 * r] = be.obs_uv[2 * r]; new_mir.uv[2 * r + 1] = be.obs_uv[2 * r + 1];
        new_mir.tag[r] = be.obs_tag[r]; new_mir.flags[r] = be.obs_flags[r] & MYSLAM_BACKEND_OBS_OUTLIER;
    }
    for (int d = t; d < nst; d += OA_NT) {                                  // the appended rows' observers
        const int rr = find_row(be.mp_id, nm, R.row_root_id[sb + d]);
        if (rr >= 0) new_mir.kf[noff[rr] + R.row_place[sb + d]] = R.row_kf_id[sb + d];
    }
    for (int m = t; m < nm; m += OA_NT) nid[m] = be.mp_id[m];
    if (t == 0) A.t_n_mp[mc ^ 1][b] = nm;
    int base = used, npc = pc;
    if (used + n_new > A.row_cap) {                                         // reclaim: the live segments that are not written afresh, in slot order
        const OaRows dst = A.pool[pc ^ 1].at((size_t)b * A.row_cap);
        base = 0; npc = pc ^ 1;
        for (int s0 = 0; s0 < aM; s0 += OA_NT) {                            // uniform
            const int s = s0 + t;
            const int c = (s < aM && seg_cnt[s] > 0 && state[s] != 2 && !(s >= lo && s <= hi && named[s])) ? seg_cnt[s] : 0;
            int tot;
            const int pos = base + block_exsum<OA_NW>(c, s_w, tot);
            if (c) {
                const int o = seg_off[s];
                for (int j = 0; j < c; j++) dst.copy_from(pos + j, old_pool, o + j);
                seg_off[s] = pos;
            }
            base += tot;
        }
    }
    const OaRows dst = A.pool[npc].at((size_t)b * A.row_cap);
    for (int s0 = lo; s0 <= hi; s0 += OA_NT) {                              // uniform: the targets outside the table, in slot order
        const int s = s0 + t;
        const bool on = s <= hi && named[s];
        const int c = (on && seg_cnt[s] > 0) ? seg_cnt[s] : 0, k = on ? c + wsz[s] : 0;
        int tot;
        const int pos = base + block_exsum<OA_NW>(k, s_w, tot);
        if (on) {
            const int o = seg_off[s];
            for (int j = 0; j < c; j++) dst.copy_from(pos + j, old_pool, o + j);
            seg_off[s] = pos; seg_cnt[s] = k;
        }
        base += tot;
    }
    __syncthreads();
    const OaRows stg{R.row_kf_id + sb, R.row_uv + sb * 2, R.row_tag + sb, R.row_flags + sb};
    for (int d = t; d < nst; d += OA_NT) {                                  // the moved rows behind them, each at its place
        const int s = R.row_slot[sb + d];
        if (s >= lo && s <= hi && named[s]) dst.copy_from(seg_off[s] + R.row_place[sb + d], stg, d);
    }
    __syncthreads();
    for (int s = lo + t; s <= hi; s += OA_NT) named[s] = 0;
    if (t == 0) {
        A.mcur[b] = mc ^ 1; A.pcur[b] = npc; A.used[b] = base;
        if (npc != pc) A.n_reclaim[b] += 1;
        status[b] = MYSLAM_MAP_UPDATED;
    }
}

__global__ __launch_bounds__(OA_NT) void k_relink_first_kf(OaTables A, const int64_t* map_kf_id, const int32_t* map_n_kf, int kf_cap, int32_t* first_kf) {
    const int b = blockIdx.y, s = blockIdx.x * OA_NT + threadIdx.x;
    const int aM = clamped_count(A.map_n_mp, b, A.point_cap);
    if (s >= aM) return;
    int out = -1;
    const int mc = A.mcur[b] & 1, pc = A.pcur[b] & 1;
    const int pn = A.t_n_mp[mc][b];
    const int32_t* const po = A.t_off[mc] + (size_t)b * (A.be_mp_cap + 1);
    const int pno = (pn >= 0 && pn <= A.be_mp_cap) ? po[pn] : -1;
    if (!A.err[b] && pno >= 0 && pno <= A.be_obs_cap && A.map_state[(size_t)b * A.point_cap + s] != 2) {
        const OaSeg o = oa_own(A, b, mc, pn, pno, s);
        if (o.n > 0) {
            const int64_t kf = o.p >= 0 ? A.mir[mc].kf[(size_t)b * A.be_obs_cap + po[o.p]] : A.pool[pc].kf[(size_t)b * A.row_cap + A.seg_off[(size_t)b * A.point_cap + s]];
            out = find_row(map_kf_id + (size_t)b * kf_cap, clamped_count(map_n_kf, b, kf_cap), kf);
        }
    }
    first_kf[(size_t)b * A.point_cap + s] = out;
}

}  // namespace myslam_hip

using namespace myslam_hip;

struct myslam_obs_archive {
    int max_batch = 0;
    hipStream_t stream = nullptr;
    OaTables t{};
    myslam_map_tables map{};
    BufSet mem;                         // owns every block that `t` names, the map's excepted
};

static int oa_copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    if (!dst || !src || bytes == 0) return MYSLAM_OK;
    const hipStream_t st = host_call_stream();
    if (!st) return MYSLAM_ERR_HIP;
    return copy_sync(dst, src, bytes, kind, st);
}
static int oa_up(void* dst, const void* src, size_t bytes) { return oa_copy(dst, src, bytes, hipMemcpyHostToDevice); }
static int oa_down(void* dst, const void* src, size_t bytes) { return oa_copy(dst, src, bytes, hipMemcpyDeviceToHost); }

static int oa_up_rows(const OaRows& r, size_t at, const int64_t* kf, const float* uv, const int32_t* tag, const uint8_t* flags, size_t n) {
    int rc;
    if ((rc = oa_up(r.kf + at, kf, n * sizeof(int64_t))) || (rc = oa_up(r.uv + 2 * at, uv, n * 2 * sizeof(float))) ||
        (rc = oa_up(r.tag + at, tag, n * sizeof(int32_t))) || (rc = oa_up(r.flags + at, flags, n)))
        return rc;
    return MYSLAM_OK;
}

// the map archive's ids and states of one item, on the host (load and get are synchronous)
static int oa_map_item(const myslam_obs_archive* h, int item, std::vector<int64_t>& id, std::vector<uint8_t>& state) {
    int32_t n = 0;
    int rc;
    if ((rc = oa_down(&n, h->map.n_mp + item, sizeof(n)))) return rc;
    const size_t nm = (size_t)clamped_count(n, h->t.point_cap);
    id.assign(nm, 0); state.assign(nm, 0);
    if ((rc = oa_down(id.data(), h->map.mp_id + (size_t)item * h->t.point_cap, nm * sizeof(int64_t))) ||
        (rc = oa_down(state.data(), h->map.mp_state + (size_t)item * h->t.point_cap, nm)))
        return rc;
    return MYSLAM_OK;
}

extern "C" {

int myslam_obs_archive_create(myslam_obs_archive** out, const myslam_map* map, int max_batch, int be_obs_cap, int row_cap) {
    if (!out || !map || max_batch < 1 || be_obs_cap < 1 || row_cap < 1) return MYSLAM_ERR_INVALID;
    myslam_map_tables mv;
    if (myslam_map_view(map, &mv) != MYSLAM_OK) return MYSLAM_ERR_INVALID;
    if (max_batch > mv.max_batch) return MYSLAM_ERR_INVALID;
    if (be_obs_cap > (1 << 24) || row_cap > (1 << 26)) return MYSLAM_ERR_CAPACITY;
    if (need_device()) return MYSLAM_ERR_HIP;
    myslam_obs_archive* h = new myslam_obs_archive();
    h->max_batch = max_batch; h->map = mv;
    OaTables& t = h->t;
    t.point_cap = mv.point_cap; t.row_cap = row_cap; t.be_mp_cap = mv.backend_mp_cap; t.be_obs_cap = be_obs_cap;
    t.map_mp_id = mv.mp_id; t.map_state = mv.mp_state; t.map_n_mp = mv.n_mp;
    const size_t B = (size_t)max_batch, P = (size_t)mv.point_cap, R = (size_t)row_cap, M = (size_t)mv.backend_mp_cap, O = (size_t)be_obs_cap;
    auto own = [&](auto*& p, size_t n) { return h->mem.own(p, n, MYSLAM_ERR_CAPACITY); };
    auto own_rows = [&](OaRows& r, size_t n) {
        int rc;
        if ((rc = own(r.kf, n)) || (rc = own(r.uv, 2 * n)) || (rc = own(r.tag, n)) || (rc = own(r.flags, n))) return rc;
        return (int)MYSLAM_OK;
    };
    int rc = MYSLAM_OK;
    for (int i = 0; i < 2 && !rc; i++)
        (void)((rc = own_rows(t.pool[i], B * R)) || (rc = own_rows(t.mir[i], B * O)) || (rc = own(t.t_mp_id[i], B * M)) || (rc = own(t.t_off[i], B * (M + 1))) ||
               (rc = own(t.t_n_mp[i], B)));
    if (!rc)
        (void)((rc = own(t.seg_off, B * P)) || (rc = own(t.seg_cnt, B * P)) || (rc = own(t.named, B * P)) || (rc = own(t.w_s, B * M)) || (rc = own(t.w_p, B * M)) ||
               (rc = own(t.w_ls, B * M)) || (rc = own(t.w_lk, B * M)) || (rc = own(t.pcur, B)) || (rc = own(t.mcur, B)) ||
               (rc = own(t.used, B)) || (rc = own(t.n_reclaim, B)) || (rc = own(t.err, B)));
    if (rc) { delete h; return rc; }
    const std::vector<int32_t> zeros(std::max(B * P, B * (M + 1)), 0);      // every store starts empty, every recorded table too
    for (int32_t* p : {t.seg_off, t.seg_cnt})
        if ((rc = upload_table(p, zeros.data(), B * P * sizeof(int32_t)))) { delete h; return rc; }
    if ((rc = upload_table(t.named, zeros.data(), B * P))) { delete h; return rc; }
    for (int32_t* p : {t.t_off[0], t.t_off[1]})
        if ((rc = upload_table(p, zeros.data(), B * (M + 1) * sizeof(int32_t)))) { delete h; return rc; }
    for (int32_t* p : {t.t_n_mp[0], t.t_n_mp[1], t.pcur, t.mcur, t.used, t.n_reclaim, t.err})
        if ((rc = upload_table(p, zeros.data(), B * sizeof(int32_t)))) { delete h; return rc; }
    *out = h;
    return MYSLAM_OK;
}

int myslam_obs_archive_destroy(myslam_obs_archive* h) {
    if (!h) return MYSLAM_ERR_INVALID;
    (void)hipStreamSynchronize(h->stream);
    delete h;
    return MYSLAM_OK;
}

int myslam_obs_archive_set_stream(myslam_obs_archive* h, void* hip_stream) {
    if (!h) return MYSLAM_ERR_INVALID;
    h->stream = (hipStream_t)hip_stream;
    return MYSLAM_OK;
}

int myslam_obs_archive_launches_per_update(const myslam_obs_archive* h) { return h ? 1 : MYSLAM_ERR_INVALID; }

int myslam_obs_archive_load(myslam_obs_archive* h, int item, const int64_t* seg_mp_id, const int32_t* seg_count, int n_seg, const int64_t* row_kf_id,
                            const float* row_uv, const int32_t* row_tag, const uint8_t* row_flags, int n_rows, const int64_t* table_mp_id,
                            const int32_t* table_mp_rows, int n_table_mp, const int64_t* table_kf_id, const float* table_uv, const int32_t* table_tag,
                            const uint8_t* table_flags, int n_table_rows) {
    if (!h || item < 0 || item >= h->max_batch) return MYSLAM_ERR_INVALID;
    const OaTables& t = h->t;
    if (n_seg < 0 || n_rows < 0 || n_table_mp < 0 || n_table_rows < 0) return MYSLAM_ERR_INVALID;
    if (n_rows > t.row_cap || n_seg > t.point_cap || n_table_mp > t.be_mp_cap || n_table_rows > t.be_obs_cap) return MYSLAM_ERR_CAPACITY;
    if ((n_seg && (!seg_mp_id || !seg_count)) || (n_rows && (!row_kf_id || !row_uv || !row_tag || !row_flags)) ||
        (n_table_mp && (!table_mp_id || !table_mp_rows)) || (n_table_rows && (!table_kf_id || !table_uv || !table_tag || !table_flags)))
        return MYSLAM_ERR_INVALID;
    int64_t sum = 0;
    for (int i = 0; i < n_seg; i++) {
        if ((i && seg_mp_id[i - 1] >= seg_mp_id[i]) || seg_count[i] < 1) return MYSLAM_ERR_INVALID;
        sum += seg_count[i];
    }
    if (sum != n_rows) return MYSLAM_ERR_INVALID;
    sum = 0;
    for (int i = 0; i < n_table_mp; i++) {
        if ((i && table_mp_id[i - 1] >= table_mp_id[i]) || table_mp_rows[i] < 0) return MYSLAM_ERR_INVALID;
        sum += table_mp_rows[i];
    }
    if (sum != n_table_rows) return MYSLAM_ERR_INVALID;
    for (int i = 0; i < n_rows; i++) if (row_flags[i] & ~MYSLAM_BACKEND_OBS_OUTLIER) return MYSLAM_ERR_INVALID;
    for (int i = 0; i < n_table_rows; i++) if (table_flags[i] & ~MYSLAM_BACKEND_OBS_OUTLIER) return MYSLAM_ERR_INVALID;
    if (stream_is_capturing(h->stream)) return MYSLAM_ERR_UNSUPPORTED;
    MYSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    std::vector<int64_t> map_id; std::vector<uint8_t> state;
    int rc;
    if ((rc = oa_map_item(h, item, map_id, state))) return rc;
    const size_t P = (size_t)t.point_cap, b = (size_t)item;
    std::vector<int32_t> off(P, 0), cnt(P, 0), toff((size_t)n_table_mp + 1, 0);
    int at = 0;
    for (int i = 0; i < n_seg; i++) {                                       // a stored point is one the map holds alive and the table does not
        const int s = find_row(map_id.data(), (int)map_id.size(), seg_mp_id[i]);
        if (s < 0 || state[s] == 2 || find_row(table_mp_id, n_table_mp, seg_mp_id[i]) >= 0) return MYSLAM_ERR_INVALID;
        off[s] = at; cnt[s] = seg_count[i]; at += seg_count[i];
    }
    for (int i = 0; i < n_table_mp; i++) toff[i + 1] = toff[i] + table_mp_rows[i];
    const int32_t zero = 0, n_tmp = n_table_mp, n_used = n_rows;
    const std::vector<uint8_t> no_marks(P, 0);
    if ((rc = oa_up_rows(t.pool[0], b * t.row_cap, row_kf_id, row_uv, row_tag, row_flags, (size_t)n_rows)) ||
        (rc = oa_up_rows(t.mir[0], b * t.be_obs_cap, table_kf_id, table_uv, table_tag, table_flags, (size_t)n_table_rows)) ||
        (rc = oa_up(t.t_mp_id[0] + b * t.be_mp_cap, table_mp_id, n_table_mp * sizeof(int64_t))) ||
        (rc = oa_up(t.t_off[0] + b * (t.be_mp_cap + 1), toff.data(), toff.size() * sizeof(int32_t))) || (rc = oa_up(t.t_n_mp[0] + b, &n_tmp, 4)) ||
        (rc = oa_up(t.seg_off + b * P, off.data(), P * sizeof(int32_t))) || (rc = oa_up(t.seg_cnt + b * P, cnt.data(), P * sizeof(int32_t))) ||
        (rc = oa_up(t.named + b * P, no_marks.data(), P)) || (rc = oa_up(t.pcur + b, &zero, 4)) || (rc = oa_up(t.mcur + b, &zero, 4)) ||
        (rc = oa_up(t.used + b, &n_used, 4)) || (rc = oa_up(t.n_reclaim + b, &zero, 4)) || (rc = oa_up(t.err + b, &zero, 4)))
        return rc;
    return MYSLAM_OK;
}

int myslam_obs_archive_get(myslam_obs_archive* h, int item, int64_t* seg_mp_id, int32_t* seg_count, int* n_seg, int64_t* row_kf_id, float* row_uv,
                           int32_t* row_tag, uint8_t* row_flags, int* n_rows, int64_t* table_mp_id, int32_t* table_mp_rows, int* n_table_mp,
                           int64_t* table_kf_id, float* table_uv, int32_t* table_tag, uint8_t* table_flags, int* n_table_rows, int* rows_in_use,
                           int* n_reclaims, int* error) {
    if (!h || item < 0 || item >= h->max_batch) return MYSLAM_ERR_INVALID;
    if (stream_is_capturing(h->stream)) return MYSLAM_ERR_UNSUPPORTED;
    MYSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    const OaTables& t = h->t;
    const size_t P = (size_t)t.point_cap, R = (size_t)t.row_cap, M = (size_t)t.be_mp_cap, O = (size_t)t.be_obs_cap, b = (size_t)item;
    std::vector<int64_t> map_id; std::vector<uint8_t> state;
    int32_t pcur = 0, mcur = 0, used = 0, nrec = 0, err = 0, ntm = 0;
    int rc;
    if ((rc = oa_map_item(h, item, map_id, state)) || (rc = oa_down(&pcur, t.pcur + b, 4)) || (rc = oa_down(&mcur, t.mcur + b, 4)) ||
        (rc = oa_down(&used, t.used + b, 4)) || (rc = oa_down(&nrec, t.n_reclaim + b, 4)) || (rc = oa_down(&err, t.err + b, 4)))
        return rc;
    pcur &= 1; mcur &= 1;
    if ((rc = oa_down(&ntm, t.t_n_mp[mcur] + b, 4))) return rc;
    ntm = clamped_count(ntm, t.be_mp_cap);
    const size_t nP = map_id.size();
    std::vector<int32_t> off(nP), cnt(nP), toff((size_t)ntm + 1);
    std::vector<int64_t> kf(R); std::vector<float> uv(2 * R); std::vector<int32_t> tag(R); std::vector<uint8_t> flags(R);
    const OaRows& pool = t.pool[pcur];
    if ((rc = oa_down(off.data(), t.seg_off + b * P, nP * sizeof(int32_t))) || (rc = oa_down(cnt.data(), t.seg_cnt + b * P, nP * sizeof(int32_t))) ||
        (rc = oa_down(toff.data(), t.t_off[mcur] + b * (M + 1), toff.size() * sizeof(int32_t))) || (rc = oa_down(kf.data(), pool.kf + b * R, R * sizeof(int64_t))) ||
        (rc = oa_down(uv.data(), pool.uv + 2 * b * R, 2 * R * sizeof(float))) || (rc = oa_down(tag.data(), pool.tag + b * R, R * sizeof(int32_t))) ||
        (rc = oa_down(flags.data(), pool.flags + b * R, R)))
        return rc;
    size_t ns = 0, nr = 0;
    for (size_t s = 0; s < nP; s++) {                                       // live segments only, ids ascending with the slots
        const int c = cnt[s], o = off[s];
        if (c <= 0 || state[s] == 2 || o < 0 || (size_t)o + (size_t)c > R || nr + (size_t)c > R) continue;
        if (seg_mp_id) seg_mp_id[ns] = map_id[s];
        if (seg_count) seg_count[ns] = c;
        for (int j = 0; j < c; j++, nr++) {
            if (row_kf_id) row_kf_id[nr] = kf[o + j];
            if (row_uv) { row_uv[2 * nr] = uv[2 * (o + j)]; row_uv[2 * nr + 1] = uv[2 * (o + j) + 1]; }
            if (row_tag) row_tag[nr] = tag[o + j];
            if (row_flags) row_flags[nr] = flags[o + j];
        }
        ns++;
    }
    const size_t ntr = (size_t)clamped_count(toff[ntm], t.be_obs_cap);
    const OaRows& mir = t.mir[mcur];
    if ((rc = oa_down(table_mp_id, t.t_mp_id[mcur] + b * M, (size_t)ntm * sizeof(int64_t))) || (rc = oa_down(table_kf_id, mir.kf + b * O, ntr * sizeof(int64_t))) ||
        (rc = oa_down(table_uv, mir.uv + 2 * b * O, 2 * ntr * sizeof(float))) || (rc = oa_down(table_tag, mir.tag + b * O, ntr * sizeof(int32_t))) ||
        (rc = oa_down(table_flags, mir.flags + b * O, ntr)))
        return rc;
    if (table_mp_rows) for (int i = 0; i < ntm; i++) table_mp_rows[i] = toff[i + 1] - toff[i];
    if (n_seg) *n_seg = (int)ns;
    if (n_rows) *n_rows = (int)nr;
    if (n_table_mp) *n_table_mp = ntm;
    if (n_table_rows) *n_table_rows = (int)ntr;
    if (rows_in_use) *rows_in_use = used;
    if (n_reclaims) *n_reclaims = nrec;
    if (error) *error = err;
    return MYSLAM_OK;
}

int myslam_obs_archive_update_batch(myslam_obs_archive* h, int mode, const int64_t* d_kf_id, const double* d_kf_pose, const int32_t* d_n_kf,
                                    const int64_t* d_mp_id, const double* d_mp_pos, const uint8_t* d_mp_outlier, const int32_t* d_n_mp,
                                    const int32_t* d_obs_mp, const int32_t* d_obs_kf, const uint8_t* d_obs_flags, const float* d_obs_uv,
                                    const int32_t* d_obs_tag, const int32_t* d_n_obs, int be_kf_cap, int be_mp_cap, int be_obs_cap,
                                    const int32_t* d_backend_status, const int32_t* d_map_status, const uint8_t* d_obs_report, int batch, int32_t* d_status) {
    if (!h || batch < 0 || (mode != MYSLAM_MAP_AFTER_INSERT && mode != MYSLAM_MAP_AFTER_OPTIMIZE)) return MYSLAM_ERR_INVALID;
    if (!d_kf_id || !d_n_kf || !d_mp_id || !d_n_mp || !d_obs_mp || !d_obs_kf || !d_obs_flags || !d_obs_uv || !d_obs_tag || !d_n_obs || !d_backend_status ||
        !d_map_status || !d_status || be_kf_cap < 1 || be_mp_cap != h->t.be_mp_cap || be_obs_cap != h->t.be_obs_cap)
        return MYSLAM_ERR_INVALID;
    if (mode == MYSLAM_MAP_AFTER_OPTIMIZE && !d_obs_report) return MYSLAM_ERR_INVALID;
    if (batch > h->max_batch) return MYSLAM_ERR_CAPACITY;
    if (batch == 0) return MYSLAM_OK;
    const BeTablesRead B{d_kf_id, d_kf_pose, d_n_kf, d_mp_id, d_mp_pos, d_mp_outlier, d_n_mp, d_obs_mp, d_obs_kf, d_obs_flags, d_obs_uv, d_obs_tag, d_n_obs,
                         be_kf_cap, be_mp_cap, be_obs_cap};
    const OaUpdateIn U{mode, d_backend_status, d_map_status, mode == MYSLAM_MAP_AFTER_OPTIMIZE ? d_obs_report : nullptr};
    hipLaunchKernelGGL(k_obs_update, dim3(batch), dim3(OA_NT), 0, h->stream, h->t, B, U, d_status);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_obs_archive_prior_rows_batch(myslam_obs_archive* h, const int64_t* d_feat_mp_id, const int32_t* d_n_feat, int feat_cap, const int64_t* d_mp_id,
                                        const int32_t* d_n_mp, int be_mp_cap, int batch, int64_t* d_prior_mp_id, int64_t* d_prior_kf_id, float* d_prior_uv,
                                        int32_t* d_prior_tag, uint8_t* d_prior_flags, int32_t* d_n_prior, int prior_cap, int32_t* d_status) {
    if (!h || batch < 0 || !d_feat_mp_id || !d_n_feat || !d_mp_id || !d_n_mp || !d_prior_mp_id || !d_prior_kf_id || !d_prior_uv || !d_prior_tag ||
        !d_prior_flags || !d_n_prior || !d_status || feat_cap < 1 || prior_cap < 1 || be_mp_cap != h->t.be_mp_cap)
        return MYSLAM_ERR_INVALID;
    if (batch > h->max_batch) return MYSLAM_ERR_CAPACITY;
    if (batch == 0) return MYSLAM_OK;
    const OaPriorIn I{d_feat_mp_id, d_n_feat, feat_cap, d_mp_id, d_n_mp, be_mp_cap};
    const OaPriorOut O{d_prior_mp_id, {d_prior_kf_id, d_prior_uv, d_prior_tag, d_prior_flags}, d_n_prior, prior_cap};
    hipLaunchKernelGGL(k_obs_prior_rows, dim3(batch), dim3(OA_NT), 0, h->stream, h->t, I, O, d_status);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_relink_stage_batch(myslam_obs_archive* oa, myslam_relink* h, const int32_t* d_plan_status, int batch, int32_t* d_status) {
    if (!oa || !h || !d_plan_status || !d_status || batch < 0) return MYSLAM_ERR_INVALID;
    myslam_relink_lists v;
    if (myslam_relink_view(h, &v) != MYSLAM_OK || v.point_cap != oa->t.point_cap) return MYSLAM_ERR_INVALID;
    if (batch > oa->max_batch || batch > v.max_batch) return MYSLAM_ERR_CAPACITY;
    if (batch == 0) return MYSLAM_OK;
    hipLaunchKernelGGL(k_relink_stage, dim3(batch), dim3(OA_NT), 0, oa->stream, oa->t, v, d_plan_status, d_status);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_relink_obs_update_batch(myslam_obs_archive* oa, myslam_relink* h, const int64_t* d_kf_id, const int32_t* d_n_kf, const int64_t* d_mp_id,
                                   const int32_t* d_n_mp, const int32_t* d_obs_mp, const int32_t* d_obs_kf, const uint8_t* d_obs_flags, const float* d_obs_uv,
                                   const int32_t* d_obs_tag, const int32_t* d_n_obs, int be_kf_cap, int be_mp_cap, int be_obs_cap,
                                   const int32_t* d_backend_status, const int32_t* d_map_status, int batch, int32_t* d_status) {
    if (!oa || !h || batch < 0 || !d_kf_id || !d_n_kf || !d_mp_id || !d_n_mp || !d_obs_mp || !d_obs_kf || !d_obs_flags || !d_obs_uv || !d_obs_tag || !d_n_obs ||
        !d_backend_status || !d_map_status || !d_status || be_kf_cap < 1 || be_mp_cap != oa->t.be_mp_cap || be_obs_cap != oa->t.be_obs_cap)
        return MYSLAM_ERR_INVALID;
    myslam_relink_lists v;
    if (myslam_relink_view(h, &v) != MYSLAM_OK || v.point_cap != oa->t.point_cap) return MYSLAM_ERR_INVALID;
    if (batch > oa->max_batch || batch > v.max_batch) return MYSLAM_ERR_CAPACITY;
    if (batch == 0) return MYSLAM_OK;
    const BeTablesRead B{d_kf_id, nullptr, d_n_kf, d_mp_id, nullptr, nullptr, d_n_mp, d_obs_mp, d_obs_kf, d_obs_flags, d_obs_uv, d_obs_tag, d_n_obs,
                         be_kf_cap, be_mp_cap, be_obs_cap};
    hipLaunchKernelGGL(k_relink_obs_update, dim3(batch), dim3(OA_NT), 0, oa->stream, oa->t, B, v, d_backend_status, d_map_status, d_status);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_relink_first_kf_batch(myslam_obs_archive* oa, int batch, int32_t* d_first_kf) {
    if (!oa || batch < 0 || !d_first_kf) return MYSLAM_ERR_INVALID;
    if (batch > oa->max_batch) return MYSLAM_ERR_CAPACITY;
    if (batch == 0) return MYSLAM_OK;
    hipLaunchKernelGGL(k_relink_first_kf, dim3((oa->t.point_cap + OA_NT - 1) / OA_NT, batch), dim3(OA_NT), 0, oa->stream, oa->t, oa->map.kf_id, oa->map.n_kf,
                       oa->map.kf_cap, d_first_kf);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

}  // extern "C"
