// relink.hip — the PLAN of LoopClosing::LoopLocalFusion's re-linking (reference src/loopclosing.cpp:509-532) for a batch of corrected loops, on
// the device: which map points of the current key-frame are merged into which points of the loop key-frame, which features adopt a loop point,
// where every archive slot's features end, and what the current key-frame's feature table looks like afterwards.
//   k_relink_plan  one workgroup per item.  The block validates every pair and slot first (nothing is written before that), clears the item's
//                  `target` row, then ONE lane walks the surviving pairs serially in their order, as the reference's loop does: a later pair sees
//                  what an earlier pair merged or adopted, so the walk is a chain of dependent decisions (at most out_cap <= 4096 of them).  The
//                  block then rewrites the feature table from `target` and compacts the changed features into the link list (a block scan).
// The walk writes the handle's own arrays and the current table only; archive states are myslam_map_relink_batch's (map_archive.hip).
// No global atomics; an item's bytes depend neither on its slot nor on its neighbours.  Integer code and copies.
// See include/myslam_hip.h, RE-LINK, for the contract.
#include <vector>

#include "dev_mem.h"
#include "dev_tables.h"

namespace myslam_hip {

constexpr int RL_NT = 256;
constexpr int RL_NW = RL_NT / WAVE;
constexpr int RL_MAX_OUT = 4096, RL_MAX_FEAT = 65536;   // myslam_loop_match_batch's limits
constexpr int RL_REPORT = MYSLAM_RELINK_REPORT_INTS;

struct RlTables {
    int32_t* merge; int32_t* n_merge;   // max_batch x out_cap x 2 (from slot, to slot), in walk order
    int32_t* adopt; int32_t* n_adopt;   // max_batch x out_cap x 2 (feature, slot), in walk order
    int32_t* target;                    // max_batch x point_cap: the slot a point's features end on, -1 = untouched
    int64_t* link_kf; int32_t* link_tag; int32_t* link_slot; int32_t* n_link;       // max_batch x feat_cap: the current key-frame's changed features
    int32_t* report;                    // max_batch x RL_REPORT
    // the moved rows (myslam_relink_stage_batch, obs_archive.hip, fills them): max_batch x stage_cap, per merge max_batch x out_cap
    int64_t* row_kf; float* row_uv; int32_t* row_tag; uint8_t* row_flags; int64_t* row_root_id; int32_t* row_slot; int32_t* row_place; int32_t* n_rows;
    int64_t* mg_from_id; int64_t* mg_root_id; int32_t* mg_rows; int32_t* mg_place; int32_t* n_mg;
    int32_t* table_mp; int32_t* table_rows; int32_t* work_size;
    const uint8_t* map_state; const int32_t* map_n_mp;  // the map archive's, not owned
    int point_cap, out_cap, feat_cap, stage_cap;
};

struct RlPlanIn {
    const int32_t* pairs; const int32_t* counts; const uint8_t* outlier; const int32_t* correct_status;
    int32_t* cur_lm; const int32_t* loop_lm; const int64_t* cur_kf_id;
};

__global__ __launch_bounds__(RL_NT) void k_relink_plan(RlTables R, RlPlanIn I, int32_t* status) {
    __shared__ int s_w[RL_NW];
    __shared__ int s_bad;
    __shared__ unsigned s_adopted[RL_MAX_FEAT / 32];                        // one bit per feature of the current key-frame: adopted in this walk
    const int b = blockIdx.x, t = threadIdx.x;
    const int aM = R.map_n_mp[b];
    int32_t* const target = R.target + (size_t)b * R.point_cap;
    int32_t* const rep = R.report + (size_t)b * RL_REPORT;
    // the handle's outputs of an item that does not run: empty lists, an untouched target row
    const auto no_plan = [&](int code) {
        for (int s = t; s < clamped_count(aM, R.point_cap); s += RL_NT) target[s] = -1;
        if (t < RL_REPORT) rep[t] = 0;
        if (t == 0) { R.n_merge[b] = 0; R.n_adopt[b] = 0; R.n_link[b] = 0; status[b] = code; }
    };
    const int cs = I.correct_status[b];
    if (cs != MYSLAM_LOOP_CORRECT_DONE && cs != MYSLAM_LOOP_CORRECT_FUSED_ONLY) {       // uniform: the reference returns before LoopLocalFusion
        no_plan(MYSLAM_RELINK_SKIPPED);
        return;
    }
    const int cnt = I.counts[b];
    const int64_t kf_id = I.cur_kf_id[b];
    if (aM < 0 || aM > R.point_cap || cnt < 0 || cnt > R.out_cap || kf_id < 0) {        // uniform
        no_plan(MYSLAM_ERR_INVALID);
        return;
    }
    const int32_t* const pairs = I.pairs + (size_t)b * R.out_cap * 2;
    const uint8_t* const outlier = I.outlier + (size_t)b * R.out_cap;
    const uint8_t* const state = R.map_state + (size_t)b * R.point_cap;
    int32_t* const cur = I.cur_lm + (size_t)b * R.feat_cap;
    const int32_t* const loop = I.loop_lm + (size_t)b * R.feat_cap;
    int32_t* const merge = R.merge + (size_t)b * R.out_cap * 2;
    int32_t* const adopt = R.adopt + (size_t)b * R.out_cap * 2;

    // ---- decide: every feature id and every slot the walk will read is in range ----
    if (t == 0) s_bad = 0;
    for (int w = t; w < RL_MAX_FEAT / 32; w += RL_NT) s_adopted[w] = 0;
    __syncthreads();
    bool bad = false;
    for (int i = t; i < cnt; i += RL_NT) {
        if (outlier[i]) continue;
        const int cf = pairs[2 * i], lf = pairs[2 * i + 1];
        if (cf < 0 || cf >= R.feat_cap || lf < 0 || lf >= R.feat_cap) { bad = true; continue; }
        const int e = cur[cf], l = loop[lf];
        bad |= e < -1 || e >= aM || l < -1 || l >= aM;
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (s_bad) {                                                            // uniform; every byte of the current table kept
        no_plan(MYSLAM_ERR_INVALID);
        return;
    }

    // ---- from here on the item is written ----
    for (int s = t; s < aM; s += RL_NT) target[s] = -1;
    __syncthreads();
    if (t == 0) {
        // during the walk target[s] is the point s was merged into (s itself for a point that only received); root() follows it to a point that stands
        const auto root = [&](int s) { while (target[s] >= 0 && target[s] != s) s = target[s]; return s; };
        const auto is_adopted = [&](int f) { return (s_adopted[f >> 5] >> (f & 31)) & 1u; };
        int nm = 0, na = 0, walked = 0, same = 0, dead = 0;
        for (int i = 0; i < cnt; i++) {
            if (outlier[i]) continue;
            walked++;
            const int cf = pairs[2 * i], lf = pairs[2 * i + 1];
            int l = loop[lf];
            if (l < 0 || state[l] == 2) { dead += l >= 0; continue; }       // loop_mp.lock() == nullptr (:512-514)
            l = root(l);                                                    // the loop feature is an observation of its point: it moved with it
            const int e = cur[cf];
            int c = -1;
            if (e >= 0 && state[e] != 2) {
                // an adopted feature is no observation of the point it took (:528-530 only sets the pointer): it does not follow a later merge of
                // that point, its pointer dies with it
                if (is_adopted(cf)) c = (target[e] >= 0 && target[e] != e) ? -1 : e;
                else c = root(e);
            }
            if (c < 0) {                                                    // adopt (:528-530)
                cur[cf] = l;
                s_adopted[cf >> 5] |= 1u << (cf & 31);
                adopt[2 * na] = cf; adopt[2 * na + 1] = l; na++;
                if (target[l] < 0) target[l] = l;
            } else if (c == l) {
                same++;                                                     // the declared deviation: a point is not merged into itself
            } else {                                                        // merge (:516-526)
                merge[2 * nm] = c; merge[2 * nm + 1] = l; nm++;
                target[c] = l;
                if (target[l] < 0) target[l] = l;
            }
        }
        // a point merged at i ends where its target ends; targets that were merged later have been finished already
        for (int i = nm - 1; i >= 0; i--) target[merge[2 * i]] = target[merge[2 * i + 1]];
        R.n_merge[b] = nm; R.n_adopt[b] = na;
        rep[0] = walked; rep[1] = nm; rep[2] = na; rep[3] = same; rep[4] = dead;
    }
    __syncthreads();

    // ---- the current key-frame's table: an observation follows its point; the changed features, in feature order, are the link list ----
    int64_t* const link_kf = R.link_kf + (size_t)b * R.feat_cap;
    int32_t* const link_tag = R.link_tag + (size_t)b * R.feat_cap;
    int32_t* const link_slot = R.link_slot + (size_t)b * R.feat_cap;
    int n_link = 0;
    for (int base = 0; base < R.feat_cap; base += RL_NT) {                  // uniform
        const int f = base + t;
        bool changed = false;
        int e = -1;
        if (f < R.feat_cap) {
            e = cur[f];
            const bool moved = e >= 0 && e < aM && target[e] >= 0 && target[e] != e;
            if ((s_adopted[f >> 5] >> (f & 31)) & 1u) {
                changed = true;
                if (moved) { e = -1; cur[f] = -1; }                         // the point it adopted was merged away afterwards: lock() is null
            } else if (moved) {
                changed = true;
                e = target[e]; cur[f] = e;
            }
        }
        int tot;
        const int pos = n_link + block_rank<RL_NW>(changed, s_w, tot);
        if (changed) { link_kf[pos] = kf_id; link_tag[pos] = f; link_slot[pos] = e; }
        n_link += tot;
    }
    if (t == 0) { R.n_link[b] = n_link; rep[5] = n_link; status[b] = MYSLAM_RELINK_DONE; }
}

}  // namespace myslam_hip

using namespace myslam_hip;

struct myslam_relink {
    int max_batch = 0;
    hipStream_t stream = nullptr;
    RlTables t{};
    BufSet mem;                         // owns every block that `t` names, the map's excepted
};

extern "C" {

int myslam_relink_create(myslam_relink** out, const myslam_map* map, int max_batch, int out_cap, int feat_cap, int stage_cap) {
    if (!out || !map || max_batch < 1 || out_cap < 1 || feat_cap < 1 || stage_cap < 1) return MYSLAM_ERR_INVALID;
    myslam_map_tables mv;
    if (myslam_map_view(map, &mv) != MYSLAM_OK) return MYSLAM_ERR_INVALID;
    if (max_batch > mv.max_batch) return MYSLAM_ERR_INVALID;
    if (out_cap > RL_MAX_OUT || feat_cap > RL_MAX_FEAT || stage_cap > (1 << 26)) return MYSLAM_ERR_CAPACITY;
    if (need_device()) return MYSLAM_ERR_HIP;
    myslam_relink* h = new myslam_relink();
    h->max_batch = max_batch;
    RlTables& t = h->t;
    t.point_cap = mv.point_cap; t.out_cap = out_cap; t.feat_cap = feat_cap; t.stage_cap = stage_cap;
    t.map_state = mv.mp_state; t.map_n_mp = mv.n_mp;
    const size_t B = (size_t)max_batch, P = (size_t)mv.point_cap, O = (size_t)out_cap, F = (size_t)feat_cap, S = (size_t)stage_cap;
    auto own = [&](auto*& p, size_t n) { return h->mem.own(p, n, MYSLAM_ERR_CAPACITY); };
    int rc;
    if ((rc = own(t.merge, B * O * 2)) || (rc = own(t.n_merge, B)) || (rc = own(t.adopt, B * O * 2)) || (rc = own(t.n_adopt, B)) || (rc = own(t.target, B * P)) ||
        (rc = own(t.link_kf, B * F)) || (rc = own(t.link_tag, B * F)) || (rc = own(t.link_slot, B * F)) || (rc = own(t.n_link, B)) ||
        (rc = own(t.report, B * RL_REPORT)) || (rc = own(t.row_kf, B * S)) || (rc = own(t.row_uv, B * S * 2)) || (rc = own(t.row_tag, B * S)) ||
        (rc = own(t.row_flags, B * S)) || (rc = own(t.row_root_id, B * S)) || (rc = own(t.row_slot, B * S)) || (rc = own(t.row_place, B * S)) ||
        (rc = own(t.n_rows, B)) || (rc = own(t.mg_from_id, B * O)) || (rc = own(t.mg_root_id, B * O)) || (rc = own(t.mg_rows, B * O)) ||
        (rc = own(t.mg_place, B * O)) || (rc = own(t.n_mg, B)) || (rc = own(t.table_mp, B)) || (rc = own(t.table_rows, B)) || (rc = own(t.work_size, B * P))) {
        delete h;
        return rc;
    }
    const std::vector<int32_t> zeros(B * RL_REPORT, 0);                     // before the first plan every list is empty
    for (int32_t* p : {t.n_merge, t.n_adopt, t.n_link, t.n_rows, t.n_mg, t.table_mp, t.table_rows})
        if ((rc = upload_table(p, zeros.data(), B * sizeof(int32_t)))) { delete h; return rc; }
    if ((rc = upload_table(t.report, zeros.data(), B * RL_REPORT * sizeof(int32_t)))) { delete h; return rc; }
    *out = h;
    return MYSLAM_OK;
}

int myslam_relink_destroy(myslam_relink* h) {
    if (!h) return MYSLAM_ERR_INVALID;
    (void)hipStreamSynchronize(h->stream);
    delete h;
    return MYSLAM_OK;
}

int myslam_relink_set_stream(myslam_relink* h, void* hip_stream) {
    if (!h) return MYSLAM_ERR_INVALID;
    h->stream = (hipStream_t)hip_stream;
    return MYSLAM_OK;
}

int myslam_relink_view(const myslam_relink* h, myslam_relink_lists* out) {
    if (!h || !out) return MYSLAM_ERR_INVALID;
    const RlTables& t = h->t;
    *out = myslam_relink_lists{t.merge, t.n_merge, t.adopt, t.n_adopt, t.target, t.link_kf, t.link_tag, t.link_slot, t.n_link, t.report,
                               t.row_kf, t.row_uv, t.row_tag, t.row_flags, t.row_root_id, t.row_slot, t.row_place, t.n_rows,
                               t.mg_from_id, t.mg_root_id, t.mg_rows, t.mg_place, t.n_mg, t.table_mp, t.table_rows, t.work_size,
                               h->max_batch, t.out_cap, t.feat_cap, t.point_cap, t.stage_cap};
    return MYSLAM_OK;
}

int myslam_relink_launches_per_plan(const myslam_relink* h) { return h ? 1 : MYSLAM_ERR_INVALID; }

int myslam_loop_relink_plan_batch(myslam_relink* h, const int32_t* d_valid_pairs, const int32_t* d_counts, const uint8_t* d_outlier,
                                  const int32_t* d_correct_status, int32_t* d_cur_feat_landmark, const int32_t* d_loop_feat_landmark,
                                  const int64_t* d_cur_kf_id, int batch, int32_t* d_status) {
    if (!h || batch < 0 || !d_valid_pairs || !d_counts || !d_outlier || !d_correct_status || !d_cur_feat_landmark || !d_loop_feat_landmark || !d_cur_kf_id ||
        !d_status)
        return MYSLAM_ERR_INVALID;
    if (batch > h->max_batch) return MYSLAM_ERR_CAPACITY;
    if (batch == 0) return MYSLAM_OK;
    const RlPlanIn I{d_valid_pairs, d_counts, d_outlier, d_correct_status, d_cur_feat_landmark, d_loop_feat_landmark, d_cur_kf_id};
    hipLaunchKernelGGL(k_relink_plan, dim3(batch), dim3(RL_NT), 0, h->stream, h->t, I, d_status);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

}  // extern "C"
