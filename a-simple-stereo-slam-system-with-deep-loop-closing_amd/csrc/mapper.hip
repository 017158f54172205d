// mapper.hip — the Backend thread's work for a bank of streams behind one handle (reference src/backend.cpp:30-37, :82-121, :126-266 with
// src/map.cpp:17-48): one enqueue maps exactly the streams that made a key-frame in the turn or the StereoInit just taken.
// The handle owns a back end, a map archive (solve attached) and an observation archive for S items, the back end's 13 tables and every array the
// stages hand to each other; the call is the units' own launches in the order of include/myslam_hip.h (MAPPER) between two launches of its own:
//   k_mapper_gate    one thread per item: takes the key-frame iff no sticky fault, turn status 0 and a key-frame id >= 0; else MYSLAM_MAPPER_IDLE.
//                    k_backend_insert and the tracker's update read this array, k_backend_flatten reads the insert's status (backend_launch.h);
//   k_mapper_status  one thread per item: the seven stage statuses -> d_status, the first negative one becomes the item's sticky fault.
// Integer code only.  No global atomics; an item's words depend neither on its slot nor on its neighbours.
#include "backend_launch.h"

namespace myslam_hip {

constexpr int MP_NT = 64, MP_STAGES = 7;

struct MapperStages { const int32_t* st[MP_STAGES]; };

__global__ __launch_bounds__(MP_NT) void k_mapper_gate(const int32_t* fault, const int32_t* report, const int64_t* new_kf_id, int S, int32_t* gate) {
    const int s = blockIdx.x * MP_NT + threadIdx.x;
    if (s >= S) return;
    gate[s] = (fault[s] == 0 && report[(size_t)s * 8] == 0 && new_kf_id[s] >= 0) ? 0 : MYSLAM_MAPPER_IDLE;
}

__global__ __launch_bounds__(MP_NT) void k_mapper_status(const int32_t* gate, int32_t* fault, MapperStages G, int S, int32_t* status) {
    const int s = blockIdx.x * MP_NT + threadIdx.x;
    if (s >= S) return;
    int32_t* const w = status + (size_t)s * MYSLAM_MAPPER_STATUS_WORDS;
    if (gate[s] != 0) {                                                     // idle: nothing of the item was touched; a faulted item says why
        const int f = fault[s];
        w[0] = f ? f : MYSLAM_MAPPER_IDLE;
        for (int k = 0; k < MP_STAGES; k++) w[1 + k] = MYSLAM_MAPPER_IDLE;
        return;
    }
    int overall = 0;
    for (int k = 0; k < MP_STAGES; k++) {
        const int v = G.st[k][s];
        w[1 + k] = v;
        if (overall == 0 && v < 0) overall = v;
    }
    w[0] = overall;
    if (overall < 0) fault[s] = overall;                                    // sticky until myslam_mapper_reset_item
}

}  // namespace myslam_hip

using namespace myslam_hip;

struct myslam_mapper {
    int S = 0, kf_cap = 0, mp_cap = 0, obs_cap = 0, feat_cap = 0, prior_cap = 0;
    hipStream_t stream = nullptr;
    myslam_backend* be = nullptr; myslam_map* map = nullptr; myslam_obs_archive* obs = nullptr;
    myslam_mapper_tables t{};
    const int64_t* culled_kf_id = nullptr; const int32_t* culled_tag = nullptr; const int32_t* n_culled = nullptr;
    BufSet mem;
    ~myslam_mapper() {
        if (obs) (void)myslam_obs_archive_destroy(obs);                      // reads the map's tables: goes first
        if (map) (void)myslam_map_destroy(map);
        if (be) (void)myslam_backend_destroy(be);
    }
};

// zero bytes of a device block, complete on return, off the legacy stream (common.h)
static int mapper_clear(void* p, size_t bytes) {
    if (bytes == 0) return MYSLAM_OK;
    const hipStream_t st = host_call_stream();
    if (!st) return MYSLAM_ERR_HIP;
    MYSLAM_HIP_CHECK(hipMemsetAsync(p, 0, bytes, st));
    MYSLAM_HIP_CHECK(hipStreamSynchronize(st));
    return MYSLAM_OK;
}

extern "C" {

int myslam_mapper_destroy(myslam_mapper* h) {
    if (!h) return MYSLAM_ERR_INVALID;
    (void)hipStreamSynchronize(h->stream);
    delete h;
    return MYSLAM_OK;
}

int myslam_mapper_create(myslam_mapper** out, int streams, int kf_cap, int mp_cap, int obs_cap, int feat_cap, int archive_kf_cap, int archive_edge_cap,
                         int archive_point_cap, int obs_row_cap, int prior_cap) {
    if (!out || streams < 1 || kf_cap < 1 || mp_cap < 1 || obs_cap < 1 || feat_cap < 1 || archive_kf_cap < 1 || archive_edge_cap < 1 ||
        archive_point_cap < 1 || obs_row_cap < 1 || prior_cap < 1)
        return MYSLAM_ERR_INVALID;
    if (feat_cap > obs_cap || prior_cap > obs_cap) return MYSLAM_ERR_CAPACITY;      // what the insert would answer at every call
    myslam_mapper* h = new myslam_mapper();
    h->S = streams; h->kf_cap = kf_cap; h->mp_cap = mp_cap; h->obs_cap = obs_cap; h->feat_cap = feat_cap; h->prior_cap = prior_cap;
    int rc;
    const double* sp = nullptr; const int32_t* ss = nullptr;
    if ((rc = myslam_backend_create(&h->be, streams, kf_cap, mp_cap, obs_cap)) ||
        (rc = myslam_map_create(&h->map, streams, archive_kf_cap, archive_edge_cap, archive_point_cap, mp_cap)) ||
        (rc = myslam_obs_archive_create(&h->obs, h->map, streams, obs_cap, obs_row_cap)) || (rc = myslam_backend_solve_view(h->be, &sp, &ss)) ||
        (rc = myslam_map_attach_solve(h->map, sp, ss)) || (rc = myslam_backend_culled_view(h->be, &h->culled_kf_id, &h->culled_tag, &h->n_culled))) {
        delete h;
        return rc;
    }
    myslam_mapper_tables& t = h->t;
    const size_t B = (size_t)streams, K = (size_t)kf_cap, M = (size_t)mp_cap, N = (size_t)obs_cap, F = (size_t)feat_cap, P = (size_t)prior_cap;
    auto own = [&](auto*& p, size_t n) {                                    // every block starts zeroed: empty tables, no fault, no stale status
        const int r = h->mem.own(p, n, MYSLAM_ERR_CAPACITY);
        return r ? r : mapper_clear(p, n * sizeof(*p));
    };
    if ((rc = own(t.kf_id, B * K)) || (rc = own(t.kf_pose, B * K * 7)) || (rc = own(t.n_kf, B)) || (rc = own(t.mp_id, B * M)) ||
        (rc = own(t.mp_pos, B * M * 3)) || (rc = own(t.mp_outlier, B * M)) || (rc = own(t.n_mp, B)) || (rc = own(t.obs_mp, B * N)) ||
        (rc = own(t.obs_kf, B * N)) || (rc = own(t.obs_flags, B * N)) || (rc = own(t.obs_uv, B * N * 2)) || (rc = own(t.obs_tag, B * N)) ||
        (rc = own(t.n_obs, B)) ||
        (rc = own(t.prior_mp_id, B * P)) || (rc = own(t.prior_kf_id, B * P)) || (rc = own(t.prior_uv, B * P * 2)) || (rc = own(t.prior_tag, B * P)) ||
        (rc = own(t.prior_flags, B * P)) || (rc = own(t.n_prior, B)) ||
        (rc = own(t.feat_row, B * F)) || (rc = own(t.mp_new_row, B * M)) || (rc = own(t.removed_kf_id, B)) || (rc = own(t.removed_kf_row, B)) ||
        (rc = own(t.dis, B * K)) ||
        (rc = own(t.obs_report, B * N)) || (rc = own(t.mp_report, B * M)) || (rc = own(t.new_outlier_mp, B * M)) || (rc = own(t.n_new_outlier_mp, B)) ||
        (rc = own(t.obs_chi2, B * N)) || (rc = own(t.rounds, B)) || (rc = own(t.n_outlier_edges, B)) || (rc = own(t.n_cleared, B)) ||
        (rc = own(t.gate, B)) || (rc = own(t.fault, B))) {
        delete h;
        return rc;
    }
    for (int k = 0; k < MP_STAGES; k++)
        if ((rc = own(t.stage_status[k], B))) { delete h; return rc; }
    t.backend = h->be; t.map = h->map; t.obs = h->obs;
    t.streams = streams; t.kf_cap = kf_cap; t.mp_cap = mp_cap; t.obs_cap = obs_cap; t.feat_cap = feat_cap; t.prior_cap = prior_cap;
    *out = h;
    return MYSLAM_OK;
}

int myslam_mapper_set_stream(myslam_mapper* h, void* hip_stream) {
    if (!h) return MYSLAM_ERR_INVALID;
    h->stream = (hipStream_t)hip_stream;
    int rc;
    if ((rc = myslam_backend_set_stream(h->be, hip_stream)) || (rc = myslam_map_set_stream(h->map, hip_stream)) ||
        (rc = myslam_obs_archive_set_stream(h->obs, hip_stream)))
        return rc;
    return MYSLAM_OK;
}

int myslam_mapper_view(const myslam_mapper* h, myslam_mapper_tables* out) {
    if (!h || !out) return MYSLAM_ERR_INVALID;
    *out = h->t;
    return MYSLAM_OK;
}

int myslam_mapper_launches_per_call(const myslam_mapper* h, int with_tracker) {
    if (!h) return MYSLAM_ERR_INVALID;
    return 2 + 1 + myslam_backend_insert_launches_per_call(h->be) + myslam_backend_launches_per_call(h->be) + 2 * myslam_map_launches_per_update(h->map) +
           2 * myslam_obs_archive_launches_per_update(h->obs) + (with_tracker ? 2 : 0);
}

int myslam_mapper_keyframe_batch(myslam_mapper* h, myslam_tracker* trk, const int64_t* d_new_kf_id, const double* d_new_kf_pose, const int64_t* d_feat_mp_id,
                                 const double* d_feat_mp_pos, const float* d_feat_uv, const int32_t* d_feat_tag, const uint8_t* d_feat_flags,
                                 const int32_t* d_n_feat, const int64_t* d_outlier_mp_id, const int32_t* d_n_outlier_mp, const float* d_right_xy,
                                 const uint8_t* d_right_ok, const int32_t* d_report, int window, double min_dis_th, double fx, double fy, double cx, double cy,
                                 double huber_delta, double chi2_th, int max_rounds, int iters_per_round, int32_t* d_status) {
    (void)d_right_xy; (void)d_right_ok;                                     // the right matches are the loop closer's and the host's, not the map's
    if (!h || !d_new_kf_id || !d_new_kf_pose || !d_feat_mp_id || !d_feat_mp_pos || !d_feat_uv || !d_feat_tag || !d_feat_flags || !d_n_feat ||
        !d_outlier_mp_id || !d_n_outlier_mp || !d_report || !d_status || window < 1 || max_rounds < 1 || iters_per_round < 1)
        return MYSLAM_ERR_INVALID;
    if (trk) {
        hipStream_t ts = nullptr;
        int tS = 0, tcap = 0;
        tracker_shape(trk, &ts, &tS, &tcap);
        if (ts != h->stream || tS != h->S || tcap != h->feat_cap) return MYSLAM_ERR_INVALID;
    }
    const myslam_mapper_tables& t = h->t;
    const int S = h->S, K = h->kf_cap, M = h->mp_cap, N = h->obs_cap, F = h->feat_cap, P = h->prior_cap, X = 2 * h->feat_cap;
    const dim3 grid((S + MP_NT - 1) / MP_NT);
    int32_t* const* st = t.stage_status;
    int rc;
    hipLaunchKernelGGL(k_mapper_gate, grid, dim3(MP_NT), 0, h->stream, t.fault, d_report, d_new_kf_id, S, t.gate);
    MYSLAM_HIP_CHECK(hipGetLastError());
    if ((rc = myslam_obs_archive_prior_rows_batch(h->obs, d_feat_mp_id, d_n_feat, F, t.mp_id, t.n_mp, M, S, t.prior_mp_id, t.prior_kf_id, t.prior_uv, t.prior_tag,
                                                  t.prior_flags, t.n_prior, P, st[0])) ||
        (rc = backend_insert_launch(h->be, t.kf_id, t.kf_pose, t.n_kf, t.mp_id, t.mp_pos, t.mp_outlier, t.n_mp, t.obs_mp, t.obs_kf, t.obs_flags, t.obs_uv, t.obs_tag,
                                    t.n_obs, d_new_kf_id, d_new_kf_pose, d_feat_mp_id, d_feat_mp_pos, d_feat_uv, d_feat_tag, d_feat_flags, d_n_feat, F,
                                    t.prior_mp_id, t.prior_kf_id, t.prior_uv, t.prior_tag, t.prior_flags, t.n_prior, P, d_outlier_mp_id, d_n_outlier_mp, X, S,
                                    window, min_dis_th, t.feat_row, t.mp_new_row, t.removed_kf_id, t.removed_kf_row, t.dis, st[1], t.gate)) ||
        (rc = myslam_map_update_batch(h->map, MYSLAM_MAP_AFTER_INSERT, t.kf_id, t.kf_pose, t.n_kf, K, t.mp_id, t.mp_pos, t.n_mp, M, t.obs_mp, t.obs_kf, t.obs_flags,
                                      t.n_obs, N, st[1], d_outlier_mp_id, d_n_outlier_mp, X, nullptr, S, st[2])) ||
        (rc = myslam_obs_archive_update_batch(h->obs, MYSLAM_MAP_AFTER_INSERT, t.kf_id, t.kf_pose, t.n_kf, t.mp_id, t.mp_pos, t.mp_outlier, t.n_mp, t.obs_mp,
                                              t.obs_kf, t.obs_flags, t.obs_uv, t.obs_tag, t.n_obs, K, M, N, st[1], st[2], nullptr, S, st[3])) ||
        // gated on the insert's status: IDLE for an idle item, an error for a refused key-frame — neither is optimised
        (rc = backend_optimize_launch(h->be, t.kf_id, t.kf_pose, t.n_kf, t.mp_id, t.mp_pos, t.mp_outlier, t.n_mp, t.obs_mp, t.obs_kf, t.obs_flags, t.obs_uv,
                                      t.obs_tag, t.n_obs, S, fx, fy, cx, cy, huber_delta, chi2_th, max_rounds, iters_per_round, t.obs_report, t.mp_report,
                                      t.new_outlier_mp, t.n_new_outlier_mp, t.obs_chi2, t.rounds, t.n_outlier_edges, st[4], st[1])) ||
        (rc = myslam_map_update_batch(h->map, MYSLAM_MAP_AFTER_OPTIMIZE, t.kf_id, t.kf_pose, t.n_kf, K, t.mp_id, t.mp_pos, t.n_mp, M, t.obs_mp, t.obs_kf,
                                      t.obs_flags, t.n_obs, N, st[4], nullptr, nullptr, 0, t.mp_report, S, st[5])) ||
        (rc = myslam_obs_archive_update_batch(h->obs, MYSLAM_MAP_AFTER_OPTIMIZE, t.kf_id, t.kf_pose, t.n_kf, t.mp_id, t.mp_pos, t.mp_outlier, t.n_mp, t.obs_mp,
                                              t.obs_kf, t.obs_flags, t.obs_uv, t.obs_tag, t.n_obs, K, M, N, st[4], st[5], t.obs_report, S, st[6])))
        return rc;
    if (trk && ((rc = myslam_tracker_clear_links_batch(trk, h->culled_kf_id, h->culled_tag, h->n_culled, N, t.n_cleared)) ||
                (rc = tracker_update_from_map_launch(trk, t.kf_id, t.kf_pose, t.n_kf, K, t.mp_id, t.mp_pos, t.mp_outlier, t.n_mp, M, t.gate))))
        return rc;
    MapperStages G;
    for (int k = 0; k < MP_STAGES; k++) G.st[k] = st[k];
    hipLaunchKernelGGL(k_mapper_status, grid, dim3(MP_NT), 0, h->stream, t.gate, t.fault, G, S, d_status);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_mapper_reset_item(myslam_mapper* h, int stream) {
    if (!h || stream < 0 || stream >= h->S) return MYSLAM_ERR_INVALID;
    if (stream_is_capturing(h->stream)) return MYSLAM_ERR_UNSUPPORTED;
    MYSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    const myslam_mapper_tables& t = h->t;
    const size_t b = (size_t)stream, K = (size_t)h->kf_cap, M = (size_t)h->mp_cap, N = (size_t)h->obs_cap;
    int rc;
    if ((rc = mapper_clear(t.kf_id + b * K, K * sizeof(int64_t))) || (rc = mapper_clear(t.kf_pose + b * K * 7, K * 7 * sizeof(double))) ||
        (rc = mapper_clear(t.n_kf + b, 4)) || (rc = mapper_clear(t.mp_id + b * M, M * sizeof(int64_t))) ||
        (rc = mapper_clear(t.mp_pos + b * M * 3, M * 3 * sizeof(double))) || (rc = mapper_clear(t.mp_outlier + b * M, M)) || (rc = mapper_clear(t.n_mp + b, 4)) ||
        (rc = mapper_clear(t.obs_mp + b * N, N * 4)) || (rc = mapper_clear(t.obs_kf + b * N, N * 4)) || (rc = mapper_clear(t.obs_flags + b * N, N)) ||
        (rc = mapper_clear(t.obs_uv + b * N * 2, N * 2 * sizeof(float))) || (rc = mapper_clear(t.obs_tag + b * N, N * 4)) || (rc = mapper_clear(t.n_obs + b, 4)) ||
        (rc = mapper_clear(t.fault + b, 4)))
        return rc;
    // an empty map, then an empty store over it (the load reads the map's ids, and clears the store's own sticky error)
    if ((rc = myslam_map_load(h->map, stream, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr,
                              nullptr, 0)) ||
        (rc = myslam_obs_archive_load(h->obs, stream, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                                      nullptr, 0)))
        return rc;
    return MYSLAM_OK;
}

}  // extern "C"
