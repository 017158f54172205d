// myslam::Mapper (host/myslam_hip.hpp) over the C ABI, compiled and run: a bank of two streams, no tracker.  Call 1: both take their first key-frame
// (12 map points each, seen where they project).  Call 2: stream 0 takes a second key-frame, stream 1 idles under MYSLAM_TRACKER_NO_TURN with a valid
// key-frame in its buffers: its status words are all MYSLAM_MAPPER_IDLE and every table byte of it stays.  Then ResetItem.  Host side uses the HIP
// runtime API only.
#include <hip/hip_runtime_api.h>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../a-simple-stereo-slam-system-with-deep-loop-closing_amd/host/myslam_hip.hpp"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)
#define EXPECT(c) do { if (!(c)) { printf("line %d: %s does not hold\n", __LINE__, #c); return 1; } } while (0)

static const int S = 2, KF = 4, MP = 32, OBS = 96, FEAT = 16, NPT = 12;
static const double FX = 718.856, FY = 718.856, CX = 607.1928, CY = 185.2157;

template <class T> static T* dev(size_t n) {
    void* p = nullptr;
    if (hipMalloc(&p, n * sizeof(T)) != hipSuccess || hipMemset(p, 0, n * sizeof(T)) != hipSuccess) return nullptr;
    return static_cast<T*>(p);
}
template <class T> static int up(T* d, const std::vector<T>& h) { return hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess ? 0 : 1; }
template <class T> static std::vector<T> down(const T* d, size_t n) {
    std::vector<T> h(n);
    (void)hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost);
    return h;
}

struct Turn {                       // one output set on the host
    std::vector<int64_t> id = std::vector<int64_t>(S, -1), fid = std::vector<int64_t>(S * FEAT, -1), xid = std::vector<int64_t>(S * 2 * FEAT, 0);
    std::vector<double> pose = std::vector<double>(S * 7, 0.0), fpos = std::vector<double>(S * FEAT * 3, 0.0);
    std::vector<float> uv = std::vector<float>(S * FEAT * 2, 0.f);
    std::vector<int32_t> tag = std::vector<int32_t>(S * FEAT, 0), nf = std::vector<int32_t>(S, 0), nx = std::vector<int32_t>(S, 0), rep = std::vector<int32_t>(S * 8, 0);
    std::vector<uint8_t> fl = std::vector<uint8_t>(S * FEAT, 0);
    // stream s: key-frame `kf` at the pure translation tx (Tcw), seeing the stream's NPT points where they project
    void keyframe(int s, int64_t kf, double tx, int status) {
        id[s] = kf; rep[s * 8] = status; nf[s] = NPT;
        double* p = &pose[s * 7];
        p[0] = p[1] = p[2] = 0; p[3] = 1; p[4] = tx; p[5] = p[6] = 0;
        for (int i = 0; i < NPT; i++) {
            const double x = -3.0 + 0.5 * i + s, y = -1.0 + 0.25 * (i % 5), z = 9.0 + 0.5 * (i % 4);
            const int f = s * FEAT + i;
            fid[f] = 100 + i; fpos[3 * f] = x; fpos[3 * f + 1] = y; fpos[3 * f + 2] = z; tag[f] = i;
            uv[2 * f] = (float)(FX * (x + tx) / z + CX); uv[2 * f + 1] = (float)(FY * y / z + CY);
        }
    }
};

int main() {
    myslam::Mapper mapper(S, KF, MP, OBS, FEAT, 8, 8, 64, 128, 16);
    hipStream_t st;
    CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    mapper.SetStream(st);
    EXPECT(mapper.launchesPerCall(false) == 11 && mapper.launchesPerCall(true) == 13 && mapper.streams() == S);
    const myslam_mapper_tables t = mapper.View();
    EXPECT(t.streams == S && t.kf_cap == KF && t.mp_cap == MP && t.obs_cap == OBS && t.feat_cap == FEAT && t.backend && t.map && t.obs);

    int64_t* d_id = dev<int64_t>(S); double* d_pose = dev<double>(S * 7); int64_t* d_fid = dev<int64_t>(S * FEAT); double* d_fpos = dev<double>(S * FEAT * 3);
    float* d_uv = dev<float>(S * FEAT * 2); int32_t* d_tag = dev<int32_t>(S * FEAT); uint8_t* d_fl = dev<uint8_t>(S * FEAT); int32_t* d_nf = dev<int32_t>(S);
    int64_t* d_xid = dev<int64_t>(S * 2 * FEAT); int32_t* d_nx = dev<int32_t>(S); int32_t* d_rep = dev<int32_t>(S * 8);
    int32_t* d_status = dev<int32_t>(S * MYSLAM_MAPPER_STATUS_WORDS);
    EXPECT(d_id && d_pose && d_fid && d_fpos && d_uv && d_tag && d_fl && d_nf && d_xid && d_nx && d_rep && d_status);
    const myslam::Mapper::TurnOutputs o{d_id, d_pose, d_fid, d_fpos, d_uv, d_tag, d_fl, d_nf, d_xid, d_nx, nullptr, nullptr, d_rep};
    auto call = [&](const Turn& h) {
        if (up(d_id, h.id) || up(d_pose, h.pose) || up(d_fid, h.fid) || up(d_fpos, h.fpos) || up(d_uv, h.uv) || up(d_tag, h.tag) || up(d_fl, h.fl) ||
            up(d_nf, h.nf) || up(d_xid, h.xid) || up(d_nx, h.nx) || up(d_rep, h.rep))
            return std::vector<int32_t>();
        mapper.KeyFrameBatch(nullptr, o, 3, FX, FY, CX, CY, d_status);
        if (hipStreamSynchronize(st) != hipSuccess) return std::vector<int32_t>();
        return mapper.Status(d_status);
    };

    Turn a;
    a.keyframe(0, 0, 0.0, 0); a.keyframe(1, 0, 0.0, 0);
    std::vector<int32_t> w = call(a);
    EXPECT(w.size() == (size_t)S * 8);
    for (int s = 0; s < S; s++)
        for (int k = 0; k < 8; k++) EXPECT(w[s * 8 + k] == (k == 5 ? MYSLAM_BACKEND_DONE : 0));
    EXPECT(down(t.n_kf, S) == std::vector<int32_t>({1, 1}) && down(t.n_mp, S) == std::vector<int32_t>({NPT, NPT}) && down(t.n_obs, S) == std::vector<int32_t>({NPT, NPT}));

    const std::vector<double> pose1 = down(t.kf_pose + (size_t)KF * 7, KF * 7), pos1 = down(t.mp_pos + (size_t)MP * 3, MP * 3);
    const std::vector<int32_t> obs1 = down(t.obs_mp + OBS, OBS);
    Turn b;
    b.keyframe(0, 1, -0.5, 0); b.keyframe(1, 1, -0.5, MYSLAM_TRACKER_NO_TURN);          // stream 1: a key-frame in the buffers, but no turn was taken
    w = call(b);
    EXPECT(w.size() == (size_t)S * 8 && w[0] == 0 && w[2] == 0 && w[5] == MYSLAM_BACKEND_DONE);
    for (int k = 0; k < 8; k++) EXPECT(w[8 + k] == MYSLAM_MAPPER_IDLE);
    EXPECT(down(t.n_kf, S) == std::vector<int32_t>({2, 1}) && down(t.n_obs, S) == std::vector<int32_t>({2 * NPT, NPT}));
    EXPECT(down(t.kf_pose + (size_t)KF * 7, KF * 7) == pose1 && down(t.mp_pos + (size_t)MP * 3, MP * 3) == pos1 && down(t.obs_mp + OBS, OBS) == obs1);
    EXPECT(down(t.gate, S) == std::vector<int32_t>({0, MYSLAM_MAPPER_IDLE}) && down(t.fault, S) == std::vector<int32_t>({0, 0}));

    mapper.ResetItem(0);
    EXPECT(down(t.n_kf, S) == std::vector<int32_t>({0, 1}) && down(t.n_mp, S) == std::vector<int32_t>({0, NPT}));
    int nk = -1, nm = -1;
    EXPECT(myslam_map_get(t.map, 0, nullptr, nullptr, &nk, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &nm, nullptr, nullptr, nullptr,
                          nullptr, nullptr, nullptr) == MYSLAM_OK && nk == 0 && nm == 0);
    bool threw = false;
    try { mapper.KeyFrameBatch(nullptr, o, 0, FX, FY, CX, CY, d_status); } catch (const std::exception&) { threw = true; }
    EXPECT(threw);
    CK(hipStreamSynchronize(st));
    printf("MAPPER TEST OK\n");
    return 0;
}
