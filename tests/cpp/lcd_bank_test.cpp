// myslam::LoopDatabaseBank (host/myslam_hip.hpp) over the C ABI, compiled and run: three streams of one bank against the literal loop of
// LoopClosing::DetectLoop (src/loopclosing.cpp:126-143) behind the gate of :62, then AddToDatabase (:651-659) for all of them.  Rows are one-hot and the
// query entries multiples of 1/8, so every score is exact in any f32 order and the comparison is equality.  Host side uses the HIP runtime API only.
#include <hip/hip_runtime_api.h>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../a-simple-stereo-slam-system-with-deep-loop-closing_amd/host/myslam_hip.hpp"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)
#define EXPECT(c) do { if (!(c)) { printf("line %d: %s does not hold\n", __LINE__, #c); return 1; } } while (0)

static const int DIM = MYSLAM_LCD_DIM;

struct Answer { uint64_t best; float mx; int cnt; int row; int status; };

static Answer detect_loop(const std::vector<uint64_t>& ids, const std::vector<float>& rows, const float* q, uint64_t cur, float thr, int minSize, bool active) {
    if (!active) return {0, 0.f, 0, -1, MYSLAM_LCDBANK_IDLE};
    if ((int)ids.size() <= minSize) return {0, 0.f, 0, -1, MYSLAM_LCDBANK_GATED};
    Answer a{0, 0.f, 0, -1, MYSLAM_LCDBANK_SCANNED};
    for (size_t r = 0; r < ids.size(); r++) {
        if (cur - ids[r] < 20) break;
        float s = 0.f;
        for (int k = 0; k < DIM; k++) s += rows[r * DIM + k] * q[k];
        if (s > a.mx) { a.mx = s; a.best = ids[r]; a.row = (int)r; }
        if (s > thr) a.cnt++;
    }
    return a;
}

int main() {
    const int S = 3, R = 2 * myslam::LoopDatabaseBank::rowTile() + 6, minSize = 3;
    const float thr = 0.92f;
    EXPECT(myslam::LoopDatabaseBank::launchesPerQuery() <= 3 && myslam::LoopDatabaseBank::rowTile() > 0);
    myslam::LoopDatabaseBank bank(S, R, thr, minSize);
    hipStream_t st;
    CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    bank.SetStream(st);

    // stream 0: R - 1 rows, ids 0, 2, 4, ...; stream 1: two rows (gated); stream 2: idle with rows of its own
    std::vector<std::vector<uint64_t>> ids(S);
    std::vector<std::vector<float>> rows(S);
    const int n0[S] = {R - 1, 2, 40};
    for (int s = 0; s < S; s++) {
        ids[s].resize(n0[s]); rows[s].assign((size_t)n0[s] * DIM, 0.f);
        for (int r = 0; r < n0[s]; r++) { ids[s][r] = 2 * (uint64_t)r + s; rows[s][(size_t)r * DIM + (r * 37 + 5 + s) % DIM] = 1.f; }
        bank.Load(s, ids[s], rows[s]);
    }
    std::vector<float> q((size_t)S * DIM, 0.f);
    for (int s = 0; s < S; s++)
        for (int r = 0; r < R; r++) q[(size_t)s * DIM + (r * 37 + 5 + s) % DIM] = (float)((3 * r + s) % 11) / 8.f;
    q[(size_t)0 * DIM + (50 * 37 + 5) % DIM] = 4.f;        // stream 0's best row, 50, lies inside the window of cur = 2 * 50 + 7: the scan ends at 44
    q[(size_t)0 * DIM + (17 * 37 + 5) % DIM] = 2.f;
    const uint64_t cur[S] = {2 * 50 + 7, 1000, 1000};
    const int32_t active[S] = {1, 1, 0};

    float* d_q; uint64_t *d_cur, *d_best; int32_t *d_active, *d_cnt, *d_row, *d_status; float* d_mx;
    CK(hipMalloc(&d_q, q.size() * 4)); CK(hipMalloc(&d_cur, 8 * S)); CK(hipMalloc(&d_best, 8 * S)); CK(hipMalloc(&d_active, 4 * S));
    CK(hipMalloc(&d_cnt, 4 * S)); CK(hipMalloc(&d_row, 4 * S)); CK(hipMalloc(&d_status, 4 * S)); CK(hipMalloc(&d_mx, 4 * S));
    CK(hipMemcpy(d_q, q.data(), q.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(d_cur, cur, 8 * S, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_active, active, 4 * S, hipMemcpyHostToDevice));
    CK(hipMemset(d_best, 0xAB, 8 * S)); CK(hipMemset(d_mx, 0xAB, 4 * S)); CK(hipMemset(d_cnt, 0xAB, 4 * S)); CK(hipMemset(d_row, 0xAB, 4 * S));
    CK(hipMemset(d_status, 0xAB, 4 * S));
    CK(hipDeviceSynchronize());

    bank.QueryBatch(d_q, d_cur, d_active, d_best, d_mx, d_cnt, d_row, d_status);
    CK(hipStreamSynchronize(st));
    uint64_t best[S]; float mx[S]; int32_t cnt[S], row[S], status[S];
    CK(hipMemcpy(best, d_best, 8 * S, hipMemcpyDeviceToHost)); CK(hipMemcpy(mx, d_mx, 4 * S, hipMemcpyDeviceToHost));
    CK(hipMemcpy(cnt, d_cnt, 4 * S, hipMemcpyDeviceToHost)); CK(hipMemcpy(row, d_row, 4 * S, hipMemcpyDeviceToHost));
    CK(hipMemcpy(status, d_status, 4 * S, hipMemcpyDeviceToHost));
    for (int s = 0; s < S; s++) {
        const Answer a = detect_loop(ids[s], rows[s], &q[(size_t)s * DIM], cur[s], thr, minSize, active[s] != 0);
        if (best[s] != a.best || memcmp(&mx[s], &a.mx, 4) != 0 || cnt[s] != a.cnt || row[s] != a.row || status[s] != a.status) {
            printf("stream %d: got (%llu, %g, %d, %d, %d), expected (%llu, %g, %d, %d, %d)\n", s, (unsigned long long)best[s], mx[s], cnt[s], row[s], status[s],
                   (unsigned long long)a.best, a.mx, a.cnt, a.row, a.status);
            return 1;
        }
    }
    EXPECT(status[0] == MYSLAM_LCDBANK_SCANNED && best[0] == 2 * 17 && mx[0] == 2.f && row[0] == 17 && cnt[0] > 0);
    EXPECT(status[1] == MYSLAM_LCDBANK_GATED && status[2] == MYSLAM_LCDBANK_IDLE);

    // AddToDatabase: stream 0 takes its last row, a second one does not fit; stream 1 refuses an id it holds; stream 2 is not selected
    const uint64_t newId[S] = {1000, 3, 5000};
    const int32_t add[S] = {1, 1, 0};
    uint64_t* d_id; int32_t* d_add;
    CK(hipMalloc(&d_id, 8 * S)); CK(hipMalloc(&d_add, 4 * S));
    CK(hipMemcpy(d_id, newId, 8 * S, hipMemcpyHostToDevice)); CK(hipMemcpy(d_add, add, 4 * S, hipMemcpyHostToDevice));
    bank.AppendBatch(d_q, d_id, d_add, d_status);
    CK(hipStreamSynchronize(st));
    CK(hipMemcpy(status, d_status, 4 * S, hipMemcpyDeviceToHost));
    EXPECT(status[0] == MYSLAM_LCDBANK_ADDED && status[1] == MYSLAM_ERR_INVALID && status[2] == MYSLAM_LCDBANK_IDLE);
    const uint64_t nextId[S] = {1001, 4, 5000};
    CK(hipMemcpy(d_id, nextId, 8 * S, hipMemcpyHostToDevice));
    bank.AppendBatch(d_q, d_id, nullptr, d_status);
    CK(hipStreamSynchronize(st));
    CK(hipMemcpy(status, d_status, 4 * S, hipMemcpyDeviceToHost));
    EXPECT(status[0] == MYSLAM_ERR_CAPACITY && status[1] == MYSLAM_LCDBANK_ADDED && status[2] == MYSLAM_LCDBANK_ADDED);
    const std::vector<int32_t> sizes = bank.Sizes();
    EXPECT(sizes[0] == R && sizes[1] == 3 && sizes[2] == 41);
    std::vector<uint64_t> gi; std::vector<float> gr;
    bank.Get(0, gi, gr);
    EXPECT((int)gi.size() == R && gi[R - 1] == 1000 && gi[R - 2] == ids[0][R - 2]);
    EXPECT(memcmp(&gr[(size_t)(R - 1) * DIM], &q[0], DIM * 4) == 0 && memcmp(gr.data(), rows[0].data(), rows[0].size() * 4) == 0);
    bank.Get(1, gi, gr);
    EXPECT(gi.size() == 3 && gi[2] == 4 && memcmp(&gr[(size_t)2 * DIM], &q[(size_t)1 * DIM], DIM * 4) == 0);

    // a stream that starts again
    const int32_t clr[S] = {0, 0, 1};
    CK(hipMemcpy(d_add, clr, 4 * S, hipMemcpyHostToDevice));
    bank.ClearBatch(d_add);
    CK(hipStreamSynchronize(st));
    const std::vector<int32_t> after = bank.Sizes();
    EXPECT(after[0] == R && after[1] == 3 && after[2] == 0);
    bool threw = false;
    try { bank.Load(1, {5, 5}, std::vector<float>(2 * DIM, 0.f)); } catch (const std::runtime_error&) { threw = true; }
    EXPECT(threw && bank.Sizes()[1] == 3);
    printf("LCD BANK TEST OK\n");
    return 0;
}
