// match_tri.hip — 256-bit Hamming brute-force matcher and stereo triangulation for gfx950.
//
// Hamming: replaces cv::BFMatcher(NORM_HAMMING)::match (reference src/loopclosing.cpp:33,172): one
// best train row per query row, ties -> lowest train index: a +-1 product on the FP4 matrix cores.
//
// Triangulation: replaces triangulation() (reference include/myslam/algorithm.h:16-33) for the
// stereo rig (src/system.cpp:108-116,141-145): DLT 4x4, smallest right singular vector by one-sided
// Jacobi in f64, accept iff sigma3/sigma2 < 1e-2 and z > 0 (src/frontend.cpp:400,471).
#include <algorithm>
#include <utility>
#include <vector>

#include "dev_tables.h"
#include "tri_solve.h"

namespace myslam_hip {

// ------------------------------------------------------------------------------------------------
// Hamming brute force on the matrix cores.  With every descriptor bit b encoded as s = 1 - 2b,
//     sum_k s_q[k] s_t[k] = 256 - 2 * hamming(q, t),
// so the 2000 x 2000 distance matrix of a stereo pair is a [nt x 256] x [256 x nq] product.
//   * block = 4 waves x HQ_TILES query tiles of 32; the query operand (B) is expanded ONCE into registers and reused against
//     every train chunk
//   * train descriptors stay bit-packed in HBM; each chunk of 32 is expanded into LDS by the whole block through a 256-entry
//     byte table, double buffered, one barrier per chunk
//   * A (train) and B (query) use the same (lane, byte) -> k map, so the hardware's k order inside an operand is irrelevant
//   * the 32x32 result puts ONE query column in every lane (16 train rows in its registers): the running best is a single
//     register per tile, key = (dot + 256) << 20 | (0xFFFFF - train index), maximised with v_max3 — highest dot = smallest
//     distance, ties to the lowest train index (BFMatcher keeps the first minimum); the two half-waves merge at the end.
// (History: xor / popcount on the VALU ran at its issue peak, 1.00 ms per 512 pairs; int8 MFMA 0.40 ms; this FP4 form 0.23 ms.)
constexpr int HQ_TILES = 4;                       // query tiles of 32 per wave -> 512 queries per block
constexpr int HQ_BLOCK = 4 * HQ_TILES * 32;
constexpr int HQ_NARROW_BELOW = 16;               // fewer pairs than this per call: one query tile per wave (k_hamming_fp4<1, HQ_SPLIT>)
constexpr int HQ_SPLIT = 4;                       // ... and this many wave groups per block, each on every HQ_SPLIT-th train chunk

// The product runs on the FP4 path of the matrix cores (v_mfma_scale_f32_32x32x64_f8f6f4, K = 64 per instruction, twice the int8
// rate): E2M1 represents +-1 exactly (0x2 / 0xA), the factor 32 of the query operand is its E8M0 block scale (2^5), sums of at most
// 256 terms of +-32 plus the (31 - row) start value are exact in f32.  One descriptor dword (32 bits) expands to the 16 operand bytes
// of a lane; 4 MFMAs per 32 x 32 tile instead of 8, 16 query registers per tile instead of 32, 4 KB of LDS per train chunk.
// the triangulation of ONE left key-point against its match (defined below, behind tri_solve): also the tail of the one-pair matcher
struct TriTail {
    const myslam_keypoint* kl; const myslam_keypoint* kr;        // kl == nullptr: no tail
    double fx, fy, cx, cy, baseline; double* xyz; uint8_t* ok;
};
__device__ __forceinline__ void tri_point(const TriTail& tt, int p, int cap, int i, int j);

typedef int hq_v8i __attribute__((ext_vector_type(8)));
typedef float hq_v16f __attribute__((ext_vector_type(16)));
constexpr int HF_ROWB = 144;                      // LDS bytes per expanded train row (128 + 16)

// TILES = query tiles of 32 per wave: 4 (512 queries per block) for batches; 1 (128 per block) for a handful of pairs — the block's loop
// over the train chunks is a chain of barrier-separated steps, and with one tile per wave a step is a quarter as long while four times
// as many blocks run side by side (one pair of 2 000 x 2 000: 50 -> ~25 us).  Same bits either way (integer arg-min, ties by row).
// SPLIT = groups of 4 waves per block, each taking every SPLIT-th train chunk for the block's queries (round 5, one-pair calls: 16 blocks
// walk 63 chunks as a chain of barrier-separated steps — 32 us on 16 of 256 CUs; with 4 groups the chain is 16 steps and the groups' keys
// merge through LDS at the end.  The key is an integer maximum: the same bits whatever the split).
// TRI: the block triangulates its 128 queries against the matches it has just found (myslam_hamming_match_triangulate_batch: a recorded
// one-pair step is bound by the number of its launches, and the triangulation of a query needs nothing but that query's match).
template <int TILES, int SPLIT = 1, bool TRI = false>
__global__ __launch_bounds__(256 * SPLIT) void k_hamming_fp4(const uint8_t* __restrict__ q, const int32_t* __restrict__ nqv,
                                                     const uint8_t* __restrict__ tr, const int32_t* __restrict__ ntv,
                                                     int cap, int nq_single, int nt_single,
                                                     int32_t* __restrict__ out_idx, int32_t* __restrict__ out_dist, TriTail tt) {
    __shared__ __attribute__((aligned(16))) uint8_t s_exp[SPLIT][2][32 * HF_ROWB];
    __shared__ uint32_t s_key[SPLIT > 1 ? SPLIT : 1][SPLIT > 1 ? 128 * TILES : 1];
    __shared__ int32_t s_match[TRI ? 128 * TILES : 1];
    __shared__ uint32_t s_lut[256];                // byte -> 8 FP4 codes (bit i -> nibble i): bit 1 -> -1.0 (0xA), bit 0 -> +1.0 (0x2)
    const int p = blockIdx.y;
    const int nq = nqv ? min(nqv[p], cap) : nq_single;
    const int nt = ntv ? min(ntv[p], cap) : nt_single;
    constexpr int QBLOCK = 4 * TILES * 32;
    const int q0 = blockIdx.x * QBLOCK;
    if (q0 >= nq) return;
    const int grp = SPLIT > 1 ? (int)threadIdx.x >> 8 : 0;      // train split of this wave group
    const int tid = threadIdx.x & 255, lane = tid & 63, wv = tid >> 6;
    if (grp == 0) {
        uint32_t v = 0;
        for (int i = 0; i < 8; i++) v |= (((tid >> i) & 1) ? 0xAu : 0x2u) << (4 * i);
        s_lut[tid] = v;
    }
    __syncthreads();
    const uint32_t* Q = reinterpret_cast<const uint32_t*>(q + (size_t)p * cap * 32);
    const uint32_t* T = reinterpret_cast<const uint32_t*>(tr + (size_t)p * cap * 32);
    auto expand32 = [&](uint32_t w) { return make_uint4(s_lut[w & 0xff], s_lut[(w >> 8) & 0xff], s_lut[(w >> 16) & 0xff], s_lut[w >> 24]); };
    // query operands: k block m of tile t takes descriptor dword 2 m + (lane >> 5) of query qb + 32 t + (lane & 31)
    const int qb = q0 + wv * (TILES * 32);
    hq_v8i B[TILES][4];
#pragma unroll
    for (int t = 0; t < TILES; t++) {
        const int qi = qb + 32 * t + (lane & 31);
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const uint4 e = expand32((qi < nq) ? Q[(size_t)qi * 8 + 2 * m + (lane >> 5)] : 0u);
            B[t][m] = hq_v8i{(int)e.x, (int)e.y, (int)e.z, (int)e.w, 0, 0, 0, 0};
        }
    }
    const int rbase = 4 * (lane >> 5);                       // row of accumulator register r: (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    hq_v16f cinit, ctail;
    const int last0 = ((nt - 1) >> 5) << 5;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = rbase + (r & 3) + 8 * (r >> 2);
        cinit[r] = (float)(31 - row);
        ctail[r] = (last0 + row < nt) ? (float)(31 - row) : -16777216.f;
    }
    int bestv[TILES], bestor[TILES], bestc[TILES];
#pragma unroll
    for (int t = 0; t < TILES; t++) { bestv[t] = -(1 << 30); bestor[t] = -(1 << 30); bestc[t] = 0; }
    const int er = tid >> 3, ed = tid & 7;                   // expansion job: dword ed of chunk row er
    auto expand = [&](int buf, uint32_t w) { *reinterpret_cast<uint4*>(&s_exp[grp][buf][er * HF_ROWB + ed * 16]) = expand32(w); };
    const int nchunk = (nt + 31) >> 5;
    const int nstep = (nchunk + SPLIT - 1) / SPLIT;          // block-uniform: every group meets every barrier
    uint32_t wnext = (32 * grp + er < nt) ? T[(size_t)(32 * grp + er) * 8 + ed] : 0u;
    if (grp < nchunk) expand(0, wnext);
    for (int i = 0; i < nstep; i++) {
        const int c = i * SPLIT + grp;                       // this group's chunk of the step (may lie past the end)
        const int t0 = c << 5;
        if (c + SPLIT < nchunk) { const int row = t0 + 32 * SPLIT + er; wnext = (row < nt) ? T[(size_t)row * 8 + ed] : 0u; }
        __syncthreads();
        if (c + SPLIT < nchunk) expand((i + 1) & 1, wnext);
        if (c >= nchunk) continue;
        const uint8_t* sb = &s_exp[grp][i & 1][(lane & 31) * HF_ROWB + (lane >> 5) * 16];
        hq_v8i A[4];
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const uint4 e = *reinterpret_cast<const uint4*>(sb + m * 32);
            A[m] = hq_v8i{(int)e.x, (int)e.y, (int)e.z, (int)e.w, 0, 0, 0, 0};
        }
        const hq_v16f c0 = (c + 1 == nchunk) ? ctail : cinit;
#pragma unroll
        for (int t = 0; t < TILES; t++) {
            // A: FP4, scale 2^0 (E8M0 127); B: FP4, scale 2^5 (132)
            hq_v16f acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A[0], B[t][0], c0, 4, 4, 0, 127, 0, 132);
#pragma unroll
            for (int m = 1; m < 4; m++) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A[m], B[t][m], acc, 4, 4, 0, 127, 0, 132);
            float vf = fmaxf(fmaxf(acc[0], acc[1]), acc[2]);
#pragma unroll
            for (int r = 3; r < 15; r += 2) vf = fmaxf(fmaxf(vf, acc[r]), acc[r + 1]);
            vf = fmaxf(vf, acc[15]);
            const int v = (int)vf;
            const bool better = v > bestor[t];
            bestv[t] = better ? v : bestv[t];
            bestor[t] = better ? (v | 31) : bestor[t];
            bestc[t] = better ? c : bestc[t];
        }
    }
#pragma unroll
    for (int t = 0; t < TILES; t++) {
        const int dot = bestv[t] >> 5, row = 31 - (bestv[t] & 31);
        const uint32_t key = bestv[t] < -(1 << 20) ? 0u
                                                     : ((uint32_t)(dot + 256) << 20) | (0xfffffu - (uint32_t)(bestc[t] * 32 + row));
        uint32_t b = max(key, (uint32_t)__shfl_xor((int)key, 32, 64));
        if (SPLIT > 1) {                                     // the groups' keys of this query: maximum through LDS, written by group 0
            if (lane < 32) s_key[grp][(wv * TILES + t) * 32 + lane] = b;
            __syncthreads();
            if (grp == 0 && lane < 32)
#pragma unroll
                for (int g2 = 1; g2 < SPLIT; g2++) b = max(b, s_key[g2][(wv * TILES + t) * 32 + lane]);
        }
        const int qi = qb + 32 * t + lane;
        if (grp == 0 && lane < 32 && qi < nq) {
            const bool any = nt > 0;
            out_idx[(size_t)p * cap + qi] = any ? (int32_t)(0xfffffu - (b & 0xfffffu)) : -1;
            out_dist[(size_t)p * cap + qi] = any ? (int32_t)((512u - (b >> 20)) >> 1) : -1;
            if (TRI) s_match[(wv * TILES + t) * 32 + lane] = any ? (int32_t)(0xfffffu - (b & 0xfffffu)) : -1;
        }
    }
    if (TRI) {                                               // whole waves: thread i of the block takes query q0 + i
        __syncthreads();
        const int i = threadIdx.x;
        if (i < 128 * TILES && q0 + i < nq) tri_point(tt, p, cap, q0 + i, s_match[i]);
    }
}

// ------------------------------------------------------------------------------------------------
// tri_solve (tri_solve.h): one-sided Jacobi SVD of the 4x4 DLT matrix, shared with the tracker's key-frame turn

__device__ __forceinline__ void tri_point(const TriTail& tt, int p, int cap, int i, int j) {
    const size_t o = (size_t)p * cap + i;
    if (j < 0 || j >= cap) { tt.ok[o] = 0;       // no match (or an index outside the pair's slots: treated as none)
        tt.xyz[3 * o] = tt.xyz[3 * o + 1] = tt.xyz[3 * o + 2] = 0; return; }
    const double ul = tt.kl[o].x, vl = tt.kl[o].y;
    const myslam_keypoint r = tt.kr[(size_t)p * cap + j];
    const double ur = r.x, vr = r.y;
    const double P[2][12] = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0},
                             {1, 0, 0, -tt.baseline, 0, 1, 0, 0, 0, 0, 1, 0}};      // system.cpp:108-116,141-145
    const double pt[2][2] = {{(ul - tt.cx) / tt.fx, (vl - tt.cy) / tt.fy}, {(ur - tt.cx) / tt.fx, (vr - tt.cy) / tt.fy}};   // camera.cpp:22-26
    double X[3], ratio;
    tri_solve(P, pt, X, ratio);
    tt.xyz[3 * o] = X[0]; tt.xyz[3 * o + 1] = X[1]; tt.xyz[3 * o + 2] = X[2];
    tt.ok[o] = (ratio < 1e-2 && X[2] > 0) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_triangulate(const float* __restrict__ xl, const float* __restrict__ yl,
                                                     const float* __restrict__ xr, const float* __restrict__ yr,
                                                     const myslam_keypoint* __restrict__ kl, const myslam_keypoint* __restrict__ kr,
                                                     const int32_t* __restrict__ match, const int32_t* __restrict__ nlv,
                                                     int cap, int n_single, double fx, double fy, double cx, double cy,
                                                     double baseline, double* __restrict__ xyz, uint8_t* __restrict__ ok) {
    const int p = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = nlv ? min(nlv[p], cap) : n_single;
    if (i >= n) return;
    const size_t o = (size_t)p * cap + i;
    if (kl) { tri_point(TriTail{kl, kr, fx, fy, cx, cy, baseline, xyz, ok}, p, cap, i, match[o]); return; }      // (the same code as the one-pair matcher's tail)
    const double ul = xl[i], vl = yl[i], ur = xr[i], vr = yr[i];
    const double P[2][12] = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0},
                             {1, 0, 0, -baseline, 0, 1, 0, 0, 0, 0, 1, 0}};      // system.cpp:108-116,141-145
    const double pt[2][2] = {{(ul - cx) / fx, (vl - cy) / fy}, {(ur - cx) / fx, (vr - cy) / fy}};   // camera.cpp:22-26
    double X[3], ratio;
    tri_solve(P, pt, X, ratio);
    xyz[3 * o] = X[0]; xyz[3 * o + 1] = X[1]; xyz[3 * o + 2] = X[2];
    ok[o] = (ratio < 1e-2 && X[2] > 0) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// LoopClosing::MatchFeatures after the matcher (src/loopclosing.cpp:175-198) and the point gather at the top of ComputeCorrectPose (:210-253)
// for one loop candidate per workgroup: what myslam_match_feature_pairs and its callers' gather loops do on the host, on the matcher's output
// where it lies.  The reference's std::set<std::pair<int,int>> becomes a sort of the keys (current id << 16 | loop id) in LDS followed by
// adjacent-unique; every list is written by an ORDERED compaction (dev_tables.h's block_rank in its run-time form: the launch picks the block
// size), so a slot never depends on which wave came first.
constexpr int LM_MAX_CAP = 16384;                 // keys of one item in LDS: 64 KB
constexpr int LM_MAX_FEAT = 65536;                // a feature id is half a key
constexpr int LM_MAX_OUT = 4096;                  // match slots of the verify handle (myslam_pnp_create)
constexpr uint32_t LM_PAD = 0xffffffffu;          // sorts last; equal to the largest real key at most, and only the first m sorted keys are read

struct LoopPairsArgs {
    const int32_t* n_loop; const int32_t* n_cur;
    const myslam_keypoint* loop_pyr; const myslam_keypoint* cur_pyr;
    int cap;
    const float* cur_feat_xy; const int32_t* loop_feat_landmark; int feat_cap;
    const double* landmark_pos; size_t landmark_stride; int landmark_cap;
    int min_matches, out_cap;
    const int32_t* train_idx; const int32_t* dist;
    int32_t* pairs; int32_t* n_pairs; int32_t* valid_pairs;
    float* pts3d; float* pts2d; int32_t* counts; int32_t* status;
};

__global__ __launch_bounds__(1024) void k_loop_pairs(LoopPairsArgs a) {
    extern __shared__ uint32_t s_keys[];                     // next power of two >= cap keys
    __shared__ int s_w[16], s_red[16];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, wv = tid >> 6, nw = nt >> 6;
    const int nl = clamped_count(a.n_loop, b, a.cap), nc = clamped_count(a.n_cur, b, a.cap);
    const size_t row0 = (size_t)b * a.cap, feat0 = (size_t)b * a.feat_cap;
    auto finish = [&](int status, int count) { if (tid == 0) { a.status[b] = status; a.counts[b] = count; } };
    if (nl == 0 || nc == 0) {                                // an empty side: no match, an empty set
        if (tid == 0) a.n_pairs[b] = 0;
        finish(0 < a.min_matches ? MYSLAM_LOOP_MATCH_FEW_PAIRS : MYSLAM_LOOP_MATCH_OK, 0);
        return;
    }
    // min_dist of :175-177
    int mn = 0x7fffffff;
    for (int i = tid; i < nl; i += nt) mn = min(mn, a.dist[row0 + i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mn = min(mn, __shfl_xor(mn, o, 64));
    if ((tid & 63) == 0) s_red[wv] = mn;
    __syncthreads();
    mn = s_red[0];
    for (int w = 1; w < nw; w++) mn = min(mn, s_red[w]);
    const double lim = fmax(2.0 * (double)mn, 30.0);         // :183
    // kept rows -> keys, in row order (:182-186)
    int m = 0;
    bool bad = false;
    for (int base = 0; base < nl; base += nt) {
        const int i = base + tid;
        bool keep = false;
        uint32_t key = 0;
        if (i < nl && (double)a.dist[row0 + i] <= lim) {
            const int t = a.train_idx[row0 + i];
            if (t < 0 || t >= nc) bad = true;
            else {
                const int c = a.cur_pyr[row0 + t].class_id, l = a.loop_pyr[row0 + i].class_id;
                if ((uint32_t)c >= (uint32_t)a.feat_cap || (uint32_t)l >= (uint32_t)a.feat_cap) bad = true;
                else { keep = true; key = ((uint32_t)c << 16) | (uint32_t)l; }
            }
        }
        int tot;
        const int r = block_rank(keep, s_w, tot);
        if (keep) s_keys[m + r] = key;
        m += tot;
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0) a.n_pairs[b] = 0;
        finish(MYSLAM_ERR_INVALID, 0);
        return;
    }
    // the set's order: bitonic sort over the next power of two >= m (m >= 1: the minimum row is always kept), padding last
    int S = 1;
    while (S < m) S <<= 1;
    for (int i = m + tid; i < S; i += nt) s_keys[i] = LM_PAD;
    __syncthreads();
    for (int k = 2; k <= S; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (S >> 1); t += nt) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const uint32_t x = s_keys[i], y = s_keys[l];
                if ((x > y) == ((i & k) == 0)) { s_keys[i] = y; s_keys[l] = x; }
            }
            __syncthreads();
        }
    // one entry per feature pair (:188-192): adjacent-unique, compacted in place — an element moves to a slot at or below its own, and the
    // last slot of a chunk can only be rewritten with its own value, so the next chunk still finds its left neighbour there
    int u = 0;
    for (int base = 0; base < m; base += nt) {
        const int i = base + tid;
        bool first = false;
        uint32_t key = 0;
        if (i < m) { key = s_keys[i]; first = i == 0 || s_keys[i - 1] != key; }
        int tot;
        const int r = block_rank(first, s_w, tot);            // (its barriers stand between the reads above and the writes below)
        if (first) {
            s_keys[u + r] = key;
            a.pairs[2 * (row0 + u + r)] = (int32_t)(key >> 16);
            a.pairs[2 * (row0 + u + r) + 1] = (int32_t)(key & 0xffffu);
        }
        u += tot;
        __syncthreads();
    }
    if (tid == 0) a.n_pairs[b] = u;
    if (u < a.min_matches) { finish(MYSLAM_LOOP_MATCH_FEW_PAIRS, 0); return; }      // :198
    // ComputeCorrectPose :218-237: pairs whose loop feature has no map point leave the set.  Counted first: nothing is written unless all fits.
    int nsurv = 0;
    bad = false;
    for (int k = tid; k < u; k += nt) {
        const int slot = a.loop_feat_landmark[feat0 + (s_keys[k] & 0xffffu)];
        if (slot < -1 || slot >= a.landmark_cap) bad = true;
        else nsurv += slot >= 0;
    }
    nsurv = wave_reduce_sum(nsurv);
    if ((tid & 63) == 0) s_red[wv] = nsurv;
    if (__syncthreads_or(bad)) { finish(MYSLAM_ERR_INVALID, 0); return; }
    nsurv = 0;
    for (int w = 0; w < nw; w++) nsurv += s_red[w];
    if (nsurv > a.out_cap) { finish(MYSLAM_ERR_CAPACITY, 0); return; }
    const size_t out0 = (size_t)b * a.out_cap;
    const double* pos = a.landmark_pos + (size_t)b * a.landmark_stride * 3;
    int n = 0;
    for (int base = 0; base < u; base += nt) {
        const int k = base + tid;
        uint32_t key = 0;
        int slot = -1;
        if (k < u) { key = s_keys[k]; slot = a.loop_feat_landmark[feat0 + (key & 0xffffu)]; }
        int tot;
        const int r = block_rank(slot >= 0, s_w, tot);
        if (slot >= 0) {
            const size_t o = out0 + n + r;
            const int c = (int)(key >> 16);
            a.valid_pairs[2 * o] = c; a.valid_pairs[2 * o + 1] = (int32_t)(key & 0xffffu);
            a.pts2d[2 * o] = a.cur_feat_xy[2 * (feat0 + c)]; a.pts2d[2 * o + 1] = a.cur_feat_xy[2 * (feat0 + c) + 1];      // :223-224
#pragma unroll
            for (int d = 0; d < 3; d++) a.pts3d[3 * o + d] = (float)pos[3 * (size_t)slot + d];      // cv::Point3f(pos(0), pos(1), pos(2)), :226
        }
        n += tot;
    }
    finish(n < a.min_matches ? MYSLAM_LOOP_MATCH_FEW_POINTS : MYSLAM_LOOP_MATCH_OK, n);      // :252
}

}  // namespace myslam_hip

using namespace myslam_hip;

extern "C" {

int myslam_hamming_match_batch(const uint8_t* d_q, const int32_t* d_nq, const uint8_t* d_t, const int32_t* d_nt, int batch,
                               int cap, int32_t* d_train_idx, int32_t* d_dist, void* hip_stream) {
    if (!d_q || !d_t || !d_nq || !d_nt || batch <= 0 || cap <= 0 || !d_train_idx || !d_dist) return MYSLAM_ERR_INVALID;
    if (cap >= (1 << 20)) return MYSLAM_ERR_UNSUPPORTED;          // the running minimum packs (distance, train index) into 32 bits
    hipStream_t s = (hipStream_t)hip_stream;
    ScopedProf sp(P_MATCH, s);
    if (batch < HQ_NARROW_BELOW)
        hipLaunchKernelGGL((k_hamming_fp4<1, HQ_SPLIT>), dim3((cap + 127) / 128, batch), dim3(256 * HQ_SPLIT), 0, s, d_q, d_nq, d_t, d_nt, cap, 0, 0, d_train_idx, d_dist, TriTail{});
    else
        hipLaunchKernelGGL(k_hamming_fp4<HQ_TILES>, dim3((cap + HQ_BLOCK - 1) / HQ_BLOCK, batch), dim3(256), 0, s, d_q, d_nq, d_t, d_nt, cap, 0, 0,
                           d_train_idx, d_dist, TriTail{});
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_hamming_match(const uint8_t* query, int nq, const uint8_t* train, int nt, int32_t* train_idx, int32_t* dist) {
    if (nq < 0 || nt < 0) return MYSLAM_ERR_INVALID;
    if (nq == 0) return MYSLAM_OK;
    if (!query || !train_idx || !dist || (nt > 0 && !train)) return MYSLAM_ERR_INVALID;
    if (nt >= (1 << 20)) return MYSLAM_ERR_UNSUPPORTED;
    if (need_device()) return MYSLAM_ERR_HIP;
    const int cap = std::max(nq, std::max(nt, 1));
    HostCall hc;                                               // thread-local staging: no allocation, one copy each way
    const int pq = hc.in(query, (size_t)nq * 32), pt = hc.in(train, (size_t)nt * 32);
    const int pi = hc.out(train_idx, (size_t)nq), pd = hc.out(dist, (size_t)nq);
    int rc = hc.upload();
    if (rc) return rc;
    const uint8_t* dq = hc.dev<uint8_t>(pq); const uint8_t* dt = hc.dev<uint8_t>(pt);
    int32_t* di = hc.dev<int32_t>(pi); int32_t* dd = hc.dev<int32_t>(pd);
    {
        ScopedProf sp(P_MATCH, hc.stream());
        hipLaunchKernelGGL((k_hamming_fp4<1, HQ_SPLIT>), dim3((nq + 127) / 128, 1), dim3(256 * HQ_SPLIT), 0, hc.stream(), dq, (const int32_t*)nullptr, dt,
                           (const int32_t*)nullptr, cap, nq, nt, di, dd, TriTail{});
    }
    MYSLAM_HIP_CHECK(hipGetLastError());
    return hc.download();
}

// src/loopclosing.cpp:175-186 — host bookkeeping (a handful of compares)
int myslam_hamming_filter(const int32_t* dist, int n, uint8_t* keep, int* min_dist) {
    if (n < 0 || (n > 0 && (!dist || !keep))) return MYSLAM_ERR_INVALID;
    if (n == 0) { if (min_dist) *min_dist = 0; return MYSLAM_OK; }
    int mn = dist[0];
    for (int i = 1; i < n; i++) mn = std::min(mn, dist[i]);
    const double lim = std::max(2.0 * (double)mn, 30.0);
    for (int i = 0; i < n; i++) keep[i] = ((double)dist[i] <= lim) ? 1 : 0;
    if (min_dist) *min_dist = mn;
    return MYSLAM_OK;
}

// LoopClosing::ProcessNewKF, src/loopclosing.cpp:94-105: every single-layer feature of the key-frame becomes nlevels pyramid key-points
// (octave = level, response = -1, class_id = index of the feature) — the input of ScreenAndComputeKPsParams.  Host bookkeeping.
int myslam_expand_pyramid_keypoints(const myslam_keypoint* feats, int n, int nlevels, myslam_keypoint* out /* n * nlevels */) {
    if (n < 0 || nlevels < 1 || (n > 0 && (!feats || !out))) return MYSLAM_ERR_INVALID;
    for (int i = 0; i < n; i++)
        for (int l = 0; l < nlevels; l++) {
            myslam_keypoint kp = feats[i];
            kp.octave = l; kp.response = -1.f; kp.class_id = i;
            out[(size_t)i * nlevels + l] = kp;
        }
    return MYSLAM_OK;
}

// LoopClosing::MatchFeatures, src/loopclosing.cpp:172-203, after the matcher: keep matches with distance <= max(2 * min_dist, 30),
// map both sides to their FEATURE ids through class_id and insert (current, loop) into a std::set — one entry per feature pair, in the
// set's order (ascending current id, then loop id), which is the order ComputeCorrectPose walks (:215-238).  query = loop key-frame's
// pyramid key-points, train = current key-frame's.  Returns MYSLAM_OK; the caller applies the `< 10 matches` rule (:196).
int myslam_match_feature_pairs(const int32_t* train_idx, const int32_t* dist, int n_query, const myslam_keypoint* loop_pyr_kps,
                               const myslam_keypoint* cur_pyr_kps, int n_train, int32_t* pairs /* n_query x 2: (current, loop) */, int* n_pairs) {
    if (n_query < 0 || !n_pairs || (n_query > 0 && (!train_idx || !dist || !loop_pyr_kps || !cur_pyr_kps || !pairs))) return MYSLAM_ERR_INVALID;
    *n_pairs = 0;
    if (n_query == 0) return MYSLAM_OK;
    int mn = dist[0];
    for (int i = 1; i < n_query; i++) mn = std::min(mn, dist[i]);
    const double lim = std::max(2.0 * (double)mn, 30.0);
    std::vector<std::pair<int, int>> v;
    for (int i = 0; i < n_query; i++) {
        if (train_idx[i] < 0 || train_idx[i] >= n_train) return MYSLAM_ERR_INVALID;
        if ((double)dist[i] <= lim) v.emplace_back(cur_pyr_kps[train_idx[i]].class_id, loop_pyr_kps[i].class_id);
    }
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    for (size_t k = 0; k < v.size(); k++) { pairs[2 * k] = v[k].first; pairs[2 * k + 1] = v[k].second; }
    *n_pairs = (int)v.size();
    return MYSLAM_OK;
}

// LoopClosing::MatchFeatures (src/loopclosing.cpp:167-203) and the gather of ComputeCorrectPose (:210-253) for `batch` candidates: the matcher's
// launch as myslam_hamming_match_batch makes it, then k_loop_pairs on its output — two dependent launches, nothing allocated, nothing read back.
int myslam_loop_match_batch(const uint8_t* d_loop_desc, const int32_t* d_n_loop, const uint8_t* d_cur_desc, const int32_t* d_n_cur,
                            const myslam_keypoint* d_loop_pyr, const myslam_keypoint* d_cur_pyr, int batch, int cap,
                            const float* d_cur_feat_xy, const int32_t* d_loop_feat_landmark, int feat_cap,
                            const double* d_landmark_pos, size_t landmark_stride, int landmark_cap, int min_matches, int out_cap,
                            int32_t* d_train_idx, int32_t* d_dist, int32_t* d_pairs, int32_t* d_n_pairs, int32_t* d_valid_pairs,
                            float* d_pts3d, float* d_pts2d, int32_t* d_counts, int32_t* d_status, void* hip_stream) {
    if (!d_loop_desc || !d_n_loop || !d_cur_desc || !d_n_cur || !d_loop_pyr || !d_cur_pyr || !d_cur_feat_xy || !d_loop_feat_landmark || !d_landmark_pos ||
        !d_train_idx || !d_dist || !d_pairs || !d_n_pairs || !d_valid_pairs || !d_pts3d || !d_pts2d || !d_counts || !d_status)
        return MYSLAM_ERR_INVALID;
    if (batch <= 0 || cap <= 0 || out_cap <= 0 || feat_cap <= 0 || landmark_cap < 0) return MYSLAM_ERR_INVALID;
    if (cap > LM_MAX_CAP || feat_cap > LM_MAX_FEAT || out_cap > LM_MAX_OUT) return MYSLAM_ERR_CAPACITY;
    hipStream_t s = (hipStream_t)hip_stream;
    int npad = 64;
    while (npad < cap) npad <<= 1;
    // the limit belongs to the function, not to a launch (see ba.hip): always what the largest cap needs
    MYSLAM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_loop_pairs), hipFuncAttributeMaxDynamicSharedMemorySize, LM_MAX_CAP * 4));
    const int rc = myslam_hamming_match_batch(d_loop_desc, d_n_loop, d_cur_desc, d_n_cur, batch, cap, d_train_idx, d_dist, hip_stream);
    if (rc) return rc;
    const LoopPairsArgs a{d_n_loop, d_n_cur, d_loop_pyr, d_cur_pyr, cap, d_cur_feat_xy, d_loop_feat_landmark, feat_cap, d_landmark_pos, landmark_stride,
                          landmark_cap, min_matches, out_cap, d_train_idx, d_dist, d_pairs, d_n_pairs, d_valid_pairs, d_pts3d, d_pts2d, d_counts, d_status};
    hipLaunchKernelGGL(k_loop_pairs, dim3(batch), dim3(npad >= 2048 ? 1024 : 256), (size_t)npad * 4, s, a);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_triangulate_stereo_batch(const myslam_keypoint* d_kps_l, const myslam_keypoint* d_kps_r, const int32_t* d_match,
                                    const int32_t* d_nl, int batch, int cap, double fx, double fy, double cx, double cy,
                                    double baseline, double* d_xyz, uint8_t* d_ok, void* hip_stream) {
    if (!d_kps_l || !d_kps_r || !d_match || !d_nl || batch <= 0 || cap <= 0 || !d_xyz || !d_ok) return MYSLAM_ERR_INVALID;
    hipStream_t s = (hipStream_t)hip_stream;
    ScopedProf sp(P_TRI, s);
    hipLaunchKernelGGL(k_triangulate, dim3((cap + 255) / 256, batch), dim3(256), 0, s, (const float*)nullptr, (const float*)nullptr,
                       (const float*)nullptr, (const float*)nullptr, d_kps_l, d_kps_r, d_match, d_nl, cap, 0, fx, fy, cx, cy,
                       baseline, d_xyz, d_ok);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

// BFMatcher.match + triangulation() of every match in one call: what the two calls above / below do, in ONE launch for a handful of pairs
int myslam_hamming_match_triangulate_batch(const uint8_t* d_q, const int32_t* d_nq, const uint8_t* d_t, const int32_t* d_nt,
                                           const myslam_keypoint* d_kps_l, const myslam_keypoint* d_kps_r, int batch, int cap,
                                           double fx, double fy, double cx, double cy, double baseline,
                                           int32_t* d_train_idx, int32_t* d_dist, double* d_xyz, uint8_t* d_ok, void* hip_stream) {
    if (!d_kps_l || !d_kps_r || !d_xyz || !d_ok) return MYSLAM_ERR_INVALID;
    if (batch >= HQ_NARROW_BELOW) {
        const int rc = myslam_hamming_match_batch(d_q, d_nq, d_t, d_nt, batch, cap, d_train_idx, d_dist, hip_stream);
        if (rc) return rc;
        return myslam_triangulate_stereo_batch(d_kps_l, d_kps_r, d_train_idx, d_nq, batch, cap, fx, fy, cx, cy, baseline, d_xyz, d_ok, hip_stream);
    }
    if (!d_q || !d_t || !d_nq || !d_nt || batch <= 0 || cap <= 0 || !d_train_idx || !d_dist) return MYSLAM_ERR_INVALID;
    if (cap >= (1 << 20)) return MYSLAM_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)hip_stream;
    ScopedProf sp(P_MATCH, s);
    hipLaunchKernelGGL((k_hamming_fp4<1, HQ_SPLIT, true>), dim3((cap + 127) / 128, batch), dim3(256 * HQ_SPLIT), 0, s, d_q, d_nq, d_t, d_nt, cap, 0, 0,
                       d_train_idx, d_dist, TriTail{d_kps_l, d_kps_r, fx, fy, cx, cy, baseline, d_xyz, d_ok});
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_triangulate_stereo(const float* xl, const float* yl, const float* xr, const float* yr, int n, double fx, double fy,
                              double cx, double cy, double baseline, double* xyz, uint8_t* ok) {
    if (n < 0) return MYSLAM_ERR_INVALID;
    if (n == 0) return MYSLAM_OK;
    if (!xl || !yl || !xr || !yr || !xyz || !ok) return MYSLAM_ERR_INVALID;
    if (need_device()) return MYSLAM_ERR_HIP;
    HostCall hc;
    const int p0 = hc.in(xl, (size_t)n), p1 = hc.in(yl, (size_t)n), p2 = hc.in(xr, (size_t)n), p3 = hc.in(yr, (size_t)n);
    const int px = hc.out(xyz, (size_t)n * 3), po = hc.out(ok, (size_t)n);
    int rc = hc.upload();
    if (rc) return rc;
    {
        ScopedProf sp(P_TRI, hc.stream());
        hipLaunchKernelGGL(k_triangulate, dim3((n + 255) / 256, 1), dim3(256), 0, hc.stream(), hc.dev<float>(p0), hc.dev<float>(p1),
                           hc.dev<float>(p2), hc.dev<float>(p3), (const myslam_keypoint*)nullptr, (const myslam_keypoint*)nullptr,
                           (const int32_t*)nullptr, (const int32_t*)nullptr, n, n, fx, fy, cx, cy, baseline, hc.dev<double>(px), hc.dev<uint8_t>(po));
    }
    MYSLAM_HIP_CHECK(hipGetLastError());
    return hc.download();
}

}  // extern "C"
