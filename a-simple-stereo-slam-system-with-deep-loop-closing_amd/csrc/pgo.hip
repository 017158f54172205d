// pgo.hip — loop correction on gfx950: LoopClosing::PoseGraphOptimization (src/loopclosing.cpp:537-646)   [SURVEY.md §8(f) rank 3]
//
// The reference hands g2o one VertexPose per key-frame (left-multiplied SE3 update, g2o_types.h:32-37), one EdgePoseGraph
// (error = log(M^-1 v0 v1^-1), information I6, g2o_types.h:157-167) per (KF, previous KF) and per (KF, loop KF), lets g2o
// differentiate the edges numerically (linearizeOplus is commented out, g2o_types.h:168-182: central differences, delta = 1e-9)
// and runs Levenberg-Marquardt for 20 iterations over a sparse Cholesky.  Afterwards every map point outside the active
// window moves rigidly with the key-frame that first observed it (:621-633).
//
// Device design.  A key-frame graph is a chain plus a handful of loop edges, so the normal equations are block tridiagonal
// apart from the rows of a few "separator" key-frames S (one endpoint per off-chain edge; chosen on the host from the edge
// list, at most PG_MAXS).  With T = the remaining free key-frames in index order:
//      [ Htt  C  ] [xT]   [bT]       Htt block tridiagonal (6x6 blocks D_t, B_t)
//      [ C^T  Hss] [xS] = [bS]       C = couplings T-S (sparse), Hss dense 6|S| x 6|S|
//   linearize   one thread per (edge, vertex side, tangent coordinate): 2 error evaluations -> one Jacobian column
//   assemble    one wave per 6x6 destination block, summing J^T J over that block's edge list in list order (deterministic)
//   sweep       block Cholesky of Htt + lambda I down the chain fused with the forward substitution of the 6|S|+1 right-hand
//               sides [C | bT]: one lane per right-hand side, the 6x6 factor chain recomputed in every lane (no barriers)
//   syrk        Z^T Z with v_mfma_f64_16x16x4 (one wave per 16x16 tile and K chunk), Z = L^-1 [C | bT]
//   schur       (Hss + lambda I - Z^T Z) xS = bS - Z^T z: dense Cholesky in one workgroup
//   back        y = z - Z xS (row parallel), then the backward chain xT_t = L_t^-T (y_t - W_{t+1}^T xT_{t+1})
//   update      pose <- exp(x) * pose per key-frame, chi2 per edge, fixed-order reductions
// The Levenberg control flow (lambda, rho, accept / reject: g2o OptimizationAlgorithmLevenberg) runs on the host on three
// scalars read back per trial; all arithmetic on poses, Jacobians and the linear system stays on the device, in double.
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <tuple>
#include <vector>

#include "common.h"
#include "pg_shared.h"

namespace myslam_hip {

constexpr int PG_MAXS = 96;          // separator key-frames of the FAST path (dense Schur system up to 576 x 576: pivots in LDS, the back substitution in registers)
constexpr int PG_MAXS_BIG = 1024;    // separator key-frames of the general path (round 6): the same factorisation with its pivots and right-hand side in device
                                     // memory — g2o + CSparse take any graph (src/loopclosing.cpp:538-543); slower is fine, refusing is not
constexpr int PG_KS = 32;            // K chunks of the Z^T Z product

// poses -> unit quaternions; measurements -> their inverses
__global__ void k_pg_prepare(double* poses, int n, const double* meas, double* minv, int E) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { Se3 T = pg_load(poses + 7 * i); pg_qnorm(T.q); pg_store(T, poses + 7 * i); }
    if (i < E) { Se3 M = pg_load(meas + 7 * i); pg_qnorm(M.q); pg_store(pg_inv(M), minv + 7 * i); }
}

// one thread per (edge, side, tangent coordinate): g2o BaseBinaryEdge::linearizeOplus numeric branch
__global__ void k_pg_linearize(const double* __restrict__ poses, const double* __restrict__ minv, const int32_t* __restrict__ e0,
                               const int32_t* __restrict__ e1, const uint8_t* __restrict__ fixedv, int E,
                               double* __restrict__ J /*E x 2 x 36*/, double* __restrict__ err /*E x 6*/) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id < 12 * E) pg_jacobian_column(id, poses, minv, e0, e1, fixedv, J, err);
}

__global__ void __launch_bounds__(256) k_pg_chi2(const double* __restrict__ poses, const double* __restrict__ minv, const int32_t* __restrict__ e0,
                                                 const int32_t* __restrict__ e1, int E, double* __restrict__ partial) {
    __shared__ double sm[256];
    const int k = blockIdx.x * 256 + threadIdx.x;
    const double s = pg_block_reduce<256>(k < E ? pg_edge_chi2(poses, minv, e0, e1, k) : 0.0, sm, 0);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// out[slot] = sum (mode 0) or max |.| (mode 1) of v[0..n), fixed order; one workgroup
__global__ void __launch_bounds__(256) k_pg_reduce(const double* __restrict__ v, int n, double* out, int mode) {
    __shared__ double sm[256];
    double a = 0;
    for (int i = threadIdx.x; i < n; i += 256) a = mode ? fmax(a, fabs(v[i])) : a + v[i];
    a = pg_block_reduce<256>(a, sm, mode);
    if (threadIdx.x == 0) *out = a;
}

// One wave per destination 6x6 block.  kind 0: D_t (+ bT_t into column mS of C)  1: B_t  2: C block (t, s)
//                                      3: Hss diagonal block (+ bS)                4: Hss block (s > s')
struct PgJob { int kind, a, b, begin, end; };

__global__ void __launch_bounds__(64) k_pg_assemble(const PgJob* __restrict__ jobs, const int2* __restrict__ list, const double* __restrict__ J,
                                                    const double* __restrict__ err, double* __restrict__ D, double* __restrict__ B,
                                                    double* __restrict__ C, double* __restrict__ Hss, double* __restrict__ bS,
                                                    double* __restrict__ diag, int ldz, int mS, int nT) {
    const PgJob jb = jobs[blockIdx.x];
    const int lane = threadIdx.x;
    const bool isb = lane >= 36;
    if (lane >= 42 || (isb && !(jb.kind == 0 || jb.kind == 3))) return;
    const int r = isb ? lane - 36 : lane / 6, c = isb ? 0 : lane - 6 * r;
    double sum = 0;
    for (int i = jb.begin; i < jb.end; i++) {
        const int2 en = list[i];
        const double* Jr = J + ((size_t)en.x * 2 + (en.y & 1)) * 36;
        const double* Jc = J + ((size_t)en.x * 2 + (en.y >> 1)) * 36;
        double h;
        if (!isb) h = pg_jtj(Jr, Jc, r, c);
        else h = pg_jte(Jr, err + (size_t)en.x * 6, r);
        sum += h;
    }
    switch (jb.kind) {
    case 0:
        if (isb) C[(size_t)(6 * jb.a + r) * ldz + mS] = -sum;
        else { D[(size_t)jb.a * 36 + r * 6 + c] = sum; if (r == c) diag[6 * jb.a + r] = sum; }
        break;
    case 1: B[(size_t)jb.a * 36 + r * 6 + c] = sum; break;
    case 2: C[(size_t)(6 * jb.a + r) * ldz + 6 * jb.b + c] = sum; break;
    case 3:
        if (isb) bS[6 * jb.a + r] = -sum;
        else { Hss[(size_t)(6 * jb.a + r) * ldz + 6 * jb.a + c] = sum; if (r == c) diag[6 * (nT + jb.a) + r] = sum; }
        break;
    default: Hss[(size_t)(6 * jb.a + r) * ldz + 6 * jb.b + c] = sum; break;
    }
}

// pg_sweep (pg_shared.h) over the columns of one 64-lane block; blockIdx.y = chain segment [seg[y], seg[y+1]): no block couples two segments
// (B = 0 at a segment start), so segments run in parallel.
__global__ void __launch_bounds__(64) k_pg_sweep(const double* __restrict__ D, const double* __restrict__ B, const double* __restrict__ C,
                                                 double* __restrict__ Z, double* __restrict__ Lw, const int32_t* __restrict__ seg, int ldz,
                                                 double lambda, int* __restrict__ status) {
    const int col = blockIdx.x * 64 + threadIdx.x;
    const bool bad = pg_sweep(D, B, C, Z, Lw, seg[blockIdx.y], seg[blockIdx.y + 1], ldz, lambda, col);
    if (bad && col == 0) *status = 1;
}

// P[ks][tile][v][lane] = partial Z^T Z over K chunk ks for the lower 16x16 tile (ti >= tj); one wave per (tile, ks)
typedef double pg_d4 __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(64) k_pg_syrk(const double* __restrict__ Z, double* __restrict__ P, int ldz, int k4 /*groups of 4 rows*/, int ntile) {
    const int tile = blockIdx.x, ks = blockIdx.y, lane = threadIdx.x;
    int ti, tj;
    pg_tri_decode(tile, ti, tj);
    const int per = (k4 + PG_KS - 1) / PG_KS, g0 = ks * per, g1 = min(k4, g0 + per);
    pg_d4 acc = {0, 0, 0, 0};
    const double* pa = Z + (size_t)(lane >> 4) * ldz + 16 * ti + (lane & 15);
    const double* pb = Z + (size_t)(lane >> 4) * ldz + 16 * tj + (lane & 15);
    for (int g = g0; g < g1; g++) {
        const double av = pa[(size_t)g * 4 * ldz], bv = pb[(size_t)g * 4 * ldz];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
    double* o = P + ((size_t)ks * ntile + tile) * 256;
#pragma unroll
    for (int v = 0; v < 4; v++) o[v * 64 + lane] = acc[v];
}

__device__ __forceinline__ double pg_ztz(const double* __restrict__ P, int ntile, int i, int j) {      // (Z^T Z)(i, j), i-tile >= j-tile
    const int ti = i >> 4, tj = j >> 4, tile = ti * (ti + 1) / 2 + tj, r = i & 15, c = j & 15;
    const size_t o = (size_t)tile * 256 + (size_t)(r >> 2) * 64 + (r & 3) * 16 + c;
    double s = 0;
    for (int ks = 0; ks < PG_KS; ks++) s += P[(size_t)ks * ntile * 256 + o];
    return s;
}

// (Hss + lambda I - Z^T Z) xS = bS - Z^T z   — blocked dense Cholesky in one workgroup (16 waves), matrix A (ld = ldz) in L2.
// The right-hand side rides along as row mS of A, so the factorisation leaves L^-1 rhs there (no separate forward pass).
// Per 16-column panel: wave 0 factors the 16x16 diagonal tile in LDS, one thread per row below solves its 16 panel entries
// against it, then the trailing matrix takes A[ti][tj] -= X_ti X_tj^T as v_mfma_f64_16x16x4 tiles spread over the waves.
// The backward substitution runs in wave 0 alone (rows of L are contiguous).
#define PG_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
template <bool BIG>
__global__ void __launch_bounds__(1024) k_pg_schur(const double* __restrict__ Hss, const double* __restrict__ bS, const double* __restrict__ P,
                                                   double* __restrict__ A, double* __restrict__ xS, int mS, int ldz, int ntile, int haveZ,
                                                   double lambda, int* __restrict__ status, double* __restrict__ gInv) {
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5, lane = tid & 63, wv = tid >> 6;
    __shared__ double sD[16][17];
    __shared__ double sInvLds[BIG ? 16 : 6 * PG_MAXS + 16];
    double* const sInv = BIG ? gInv : sInvLds;          // BIG (more than PG_MAXS separators): the reciprocal pivots live in device memory (written by one lane, read after barriers)
    __shared__ int sbad;
    if (tid == 0) sbad = 0;
    for (int i = ty; i < ldz; i += 32)
        for (int j = tx; j < ldz; j += 32) {
            double v = 0;
            if (pg_schur_kept(i, j, mS)) {
                v = pg_schur_entry(Hss, bS, i, j, mS, ldz, lambda);
                if (haveZ) v -= pg_ztz(P, ntile, i, j);
            }
            A[(size_t)i * ldz + j] = v;
        }
    __syncthreads();
    const int nt = ldz >> 4;
    for (int p = 0; 16 * p < mS; p++) {
        const int c0 = 16 * p;
        if (tid < 256) sD[tid >> 4][tid & 15] = A[(size_t)(c0 + (tid >> 4)) * ldz + c0 + (tid & 15)];
        __syncthreads();
        if (wv == 0) {                               // unblocked factor of the diagonal tile, lane r = row r
            const int r = lane & 15;
            for (int j = 0; j < 16 && c0 + j < mS; j++) {
                double piv = sD[j][j];
                if (!(piv > 0)) { if (lane == 0) sbad = 1; piv = 1.0; }
                const double d = sqrt(piv), inv = 1.0 / d;
                double l = 0;
                if (lane < 16 && r > j) { l = sD[r][j] * inv; sD[r][j] = l; }
                if (lane == j) { sD[j][j] = d; sInv[c0 + j] = inv; }
                PG_WAVE_SYNC();
                if (lane < 16 && r > j) for (int k = j + 1; k <= r; k++) sD[r][k] -= l * sD[k][j];
                PG_WAVE_SYNC();
            }
        }
        __syncthreads();
        if (tid < 256 && (tid & 15) <= (tid >> 4)) A[(size_t)(c0 + (tid >> 4)) * ldz + c0 + (tid & 15)] = sD[tid >> 4][tid & 15];
        const int ncol = min(16, mS - c0);
        for (int i = c0 + 16 + tid; i <= mS; i += 1024) {       // panel rows below the tile: X = A_panel Ld^-T
            double* row = A + (size_t)i * ldz + c0;
            double x[16];
#pragma unroll
            for (int j = 0; j < 16; j++) x[j] = row[j];
#pragma unroll
            for (int j = 0; j < 16; j++) {
                if (j < ncol) {
                    double v = x[j];
#pragma unroll
                    for (int k = 0; k < j; k++) v -= x[k] * sD[j][k];
                    x[j] = v * sInv[c0 + j];
                }
            }
#pragma unroll
            for (int j = 0; j < 16; j++) row[j] = x[j];
        }
        __syncthreads();
        // trailing update: tile (ti, tj), p < tj <= ti < nt; A-operand lane value X[16 ti + (lane & 15)][c0 + 4 g + (lane >> 4)]
        const int nrem = nt - p - 1, ntr = nrem * (nrem + 1) / 2;
        for (int q = wv; q < ntr; q += 16) {
            int ti, tj;
            pg_tri_decode(q, ti, tj);
            ti += p + 1; tj += p + 1;
            const double* pa = A + (size_t)(16 * ti + (lane & 15)) * ldz + c0 + (lane >> 4);
            const double* pb = A + (size_t)(16 * tj + (lane & 15)) * ldz + c0 + (lane >> 4);
            double* pc = A + (size_t)(16 * ti + (lane >> 4)) * ldz + 16 * tj + (lane & 15);
            double av[4], bv[4];
            pg_d4 acc;
#pragma unroll
            for (int g = 0; g < 4; g++) { av[g] = pa[4 * g]; bv[g] = pb[4 * g]; }
#pragma unroll
            for (int v = 0; v < 4; v++) acc[v] = -pc[(size_t)4 * v * ldz];
#pragma unroll
            for (int g = 0; g < 4; g++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[g], bv[g], acc, 0, 0, 0);
#pragma unroll
            for (int v = 0; v < 4; v++) pc[(size_t)4 * v * ldz] = -acc[v];
        }
        __syncthreads();
    }
    if constexpr (BIG) {
        // backward substitution L^T x = y with y = row mS of A in device memory, the whole workgroup on every column (same order of subtractions per entry)
        double* y = A + (size_t)mS * ldz;
        for (int j = mS - 1; j >= 0; j--) {
            __syncthreads();
            const double xj = y[j] * sInv[j];
            const double* Lj = A + (size_t)j * ldz;
            for (int k = tid; k < j; k += 1024) y[k] -= Lj[k] * xj;
            if (tid == 0) xS[j] = xj;
        }
        if (tid == 0 && sbad) *status = 1;
        return;
    }
    // backward substitution L^T x = y in wave 0: lane l owns x[l], x[l + 64], ...
    if (tid < 64) {
        constexpr int PER = (6 * PG_MAXS + 63) / 64;
        double yv[PER];
#pragma unroll
        for (int q = 0; q < PER; q++) { const int k = tid + 64 * q; yv[q] = k < mS ? A[(size_t)mS * ldz + k] : 0.0; }
        for (int j = mS - 1; j >= 0; j--) {
            double mine = 0;
#pragma unroll
            for (int q = 0; q < PER; q++) if (q == (j >> 6)) mine = yv[q];
            const double xj = __shfl(mine, j & 63, 64) * sInv[j];
            if (tid == (j & 63)) {
#pragma unroll
                for (int q = 0; q < PER; q++) if (q == (j >> 6)) yv[q] = xj;
            }
            const double* Lj = A + (size_t)j * ldz;
#pragma unroll
            for (int q = 0; q < PER; q++) { const int k = tid + 64 * q; if (k < j) yv[q] -= Lj[k] * xj; }
        }
#pragma unroll
        for (int q = 0; q < PER; q++) { const int k = tid + 64 * q; if (k < mS) xS[k] = yv[q]; }
    }
    if (tid == 0 && sbad) *status = 1;
}

// y = z - Z[:, 0..mS) xS, one thread per row
__global__ void __launch_bounds__(256) k_pg_y(const double* __restrict__ Z, const double* __restrict__ xS, double* __restrict__ y, int rows, int ldz, int mS) {
    __shared__ double sx[6 * PG_MAXS];
    const bool big = mS > 6 * PG_MAXS;                  // the general path reads xS from device memory (block-uniform)
    if (!big) for (int i = threadIdx.x; i < mS; i += 256) sx[i] = xS[i];
    __syncthreads();
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= rows) return;
    const double* zr = Z + (size_t)k * ldz;
    double s = zr[mS];
    if (!big) { for (int j = 0; j < mS; j++) s -= zr[j] * sx[j]; }
    else { for (int j = 0; j < mS; j++) s -= zr[j] * xS[j]; }
    y[k] = s;
}

// xT_t = L_t^-T (y_t - W_{t+1}^T xT_{t+1}), the backward chain of one segment per workgroup (W = 0 across segment boundaries)
__global__ void __launch_bounds__(64) k_pg_back(const double* __restrict__ Lw, const double* __restrict__ y, double* __restrict__ xT,
                                                const int32_t* __restrict__ seg) {
    pg_back(Lw, y, xT, seg[blockIdx.x], seg[blockIdx.x + 1], threadIdx.x);
}

// pose <- exp(x) * pose for every free key-frame; sc[v] = x . (lambda x + b)
__global__ void __launch_bounds__(256) k_pg_update(double* __restrict__ poses, const int32_t* __restrict__ slot /*n: -1 fixed, t, or nT + s*/,
                                                   int n, int nT, const double* __restrict__ xT, const double* __restrict__ xS,
                                                   const double* __restrict__ C, const double* __restrict__ bS, int ldz, int mS, double lambda,
                                                   double* __restrict__ sc) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const int sl = slot[v];
    sc[v] = sl >= 0 ? pg_update_pose(poses + 7 * v, sl, nT, xT, xS, C, bS, ldz, mS, lambda) : 0.0;
}

// src/loopclosing.cpp:621-633: p <- T_new[kf]^-1 * (T_old[kf] * p)
__global__ void __launch_bounds__(256) k_correct_map_points(const double* __restrict__ oldp, const double* __restrict__ newp, int nposes,
                                                            const int32_t* __restrict__ kf, double* __restrict__ pts, int npts, int* __restrict__ status) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= npts) return;
    const int k = kf[i];
    if (k < 0) return;
    if (k >= nposes) { *status = MYSLAM_ERR_INVALID; return; }
    pg_move_point(pg_load(oldp + 7 * k), pg_load(newp + 7 * k), pts + 3 * i);
}

}  // namespace myslam_hip

using namespace myslam_hip;

extern "C" {

int myslam_pose_graph_optimize(double* poses, int n, const uint8_t* fixed, const int32_t* edge_v0, const int32_t* edge_v1,
                               const double* meas, int n_edges, int max_iters, double* final_chi2, int* iters) {
    if (n < 0 || n_edges < 0 || max_iters < 0 || (n > 0 && !poses) || (n_edges > 0 && (!edge_v0 || !edge_v1 || !meas))) return MYSLAM_ERR_INVALID;
    const int E = n_edges;
    for (int k = 0; k < E; k++)
        if (edge_v0[k] < 0 || edge_v0[k] >= n || edge_v1[k] < 0 || edge_v1[k] >= n || edge_v0[k] == edge_v1[k]) return MYSLAM_ERR_INVALID;
    if (need_device()) return MYSLAM_ERR_HIP;
    if (final_chi2) *final_chi2 = 0;
    if (iters) *iters = 0;
    if (n == 0) return MYSLAM_OK;

    // ---- structure: fixed / chain (T) / separator (S) key-frames ----
    std::vector<uint8_t> fx(n, 0);
    if (fixed) for (int i = 0; i < n; i++) fx[i] = fixed[i] ? 1 : 0;
    std::vector<char> inS(n, 0);
    std::vector<int> tpos(n, -1), deg(n);
    int nS = 0, nT = 0;
    for (;;) {
        nT = 0;
        for (int i = 0; i < n; i++) tpos[i] = (!fx[i] && !inS[i]) ? nT++ : -1;
        std::fill(deg.begin(), deg.end(), 0);
        bool any = false;
        for (int k = 0; k < E; k++) {
            const int a = tpos[edge_v0[k]], b = tpos[edge_v1[k]];
            if (a >= 0 && b >= 0 && std::abs(a - b) > 1) { deg[edge_v0[k]]++; deg[edge_v1[k]]++; any = true; }
        }
        if (!any) break;
        int best = -1;                                   // the key-frame on the most off-chain edges, latest on ties
        for (int i = 0; i < n; i++) if (deg[i] > 0 && (best < 0 || deg[i] >= deg[best])) best = i;
        inS[best] = 1;
        if (++nS > PG_MAXS_BIG) return MYSLAM_ERR_UNSUPPORTED;
    }
    const int sepBudget = nS <= PG_MAXS ? PG_MAXS : PG_MAXS_BIG;      // graphs that fit the fast path keep it (and their results of rounds 3-5)
    // Cut long chain runs with extra separators so that the serial sweeps (one step per key-frame of a run) become short and
    // run in parallel: run length ~ sqrt(11 nT) (measured optimum at 1500 key-frames) balances them against the dense Schur system, which grows by 6 per cut.
    auto chain_links = [&](std::vector<char>& link) {     // link[t] = an edge joins chain positions t-1 and t
        link.assign(nT + 1, 0);
        for (int k = 0; k < E; k++) {
            const int a = tpos[edge_v0[k]], b = tpos[edge_v1[k]];
            if (a >= 0 && b >= 0) link[std::max(a, b)] = 1;
        }
        if (nT > 0) link[0] = 0;
        link[nT] = 0;
    };
    std::vector<char> link;
    chain_links(link);
    {
        std::vector<int> tvert(nT);
        for (int i = 0; i < n; i++) if (tpos[i] >= 0) tvert[tpos[i]] = i;
        int lmax = std::max(16, (int)std::ceil(std::sqrt(11.0 * nT)));
        for (;; lmax *= 2) {
            std::vector<int> cuts;
            for (int s0 = 0; s0 < nT;) {
                int e = s0 + 1;
                while (e < nT && link[e]) e++;
                const int len = e - s0, parts = (len + 1 + lmax) / (lmax + 1);
                for (int i = 1; i < parts; i++) cuts.push_back(s0 + (int)((long long)i * len / parts));
                s0 = e;
            }
            if (nS + (int)cuts.size() > sepBudget) { if (cuts.empty()) return MYSLAM_ERR_UNSUPPORTED; continue; }
            for (int t : cuts) inS[tvert[t]] = 1;
            nS += (int)cuts.size();
            break;
        }
        nT = 0;
        for (int i = 0; i < n; i++) tpos[i] = (!fx[i] && !inS[i]) ? nT++ : -1;
        chain_links(link);
    }
    std::vector<int32_t> seg;                             // chain runs [seg[i], seg[i+1])
    for (int t = 0; t < nT; t++) if (!link[t]) seg.push_back(t);
    seg.push_back(nT);
    const int nseg = (int)seg.size() - 1;
    std::vector<int> spos(n, -1), slot(n, -1);
    { int s2 = 0; for (int i = 0; i < n; i++) if (inS[i]) spos[i] = s2++; }
    for (int i = 0; i < n; i++) slot[i] = tpos[i] >= 0 ? tpos[i] : (spos[i] >= 0 ? nT + spos[i] : -1);
    const int nF = nT + nS, mS = 6 * nS, ldz = ((mS + 1 + 15) / 16) * 16, nt16 = ldz / 16, ntile = nt16 * (nt16 + 1) / 2;
    const int rows = 6 * nT, k4 = (rows + 3) / 4, rowsPad = 4 * k4;

    // ---- assembly jobs: destination block -> list of (edge, row side | col side << 1) ----
    std::map<std::tuple<int, int, int>, std::vector<int2>> jobmap;
    for (int k = 0; k < E; k++) {
        const int v[2] = {edge_v0[k], edge_v1[k]};
        for (int s = 0; s < 2; s++) {
            if (slot[v[s]] < 0) continue;
            if (tpos[v[s]] >= 0) jobmap[{0, tpos[v[s]], 0}].push_back(make_int2(k, s | (s << 1)));
            else jobmap[{3, spos[v[s]], 0}].push_back(make_int2(k, s | (s << 1)));
        }
        if (slot[v[0]] < 0 || slot[v[1]] < 0) continue;
        const bool t0 = tpos[v[0]] >= 0, t1 = tpos[v[1]] >= 0;
        if (t0 && t1) {
            const int rs = tpos[v[0]] > tpos[v[1]] ? 0 : 1;       // row block = the later key-frame of the chain
            jobmap[{1, tpos[v[rs]], 0}].push_back(make_int2(k, rs | ((1 - rs) << 1)));
        } else if (t0 != t1) {
            const int rs = t0 ? 0 : 1;                             // rows = the chain key-frame, columns = the separator
            jobmap[{2, tpos[v[rs]], spos[v[1 - rs]]}].push_back(make_int2(k, rs | ((1 - rs) << 1)));
        } else {
            const int rs = spos[v[0]] > spos[v[1]] ? 0 : 1;
            jobmap[{4, spos[v[rs]], spos[v[1 - rs]]}].push_back(make_int2(k, rs | ((1 - rs) << 1)));
        }
    }
    std::vector<PgJob> jobs;
    std::vector<int2> list;
    for (auto& kv : jobmap) {
        PgJob j{std::get<0>(kv.first), std::get<1>(kv.first), std::get<2>(kv.first), (int)list.size(), 0};
        list.insert(list.end(), kv.second.begin(), kv.second.end());
        j.end = (int)list.size();
        jobs.push_back(j);
    }

    // ---- device state: one staged call (HostCall, common.h) ----
    const int nchi = (E + 255) / 256;
    const bool bigS = nS > PG_MAXS;
    const size_t nCZ = (size_t)rowsPad * ldz;
    HostCall hc;
    const int i_seg = hc.in(seg.data(), seg.size()), i_fx = hc.in(fx.data(), (size_t)n), i_slot = hc.in(slot.data(), (size_t)n);
    const int i_meas = hc.in(meas, (size_t)7 * E), i_e0 = hc.in(edge_v0, (size_t)E), i_e1 = hc.in(edge_v1, (size_t)E);
    const int i_jobs = hc.in(jobs.data(), jobs.size()), i_list = hc.in(list.data(), list.size());
    const int io_pose = hc.inout(poses, (size_t)7 * n);
    const int o_res = hc.out<double>(nullptr, 5);          // chi2, x . (lambda x + b), two spare, and the factorisations' status word behind them: one read per trial
    // blocks no job writes stay zero for the whole run (the sparsity pattern is fixed)
    const int z_D = hc.zero<double>((size_t)36 * nT), z_B = hc.zero<double>((size_t)36 * nT), z_C = hc.zero<double>(nCZ), z_Z = hc.zero<double>(nCZ);
    const int z_Hss = hc.zero<double>((size_t)ldz * ldz), z_bS = hc.zero<double>((size_t)ldz), z_diag = hc.zero<double>((size_t)6 * nF);
    const int z_xS = hc.zero<double>((size_t)ldz), z_xT = hc.zero<double>((size_t)rowsPad);
    const int t_save = hc.tmp<double>((size_t)7 * n), t_minv = hc.tmp<double>((size_t)7 * E), t_J = hc.tmp<double>((size_t)72 * E), t_err = hc.tmp<double>((size_t)6 * E);
    const int t_Lw = hc.tmp<double>((size_t)72 * nT), t_A = hc.tmp<double>((size_t)ldz * ldz), t_y = hc.tmp<double>((size_t)rowsPad);
    const int t_P = hc.tmp<double>((size_t)PG_KS * ntile * 256), t_sc = hc.tmp<double>((size_t)n), t_part = hc.tmp<double>((size_t)nchi);
    const int t_inv = hc.tmp<double>((size_t)ldz + 16);
    int it = 0, rc;
    if ((rc = hc.upload())) return rc;
    const hipStream_t st = hc.stream();                    // this thread's own non-blocking stream for every kernel, copy and memset of the call (never the legacy stream: common.h)
    const auto D = [&](int piece) { return hc.dev<double>(piece); };
    double *const d_pose = D(io_pose), *const d_save = D(t_save), *const d_meas = D(i_meas), *const d_minv = D(t_minv), *const d_J = D(t_J), *const d_err = D(t_err);
    double *const d_D = D(z_D), *const d_B = D(z_B), *const d_C = D(z_C), *const d_Z = D(z_Z), *const d_Lw = D(t_Lw), *const d_Hss = D(z_Hss), *const d_bS = D(z_bS);
    double *const d_A = D(t_A), *const d_xS = D(z_xS), *const d_xT = D(z_xT), *const d_y = D(t_y), *const d_P = D(t_P), *const d_diag = D(z_diag), *const d_sc = D(t_sc);
    double *const d_part = D(t_part), *const d_res = D(o_res), *const d_inv = D(t_inv);
    int32_t *const d_e0 = hc.dev<int32_t>(i_e0), *const d_e1 = hc.dev<int32_t>(i_e1), *const d_slot = hc.dev<int32_t>(i_slot), *const d_seg = hc.dev<int32_t>(i_seg);
    uint8_t* const d_fx = hc.dev<uint8_t>(i_fx);
    PgJob* const d_jobs = hc.dev<PgJob>(i_jobs);
    int2* const d_list = hc.dev<int2>(i_list);
    int* const d_status = reinterpret_cast<int*>(d_res + 4);
    const double* const res = hc.host<double>(o_res);      // valid after a fetch

    const int npe = std::max(n, E);
    hipLaunchKernelGGL(k_pg_prepare, dim3((npe + 255) / 256), dim3(256), 0, st, d_pose, n, d_meas, d_minv, E);
    auto chi2 = [&](double* out) -> int {               // d_res[0] <- sum of e^T e over all edges
        if (E == 0) { *out = 0; return MYSLAM_OK; }
        hipLaunchKernelGGL(k_pg_chi2, dim3(nchi), dim3(256), 0, st, d_pose, d_minv, d_e0, d_e1, E, d_part);
        hipLaunchKernelGGL(k_pg_reduce, dim3(1), dim3(256), 0, st, d_part, nchi, d_res, 0);
        const int rc_ = hc.fetch(o_res);
        *out = res[0];
        return rc_;
    };
    double currentChi = 0;
    if ((rc = chi2(&currentChi)) != MYSLAM_OK) return rc;
    if (nF > 0 && E > 0) {
        double lambda = 0, ni = 2;
        for (; it < max_iters; it++) {
            double tempChi = currentChi;
            hipLaunchKernelGGL(k_pg_linearize, dim3((12 * E + 127) / 128), dim3(128), 0, st, d_pose, d_minv, d_e0, d_e1, d_fx, E, d_J, d_err);
            hipLaunchKernelGGL(k_pg_assemble, dim3((unsigned)jobs.size()), dim3(64), 0, st, d_jobs, d_list, d_J, d_err, d_D, d_B, d_C, d_Hss, d_bS, d_diag,
                               ldz, mS, nT);
            if (it == 0) {                              // computeLambdaInit: tau * max diagonal
                hipLaunchKernelGGL(k_pg_reduce, dim3(1), dim3(256), 0, st, d_diag, 6 * nF, d_res, 1);
                if ((rc = hc.fetch(o_res))) return rc;
                lambda = 1e-5 * res[0]; ni = 2;
            }
            double rho = 0;
            int qmax = 0;
            do {
                MYSLAM_HIP_CHECK(hipMemcpyAsync(d_save, d_pose, sizeof(double) * 7 * n, hipMemcpyDeviceToDevice, st));
                MYSLAM_HIP_CHECK(hipMemsetAsync(d_status, 0, sizeof(int), st));
                if (nT > 0) {
                    hipLaunchKernelGGL(k_pg_sweep, dim3((ldz + 63) / 64, nseg), dim3(64), 0, st, d_D, d_B, d_C, d_Z, d_Lw, d_seg, ldz, lambda, d_status);
                    hipLaunchKernelGGL(k_pg_syrk, dim3(ntile, PG_KS), dim3(64), 0, st, d_Z, d_P, ldz, k4, ntile);
                }
                if (mS > 0) {
                    if (bigS) hipLaunchKernelGGL(k_pg_schur<true>, dim3(1), dim3(1024), 0, st, d_Hss, d_bS, d_P, d_A, d_xS, mS, ldz, ntile, nT > 0 ? 1 : 0, lambda, d_status, d_inv);
                    else hipLaunchKernelGGL(k_pg_schur<false>, dim3(1), dim3(1024), 0, st, d_Hss, d_bS, d_P, d_A, d_xS, mS, ldz, ntile, nT > 0 ? 1 : 0, lambda, d_status, d_inv);
                }
                if (nT > 0) {
                    hipLaunchKernelGGL(k_pg_y, dim3((rows + 255) / 256), dim3(256), 0, st, d_Z, d_xS, d_y, rows, ldz, mS);
                    hipLaunchKernelGGL(k_pg_back, dim3(nseg), dim3(64), 0, st, d_Lw, d_y, d_xT, d_seg);
                }
                hipLaunchKernelGGL(k_pg_update, dim3((n + 255) / 256), dim3(256), 0, st, d_pose, d_slot, n, nT, d_xT, d_xS, d_C, d_bS, ldz, mS, lambda, d_sc);
                hipLaunchKernelGGL(k_pg_reduce, dim3(1), dim3(256), 0, st, d_sc, n, d_res + 1, 0);
                hipLaunchKernelGGL(k_pg_chi2, dim3(nchi), dim3(256), 0, st, d_pose, d_minv, d_e0, d_e1, E, d_part);
                hipLaunchKernelGGL(k_pg_reduce, dim3(1), dim3(256), 0, st, d_part, nchi, d_res, 0);
                MYSLAM_HIP_CHECK(hipGetLastError());
                if ((rc = hc.fetch(o_res))) return rc;
                const bool ok = !*reinterpret_cast<const int*>(res + 4);
                tempChi = ok ? res[0] : 1e300;
                rho = currentChi - tempChi;
                double scale = 1e-3;
                if (ok) scale += res[1];
                rho /= scale;
                if (rho > 0 && std::isfinite(tempChi) && ok) {
                    double alpha = 1. - pow(2 * rho - 1, 3);                 // k_loop_correct (loop_correct.hip) writes t * t * t: kept apart, the two need not round alike
                    alpha = std::min(alpha, 2. / 3.);
                    lambda *= std::max(1. / 3., alpha); ni = 2; currentChi = tempChi;
                } else {
                    lambda *= ni; ni *= 2;
                    MYSLAM_HIP_CHECK(hipMemcpyAsync(d_pose, d_save, sizeof(double) * 7 * n, hipMemcpyDeviceToDevice, st));
                    if (!std::isfinite(lambda)) break;
                }
                qmax++;
            } while (rho < 0 && qmax < 10);
            if (qmax == 10 || rho == 0 || !std::isfinite(lambda)) { it++; break; }
        }
    }
    if ((rc = hc.download())) return rc;
    if (final_chi2) *final_chi2 = currentChi;
    if (iters) *iters = it;
    return MYSLAM_OK;
}

// LoopClosing::LoopLocalFusion, src/loopclosing.cpp:466-507 (the arithmetic; the re-linking of observations :509-532 is Map bookkeeping
// and stays with the integrator).  A handful of SE3 products on the host (unit quaternion + translation, renormalised after every
// product as Sophus does: se3_quat.h, the device's own functions), the map points on the device.
int myslam_loop_local_fusion(double* active_poses, int n_active, int cur, const double* corrected_cur_pose7, const int32_t* first_active_kf,
                             double* points, int n_points) {
    if (!active_poses || n_active < 1 || n_active > 64 || cur < 0 || cur >= n_active || !corrected_cur_pose7 || n_points < 0 ||
        (n_points > 0 && (!first_active_kf || !points)))
        return MYSLAM_ERR_INVALID;
    std::vector<double> oldp(active_poses, active_poses + (size_t)7 * n_active), newp((size_t)7 * n_active);
    const auto load_unit = [](const double* p) { Se3 T = pg_load(p); pg_qnorm(T.q); return T; };
    const Se3 Tc_inv = pg_inv(load_unit(active_poses + 7 * cur)), Tcc = load_unit(corrected_cur_pose7);
    for (int a = 0; a < n_active; a++)
        pg_store((a == cur) ? Tcc : pg_mul(pg_mul(load_unit(active_poses + 7 * a), Tc_inv), Tcc), newp.data() + 7 * a);       // :480-482
    if (n_points > 0) {
        int rc = myslam_correct_map_points(oldp.data(), newp.data(), n_active, first_active_kf, points, n_points);     // :486-502
        if (rc) return rc;
    }
    for (size_t k = 0; k < newp.size(); k++) active_poses[k] = newp[k];                                       // :505-507
    return MYSLAM_OK;
}

int myslam_correct_map_points_device(const double* d_old_poses, const double* d_new_poses, int n_poses, const int32_t* d_first_kf,
                                     double* d_points, int n_points, int32_t* d_status, void* hip_stream) {
    if (n_points < 0 || n_poses < 0 || (n_points > 0 && (!d_old_poses || !d_new_poses || !d_first_kf || !d_points || !d_status))) return MYSLAM_ERR_INVALID;
    if (n_points == 0) return MYSLAM_OK;
    hipLaunchKernelGGL(k_correct_map_points, dim3((n_points + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, d_old_poses, d_new_poses, n_poses,
                       d_first_kf, d_points, n_points, d_status);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_correct_map_points(const double* old_poses, const double* new_poses, int n_poses, const int32_t* first_kf, double* points, int n_points) {
    if (n_points < 0 || n_poses < 0 || (n_points > 0 && (!old_poses || !new_poses || !first_kf || !points))) return MYSLAM_ERR_INVALID;
    if (n_points == 0) return MYSLAM_OK;
    if (need_device()) return MYSLAM_ERR_HIP;
    HostCall hc;
    int32_t stt = 0;                                       // goes up as 0 and comes back as the kernel's verdict
    const int i_o = hc.in(old_poses, (size_t)7 * n_poses), i_n = hc.in(new_poses, (size_t)7 * n_poses), i_k = hc.in(first_kf, (size_t)n_points);
    const int io_p = hc.inout(points, (size_t)3 * n_points, false), io_s = hc.inout(&stt, 1);
    int rc;
    if ((rc = hc.upload()) ||
        (rc = myslam_correct_map_points_device(hc.dev<double>(i_o), hc.dev<double>(i_n), n_poses, hc.dev<int32_t>(i_k), hc.dev<double>(io_p), n_points,
                                               hc.dev<int32_t>(io_s), hc.stream())) ||
        (rc = hc.download()))
        return rc;
    if (stt != 0) return stt;                              // the caller's points stay as they were
    memcpy(points, hc.host<double>(io_p), sizeof(double) * 3 * n_points);
    return MYSLAM_OK;
}

}  // extern "C"
