// loop_correct.hip — LoopClosing::LoopCorrect (src/loopclosing.cpp:437-463) for a batch of maps in one enqueue on gfx950:
// the loop edge of :328-330, the need-correct test of :284-289, LoopLocalFusion's arithmetic (:470-507), PoseGraphOptimization
// (:537-610) and its write-back (:612-641).  Device pointers in, device pointers out, nothing read back: the Levenberg control flow that
// myslam_pose_graph_optimize runs on the host (pgo.hip) runs here on the device.
//
// One workgroup of 256 threads owns one map from its gate to its status, so no workgroup ever waits on another: every phase below is
// separated from the next by a workgroup barrier, every loop is bounded by a count of the item (key-frames, edges, points, separators),
// by max_iters or by Levenberg's ten trials.  All sums run in a fixed order (per-thread strided partial sums, then a tree), so an
// item's bytes depend on the item alone.
//
//   check      counts against the caps, every index against its count, cur in the active list                        -> ERR_INVALID / ERR_CAPACITY
//   edge, gate one thread: append (cur, loop, Tcc Tloop^-1), |log(Tcur Tcc^-1)| against the threshold                    -> NOT_NEEDED
//   fusion     one thread per active key-frame / per active point
//   structure  fixed = active + loop + row 0.  Free key-frames in row order form the chain; an edge whose two free endpoints are not
//              neighbours in that order makes its LATER endpoint a separator (lc_separator: no greedy pass, one thread per edge).
//              What remains of the chain is block tridiagonal: two remaining free key-frames joined by an edge were neighbours
//              before the separators left, and still are.  More than MYSLAM_LOOP_CORRECT_MAX_SEPARATORS                 -> FUSED_ONLY
//   adjacency  per key-frame the list of (edge, side) in edge order: the assembly sums in that order
//   per iteration: linearize (pg_shared.h's numeric Jacobian, one thread per (edge, side, coordinate)), assemble (one wave per key-frame:
//              its diagonal block and right-hand side, then every off-diagonal block it owns), and per Levenberg trial:
//              sweep (pg_sweep: one lane per right-hand-side column, 6 S + 1 <= 193 columns in the 256 threads), Z^T Z with
//              v_mfma_f64_16x16x4 one wave per 16x16 tile subtracted from Hss + lambda I, dense Cholesky with the right-hand side as the
//              last row, back substitution, y = z - Z xS, pg_back in wave 0, pose update, chi2, and the accept / reject rules.
//   write-back non-active points from the fused to the optimised pose of their first key-frame, the free key-frames' poses.
#include "common.h"
#include "pg_shared.h"

namespace myslam_hip {

constexpr int LC_THREADS = 256;
constexpr int LC_MAXS = MYSLAM_LOOP_CORRECT_MAX_SEPARATORS;
constexpr int LC_LDZ = ((6 * LC_MAXS + 1 + 15) / 16) * 16;       // columns of [C | bT], padded to whole 16x16 tiles
static_assert(LC_LDZ <= LC_THREADS, "the sweep runs one lane per right-hand-side column inside one workgroup");

// The separator rule.  fa, fb: positions of an edge's endpoints va, vb among the FREE key-frames in row order (-1 = fixed).
// Returns the key-frame that becomes a separator, or -1 when the edge stays in the block-tridiagonal chain.
__host__ __device__ inline int lc_separator(int fa, int fb, int va, int vb) {
    if (fa < 0 || fb < 0) return -1;
    const int d = fa > fb ? fa - fb : fb - fa;
    if (d <= 1) return -1;
    return fa > fb ? va : vb;
}

// per-item scratch, carved out of the handle's two blocks (offsets in elements)
struct LcLayout {
    size_t dstride, istride;
    size_t P, Pf, Ps, oldA, minv, J, err, D, B, C, Z, Lw, Hss, bS, A, xT, y;      // doubles
    size_t fx, fpos, inS, slot, adjOff, adj;                                       // int32
};

struct LcArgs {
    double* poses; const int32_t* n_kf; const int32_t* active; const int32_t* n_active; const int32_t* cur; const int32_t* loop;
    const double* corrected; const int32_t* verify_status; int32_t* e0; int32_t* e1; double* meas; int32_t* n_edges;
    double* points; const int32_t* n_points; const int32_t* first_active; const int32_t* first_kf;
    double correct_threshold; int max_iters; double* chi2; int32_t* iters; int32_t* status;
    int kf_cap, edge_cap, active_cap, point_cap;
    double* dscratch; int32_t* iscratch; LcLayout lay;
};

__device__ __forceinline__ Se3 lc_load_unit(const double* p) { Se3 T = pg_load(p); pg_qnorm(T.q); return T; }

__device__ __forceinline__ double lc_chi2(const double* P, const double* minv, const int32_t* e0, const int32_t* e1, int E, double* sm) {
    double c = 0;
    for (int k = threadIdx.x; k < E; k += LC_THREADS)
        c += pg_edge_chi2(P, minv, e0, e1, k);
    return pg_block_reduce<LC_THREADS>(c, sm, 0);
}

typedef double lc_d4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(LC_THREADS) k_loop_correct(const LcArgs a) {
    __shared__ double sRed[LC_THREADS];
    __shared__ double sInv[6 * LC_MAXS], sY[6 * LC_MAXS], sX[6 * LC_MAXS];
    __shared__ int sErr, sCurSlot, sNT, sNS, sBad;
    __shared__ double sGate;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    constexpr int NW = LC_THREADS / 64;

    // ---- 1. gate on the verification's verdict ----
    if (a.verify_status && a.verify_status[b] != MYSLAM_VERIFY_CONFIRMED) {
        if (tid == 0) { a.status[b] = MYSLAM_LOOP_CORRECT_SKIPPED; a.chi2[b] = 0; a.iters[b] = 0; }
        return;
    }
    const int n = a.n_kf[b], na = a.n_active[b], E = a.n_edges[b], np = a.n_points[b], cur = a.cur[b], loop = a.loop[b];
    double* const poses = a.poses + (size_t)b * a.kf_cap * 7;
    const int32_t* const active = a.active + (size_t)b * a.active_cap;
    int32_t* const e0 = a.e0 + (size_t)b * a.edge_cap;
    int32_t* const e1 = a.e1 + (size_t)b * a.edge_cap;
    double* const meas = a.meas + (size_t)b * a.edge_cap * 7;
    double* const points = a.points + (size_t)b * a.point_cap * 3;
    const int32_t* const first_active = a.first_active + (size_t)b * a.point_cap;
    const int32_t* const first_kf = a.first_kf + (size_t)b * a.point_cap;

    // ---- checks: nothing of the item is written before they have all passed ----
    if (tid == 0) { sErr = 0; sCurSlot = -1; sBad = 0; }
    __syncthreads();
    const bool counts_ok = n >= 1 && n <= a.kf_cap && na >= 1 && na <= a.active_cap && E >= 0 && E <= a.edge_cap && np >= 0 && np <= a.point_cap &&
                           cur >= 0 && cur < n && loop >= 0 && loop < n && cur != loop;       // (cur, cur) would be a self edge, refused as myslam_pose_graph_optimize refuses it
    if (counts_ok) {
        bool bad = false;
        for (int i = tid; i < na; i += LC_THREADS) {
            const int v = active[i];
            if (v < 0 || v >= n || (i > 0 && active[i - 1] >= v)) bad = true;
            if (v == cur) sCurSlot = i;
        }
        for (int k = tid; k < E; k += LC_THREADS) {
            const int v0 = e0[k], v1 = e1[k];
            if (v0 < 0 || v0 >= n || v1 < 0 || v1 >= n || v0 == v1) bad = true;
        }
        for (int i = tid; i < np; i += LC_THREADS)
            if (first_active[i] >= na || first_kf[i] >= n) bad = true;
        if (bad) sErr = MYSLAM_ERR_INVALID;
    }
    __syncthreads();
    {
        int err = sErr;
        if (!counts_ok || sCurSlot < 0) err = MYSLAM_ERR_INVALID;
        else if (err == 0 && E >= a.edge_cap) err = MYSLAM_ERR_CAPACITY;
        if (err) {
            if (tid == 0) { a.status[b] = err; a.chi2[b] = 0; a.iters[b] = 0; }
            return;
        }
    }
    const LcLayout& L = a.lay;
    double* const ds = a.dscratch + (size_t)b * L.dstride;
    int32_t* const is = a.iscratch + (size_t)b * L.istride;
    double *P = ds + L.P, *Pf = ds + L.Pf, *Ps = ds + L.Ps, *oldA = ds + L.oldA, *minv = ds + L.minv, *J = ds + L.J, *err = ds + L.err, *D = ds + L.D,
           *B = ds + L.B, *C = ds + L.C, *Z = ds + L.Z, *Lw = ds + L.Lw, *Hss = ds + L.Hss, *bS = ds + L.bS, *A = ds + L.A, *xT = ds + L.xT, *yv = ds + L.y;
    int32_t *fx = is + L.fx, *fpos = is + L.fpos, *inS = is + L.inS, *slot = is + L.slot, *adjOff = is + L.adjOff, *adj = is + L.adj;

    // ---- 2. the loop edge (:328-330) and 3. the need-correct test (:284-289) ----
    const Se3 Tcc = lc_load_unit(a.corrected + 7 * b);
    if (tid == 0) {
        const Se3 Tloop = lc_load_unit(poses + 7 * loop), Tcur = lc_load_unit(poses + 7 * cur);
        pg_store(pg_mul(Tcc, pg_inv(Tloop)), meas + 7 * E);
        e0[E] = cur; e1[E] = loop;
        a.n_edges[b] = E + 1;
        double d[6], s = 0;
        pg_log(pg_mul(Tcur, pg_inv(Tcc)), d);
        for (int k = 0; k < 6; k++) s += d[k] * d[k];
        sGate = sqrt(s);
    }
    __syncthreads();
    if (!(sGate > a.correct_threshold)) {
        if (tid == 0) { a.status[b] = MYSLAM_LOOP_CORRECT_NOT_NEEDED; a.chi2[b] = 0; a.iters[b] = 0; }
        return;
    }
    const int E1 = E + 1;

    // ---- 4. LoopLocalFusion (:470-507) ----
    for (int v = tid; v < n; v += LC_THREADS) { pg_store(lc_load_unit(poses + 7 * v), P + 7 * v); fx[v] = 0; inS[v] = 0; }
    __syncthreads();
    {
        const Se3 Tc_inv = pg_inv(pg_load(P + 7 * cur));
        for (int i = tid; i < na; i += LC_THREADS) {
            const int v = active[i];
            const Se3 To = pg_load(P + 7 * v);
            pg_store(To, oldA + 7 * i);
            const Se3 Tn = (v == cur) ? Tcc : pg_mul(pg_mul(To, Tc_inv), Tcc);       // :480-482
            pg_store(Tn, poses + 7 * v);                                              // :505-507
            fx[v] = 1;
        }
    }
    __syncthreads();
    for (int i = tid; i < na; i += LC_THREADS) pg_store(pg_load(poses + 7 * active[i]), P + 7 * active[i]);
    for (int i = tid; i < np; i += LC_THREADS) {
        const int fa = first_active[i];
        if (fa >= 0) pg_move_point(pg_load(oldA + 7 * fa), pg_load(poses + 7 * active[fa]), points + 3 * i);      // :486-502
    }
    if (tid == 0) { fx[loop] = 1; fx[0] = 1; }
    __syncthreads();
    for (int v = tid; v < n; v += LC_THREADS) pg_store(pg_load(P + 7 * v), Pf + 7 * v);

    // ---- structure: chain, separators, adjacency ----
    if (tid == 0) {
        int f = 0;
        for (int v = 0; v < n; v++) fpos[v] = fx[v] ? -1 : f++;
    }
    __syncthreads();
    for (int k = tid; k < E1; k += LC_THREADS) {
        const int s = lc_separator(fpos[e0[k]], fpos[e1[k]], e0[k], e1[k]);
        if (s >= 0) inS[s] = 1;
    }
    for (int v = tid; v < n; v += LC_THREADS) {           // degree, kept in slot[] until the prefix sum
        int d = 0;
        for (int k = 0; k < E1; k++) d += (e0[k] == v) + (e1[k] == v);
        slot[v] = d;
    }
    __syncthreads();
    if (tid == 0) {
        int t = 0, s = 0, o = 0;
        for (int v = 0; v < n; v++) {
            adjOff[v] = o; o += slot[v];
            slot[v] = fx[v] ? -1 : (inS[v] ? -2 - s++ : t++);       // chain position, or -2 - separator index for now
        }
        adjOff[n] = o;
        sNT = t; sNS = s;
    }
    __syncthreads();
    const int nT = sNT, nS = sNS;
    if (nS > LC_MAXS) {                                    // the caller finishes with myslam_pose_graph_optimize + myslam_correct_map_points
        if (tid == 0) { a.status[b] = MYSLAM_LOOP_CORRECT_FUSED_ONLY; a.chi2[b] = 0; a.iters[b] = 0; }
        return;
    }
    const int nF = nT + nS, mS = 6 * nS, ldz = ((mS + 1 + 15) / 16) * 16, rows = 6 * nT;
    for (int v = tid; v < n; v += LC_THREADS) {
        if (slot[v] <= -2) slot[v] = nT + (-2 - slot[v]);                              // slot: -1 fixed, t, or nT + s
        int o = adjOff[v];
        for (int k = 0; k < E1; k++) {
            if (e0[k] == v) adj[o++] = 2 * k;
            if (e1[k] == v) adj[o++] = 2 * k + 1;
        }
    }
    for (int k = tid; k < E1; k += LC_THREADS) pg_store(pg_inv(lc_load_unit(meas + 7 * k)), minv + 7 * k);
    // blocks the assembly never writes stay zero for the whole run (the sparsity pattern is fixed)
    for (int i = tid; i < 36 * nT; i += LC_THREADS) { D[i] = 0; B[i] = 0; }
    for (size_t i = tid; i < (size_t)rows * ldz; i += LC_THREADS) C[i] = 0;
    for (int i = tid; i < ldz * ldz; i += LC_THREADS) Hss[i] = 0;
    for (int i = tid; i < ldz; i += LC_THREADS) bS[i] = 0;
    for (int i = tid; i < rows; i += LC_THREADS) xT[i] = 0;
    if (tid < 6 * LC_MAXS) sX[tid] = 0;
    __syncthreads();

    // ---- 5. PoseGraphOptimization (:537-610): g2o's Levenberg over the rules of myslam_pose_graph_optimize ----
    int it = 0;
    double currentChi = lc_chi2(P, minv, e0, e1, E1, sRed);
    if (nF > 0) {
        double lambda = 0, ni = 2;
        for (; it < a.max_iters; it++) {
            // linearize: one thread per (edge, side, tangent coordinate), central differences with delta 1e-9
            for (int id = tid; id < 12 * E1; id += LC_THREADS) pg_jacobian_column(id, P, minv, e0, e1, fx, J, err);
            __syncthreads();
            // assemble: one wave per free key-frame; lanes 0..35 one entry of a 6x6 block, lanes 36..41 one entry of the right-hand side
            for (int v = wv; v < n; v += NW) {
                const int sl = slot[v];
                if (sl < 0 || lane >= 42) continue;
                const bool isb = lane >= 36, vT = sl < nT;
                const int r = isb ? lane - 36 : lane / 6, c = isb ? 0 : lane - 6 * r;
                const int a0 = adjOff[v], a1 = adjOff[v + 1];
                double sum = 0;
                for (int p = a0; p < a1; p++) {
                    const int k = adj[p] >> 1, side = adj[p] & 1;
                    const double* Jr = J + ((size_t)k * 2 + side) * 36;
                    double h;
                    if (!isb) h = pg_jtj(Jr, Jr, r, c);
                    else h = pg_jte(Jr, err + (size_t)k * 6, r);
                    sum += h;
                }
                if (vT) {
                    if (isb) C[(size_t)(6 * sl + r) * ldz + mS] = -sum;
                    else D[(size_t)sl * 36 + r * 6 + c] = sum;
                } else {
                    const int s = sl - nT;
                    if (isb) bS[6 * s + r] = -sum;
                    else Hss[(size_t)(6 * s + r) * ldz + 6 * s + c] = sum;
                }
                if (isb) continue;
                // off-diagonal blocks whose ROWS are this key-frame's: the later of two chain key-frames, the chain key-frame of a
                // chain-separator pair, the later separator of two.  Parallel edges to one neighbour sum into one block, in edge order.
                for (int p = a0; p < a1; p++) {
                    const int k = adj[p] >> 1, side = adj[p] & 1, u = side ? e0[k] : e1[k], su = slot[u];
                    if (su < 0) continue;
                    const bool uT = su < nT;
                    if (vT ? (uT && su > sl) : (uT || su > sl)) continue;
                    bool first = true;
                    for (int q = a0; q < p; q++) { const int kq = adj[q] >> 1; if (((adj[q] & 1) ? e0[kq] : e1[kq]) == u) first = false; }
                    if (!first) continue;
                    double s2 = 0;
                    for (int q = p; q < a1; q++) {
                        const int kq = adj[q] >> 1, sq = adj[q] & 1;
                        if ((sq ? e0[kq] : e1[kq]) != u) continue;
                        const double* Jr = J + ((size_t)kq * 2 + sq) * 36;
                        const double* Jc = J + ((size_t)kq * 2 + (1 - sq)) * 36;
                        // pg_jtj(Jr, Jc, r, c), written out: behind the call, in whatever form, this kernel's register allocation tips over
                        // (SGPR spills 210 -> 221, +440 instructions) and a batch runs 2.3 % longer (measured)
                        double h = 0;
                        for (int m = 0; m < 6; m++) h += Jr[m * 6 + r] * Jc[m * 6 + c];
                        s2 += h;
                    }
                    if (vT && uT) B[(size_t)sl * 36 + r * 6 + c] = s2;                                   // su == sl - 1 by the separator rule
                    else if (vT) C[(size_t)(6 * sl + r) * ldz + 6 * (su - nT) + c] = s2;
                    else Hss[(size_t)(6 * (sl - nT) + r) * ldz + 6 * (su - nT) + c] = s2;
                }
            }
            __syncthreads();
            if (it == 0) {                                 // computeLambdaInit: tau * max diagonal
                double mx = 0;
                for (int i = tid; i < 6 * nF; i += LC_THREADS) {
                    const int f = i / 6, q = i - 6 * f;
                    mx = fmax(mx, fabs(f < nT ? D[(size_t)f * 36 + 7 * q] : Hss[(size_t)(6 * (f - nT) + q) * ldz + 6 * (f - nT) + q]));
                }
                lambda = 1e-5 * pg_block_reduce<LC_THREADS>(mx, sRed, 1); ni = 2;
            }
            double rho = 0;
            int qmax = 0;
            do {
                for (int i = tid; i < 7 * n; i += LC_THREADS) Ps[i] = P[i];
                if (tid == 0) sBad = 0;
                __syncthreads();
                // forward sweep down the chain, one lane per column of [C | bT]
                if (nT > 0 && pg_sweep(D, B, C, Z, Lw, 0, nT, ldz, lambda, tid) && tid == 0) sBad = 1;
                __syncthreads();
                // A = Hss + lambda I - Z^T Z (lower), its last row bS - Z^T z: one wave per 16x16 tile
                if (mS > 0) {
                    const int nt = ldz >> 4, ntile = nt * (nt + 1) / 2, k4 = (rows + 3) >> 2;
                    for (int tile = wv; tile < ntile; tile += NW) {
                        int ti, tj;
                        pg_tri_decode(tile, ti, tj);
                        lc_d4 acc = {0, 0, 0, 0};
                        const int zr = lane >> 4, zc = lane & 15;
                        for (int g = 0; g < k4; g++) {
                            const int row = 4 * g + zr;
                            const double av = row < rows ? Z[(size_t)row * ldz + 16 * ti + zc] : 0.0;
                            const double bv = row < rows ? Z[(size_t)row * ldz + 16 * tj + zc] : 0.0;
                            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
                        }
#pragma unroll
                        for (int v = 0; v < 4; v++) {
                            const int i = 16 * ti + 4 * v + zr, j = 16 * tj + zc;
                            double val = 0;
                            if (pg_schur_kept(i, j, mS)) val = pg_schur_entry(Hss, bS, i, j, mS, ldz, lambda) - acc[v];
                            A[(size_t)i * ldz + j] = val;
                        }
                    }
                    __syncthreads();
                    // right-looking Cholesky; the right-hand side rides along as row mS, so the factorisation leaves L^-1 rhs there
                    for (int j = 0; j < mS; j++) {
                        double piv = A[(size_t)j * ldz + j];
                        if (!(piv > 0)) { if (tid == 0) sBad = 1; piv = 1.0; }
                        const double inv = 1.0 / sqrt(piv);
                        if (tid == 0) sInv[j] = inv;
                        for (int i = j + 1 + tid; i <= mS; i += LC_THREADS) A[(size_t)i * ldz + j] *= inv;
                        __syncthreads();
                        const int w = mS - 1 - j, cnt = w * (mS - j);
                        for (int idx = tid; idx < cnt; idx += LC_THREADS) {
                            const int di = idx / w, i = j + 1 + di, k = j + 1 + (idx - di * w);
                            if (k <= i) A[(size_t)i * ldz + k] -= A[(size_t)i * ldz + j] * A[(size_t)k * ldz + j];
                        }
                        __syncthreads();
                    }
                    // L^T xS = y
                    for (int k = tid; k < mS; k += LC_THREADS) sY[k] = A[(size_t)mS * ldz + k];
                    for (int j = mS - 1; j >= 0; j--) {
                        __syncthreads();
                        const double xj = sY[j] * sInv[j];
                        for (int k = tid; k < j; k += LC_THREADS) sY[k] -= A[(size_t)j * ldz + k] * xj;
                        if (tid == 0) sX[j] = xj;
                    }
                    __syncthreads();
                }
                if (nT > 0) {
                    for (int r = tid; r < rows; r += LC_THREADS) {
                        const double* zr = Z + (size_t)r * ldz;
                        double s = zr[mS];
                        for (int j = 0; j < mS; j++) s -= zr[j] * sX[j];
                        yv[r] = s;
                    }
                    __syncthreads();
                    if (wv == 0) pg_back(Lw, yv, xT, 0, nT, lane);
                    __syncthreads();
                }
                // pose <- exp(x) * pose for every free key-frame; the gain's denominator x . (lambda x + b)
                double sc = 0;
                for (int v = tid; v < n; v += LC_THREADS) {
                    const int sl = slot[v];
                    if (sl < 0) continue;
                    sc += pg_update_pose(P + 7 * v, sl, nT, xT, sX, C, bS, ldz, mS, lambda);
                }
                const double den = pg_block_reduce<LC_THREADS>(sc, sRed, 0);
                const double newChi = lc_chi2(P, minv, e0, e1, E1, sRed);
                const bool ok = !sBad;
                const double tempChi = ok ? newChi : 1e300;
                rho = currentChi - tempChi;
                double scale = 1e-3;
                if (ok) scale += den;
                rho /= scale;
                if (rho > 0 && isfinite(tempChi) && ok) {
                    const double t = 2 * rho - 1;                     // myslam_pose_graph_optimize (pgo.hip) writes pow(2 * rho - 1, 3): kept apart, the two need not round alike
                    double alpha = 1. - t * t * t;
                    alpha = fmin(alpha, 2. / 3.);
                    lambda *= fmax(1. / 3., alpha); ni = 2; currentChi = tempChi;
                } else {
                    lambda *= ni; ni *= 2;
                    __syncthreads();
                    for (int i = tid; i < 7 * n; i += LC_THREADS) P[i] = Ps[i];
                    __syncthreads();
                    if (!isfinite(lambda)) break;
                }
                qmax++;
            } while (rho < 0 && qmax < 10);
            if (qmax == 10 || rho == 0 || !isfinite(lambda)) { it++; break; }
        }
    }
    __syncthreads();

    // ---- 6. write-back (:612-641): non-active points move with their first key-frame, then the optimised poses ----
    for (int i = tid; i < np; i += LC_THREADS) {
        const int k = first_kf[i];
        if (first_active[i] >= 0 || k < 0) continue;                                   // :616-619, :627-631
        pg_move_point(pg_load(Pf + 7 * k), pg_load(P + 7 * k), points + 3 * i);
    }
    for (int v = tid; v < n; v += LC_THREADS)
        if (slot[v] >= 0) pg_store(pg_load(P + 7 * v), poses + 7 * v);
    if (tid == 0) { a.status[b] = MYSLAM_LOOP_CORRECT_DONE; a.chi2[b] = currentChi; a.iters[b] = it; }
}

}  // namespace myslam_hip

using namespace myslam_hip;

struct myslam_loop_corrector {
    int max_batch = 0, kf_cap = 0, edge_cap = 0, active_cap = 0, point_cap = 0;
    hipStream_t stream = nullptr;
    Buf<double> d_scratch;
    Buf<int32_t> i_scratch;
    LcLayout lay{};
};

extern "C" {

int myslam_loop_corrector_destroy(myslam_loop_corrector* h) {
    if (!h) return MYSLAM_ERR_INVALID;
    (void)hipStreamSynchronize(h->stream);
    delete h;
    return MYSLAM_OK;
}

int myslam_loop_corrector_create(myslam_loop_corrector** out, int max_batch, int kf_cap, int edge_cap, int active_cap, int point_cap) {
    if (!out || max_batch < 1 || max_batch > 65535 || kf_cap < 1 || edge_cap < 1 || active_cap < 1 || active_cap > kf_cap || point_cap < 0)
        return MYSLAM_ERR_INVALID;
    if (kf_cap > (1 << 20) || edge_cap > (1 << 20)) return MYSLAM_ERR_CAPACITY;
    if (need_device()) return MYSLAM_ERR_HIP;
    myslam_loop_corrector* h = new myslam_loop_corrector();
    h->max_batch = max_batch; h->kf_cap = kf_cap; h->edge_cap = edge_cap; h->active_cap = active_cap; h->point_cap = point_cap;
    const size_t n = (size_t)kf_cap, E = (size_t)edge_cap;
    LcLayout& L = h->lay;
    size_t o = 0;
    auto take = [&o](size_t count) { const size_t at = o; o += (count + 1) & ~(size_t)1; return at; };
    L.P = take(7 * n); L.Pf = take(7 * n); L.Ps = take(7 * n); L.oldA = take(7 * (size_t)active_cap); L.minv = take(7 * E); L.J = take(72 * E);
    L.err = take(6 * E); L.D = take(36 * n); L.B = take(36 * n); L.C = take(6 * n * LC_LDZ); L.Z = take(6 * n * LC_LDZ); L.Lw = take(72 * n);
    L.Hss = take((size_t)LC_LDZ * LC_LDZ); L.bS = take(LC_LDZ); L.A = take((size_t)LC_LDZ * LC_LDZ); L.xT = take(6 * n); L.y = take(6 * n);
    L.dstride = o;
    o = 0;
    L.fx = take(n); L.fpos = take(n); L.inS = take(n); L.slot = take(n); L.adjOff = take(n + 1); L.adj = take(2 * E);
    L.istride = o;
    int rc;
    if ((rc = h->d_scratch.renew(L.dstride * (size_t)max_batch, MYSLAM_ERR_CAPACITY)) ||
        (rc = h->i_scratch.renew(L.istride * (size_t)max_batch, MYSLAM_ERR_CAPACITY))) {
        delete h;
        return rc;
    }
    *out = h;
    return MYSLAM_OK;
}

int myslam_loop_corrector_set_stream(myslam_loop_corrector* h, void* hip_stream) {
    if (!h) return MYSLAM_ERR_INVALID;
    h->stream = (hipStream_t)hip_stream;
    return MYSLAM_OK;
}

int myslam_loop_correct_batch(myslam_loop_corrector* h, double* d_poses, const int32_t* d_n_kf, const int32_t* d_active, const int32_t* d_n_active,
                              const int32_t* d_cur, const int32_t* d_loop, const double* d_corrected_pose7, const int32_t* d_verify_status,
                              int32_t* d_edge_v0, int32_t* d_edge_v1, double* d_meas, int32_t* d_n_edges, double* d_points, const int32_t* d_n_points,
                              const int32_t* d_first_active, const int32_t* d_first_kf, int batch, double correct_threshold, int max_iters,
                              double* d_chi2, int32_t* d_iters, int32_t* d_status) {
    if (!h || batch < 0 || max_iters < 0 || !(correct_threshold >= 0)) return MYSLAM_ERR_INVALID;
    if (batch > h->max_batch) return MYSLAM_ERR_CAPACITY;
    if (batch == 0) return MYSLAM_OK;
    if (!d_poses || !d_n_kf || !d_active || !d_n_active || !d_cur || !d_loop || !d_corrected_pose7 || !d_edge_v0 || !d_edge_v1 || !d_meas || !d_n_edges ||
        !d_n_points || !d_chi2 || !d_iters || !d_status || (h->point_cap > 0 && (!d_points || !d_first_active || !d_first_kf)))
        return MYSLAM_ERR_INVALID;
    LcArgs a;
    a.poses = d_poses; a.n_kf = d_n_kf; a.active = d_active; a.n_active = d_n_active; a.cur = d_cur; a.loop = d_loop; a.corrected = d_corrected_pose7;
    a.verify_status = d_verify_status; a.e0 = d_edge_v0; a.e1 = d_edge_v1; a.meas = d_meas; a.n_edges = d_n_edges; a.points = d_points;
    a.n_points = d_n_points; a.first_active = d_first_active; a.first_kf = d_first_kf; a.correct_threshold = correct_threshold; a.max_iters = max_iters;
    a.chi2 = d_chi2; a.iters = d_iters; a.status = d_status; a.kf_cap = h->kf_cap; a.edge_cap = h->edge_cap; a.active_cap = h->active_cap;
    a.point_cap = h->point_cap; a.dscratch = h->d_scratch; a.iscratch = h->i_scratch; a.lay = h->lay;
    hipLaunchKernelGGL(k_loop_correct, dim3(batch), dim3(LC_THREADS), 0, h->stream, a);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int myslam_loop_correct_structure(int n_kf, const int32_t* active, int n_active, int loop, const int32_t* edge_v0, const int32_t* edge_v1, int n_edges,
                                  int* n_separators, int* chain_length, int* supported) {
    if (n_kf < 1 || n_active < 0 || n_edges < 0 || loop < 0 || loop >= n_kf || (n_active > 0 && !active) || (n_edges > 0 && (!edge_v0 || !edge_v1)))
        return MYSLAM_ERR_INVALID;
    std::vector<int> fpos(n_kf, 0);
    std::vector<char> inS(n_kf, 0);
    for (int i = 0; i < n_active; i++) {
        if (active[i] < 0 || active[i] >= n_kf) return MYSLAM_ERR_INVALID;
        fpos[active[i]] = -1;
    }
    fpos[loop] = -1; fpos[0] = -1;
    int f = 0;
    for (int v = 0; v < n_kf; v++) if (fpos[v] == 0) fpos[v] = f++;
    for (int k = 0; k < n_edges; k++) {
        const int v0 = edge_v0[k], v1 = edge_v1[k];
        if (v0 < 0 || v0 >= n_kf || v1 < 0 || v1 >= n_kf || v0 == v1) return MYSLAM_ERR_INVALID;
        const int s = lc_separator(fpos[v0], fpos[v1], v0, v1);
        if (s >= 0) inS[s] = 1;
    }
    int nS = 0;
    for (int v = 0; v < n_kf; v++) nS += inS[v];
    if (n_separators) *n_separators = nS;
    if (chain_length) *chain_length = f - nS;
    if (supported) *supported = nS <= LC_MAXS ? 1 : 0;
    return MYSLAM_OK;
}

}  // extern "C"
