// pg_shared.h — every rule the two pose-graph solvers have in common, once.  pgo.hip runs them as kernels per phase driven by the host,
// loop_correct.hip inside one workgroup with barriers; what this header owns is the same lines in both:
//   SE3 exp / log on unit quaternions (the products and the pose layout: se3_quat.h, shared with the host) and the edge error of g2o_types.h:161-167
//   pg_jacobian_column    g2o's numeric Jacobian column of one (edge, side, coordinate)
//   pg_edge_chi2          e^T e of one edge
//   pg_jtj / pg_jte       the 6-term products of the assembly
//   pg_sweep / pg_back    the two serial halves of the block-tridiagonal elimination (forward sweep, backward chain)
//   pg_tri_decode         lower-triangle tile number -> (row tile, column tile)
//   pg_schur_kept, _entry Hss + lambda I | bS, the dense Schur system before Z^T Z comes off
//   pg_update_pose        pose <- exp(x) pose and the gain term x . (lambda x + b)
//   pg_move_point         p <- Tn^-1 (To p), the rigid move of a map point
//   pg_block_reduce       fixed-order sum / maximum of one value per thread
// Left apart on purpose: the dense factorisation (blocked MFMA Cholesky in k_pg_schur, unblocked in k_loop_correct), the separator rule (greedy on
// the host, lc_separator on the device) and Levenberg's accept / reject arithmetic (pow on the host, t*t*t on the device: they need not round alike).
// gfx950 only.
#pragma once
#include <math.h>

#include "common.h"
#include "se3_quat.h"

namespace myslam_hip {

constexpr double PG_EPS = 1e-10;     // Sophus::Constants<double>::epsilon()

// Sophus SE3::exp, tangent (upsilon, omega)
__device__ inline Se3 pg_exp(const double* d) {
    Se3 r;
    const double wx = d[3], wy = d[4], wz = d[5];
    const double th2 = wx * wx + wy * wy + wz * wz;
    double imag, real, B, C;
    if (th2 < PG_EPS * PG_EPS) {
        const double th4 = th2 * th2;
        imag = 0.5 - th2 / 48.0 + th4 / 3840.0;
        real = 1.0 - th2 / 8.0 + th4 / 384.0;
        B = 0.5; C = 1.0 / 6.0;
    } else {
        const double th = sqrt(th2), h = 0.5 * th;
        imag = sin(h) / th;
        real = cos(h);
        B = (1.0 - cos(th)) / th2; C = (th - sin(th)) / (th2 * th);
    }
    r.q[0] = imag * wx; r.q[1] = imag * wy; r.q[2] = imag * wz; r.q[3] = real;
    pg_qnorm(r.q);
    const double u[3] = {d[0], d[1], d[2]};
    const double wu[3] = {wy * u[2] - wz * u[1], wz * u[0] - wx * u[2], wx * u[1] - wy * u[0]};
    const double wwu[3] = {wy * wu[2] - wz * wu[1], wz * wu[0] - wx * wu[2], wx * wu[1] - wy * wu[0]};
    for (int k = 0; k < 3; k++) r.t[k] = u[k] + B * wu[k] + C * wwu[k];
    return r;
}

// Sophus SE3::log -> (upsilon, omega)
__device__ inline void pg_log(const Se3& T, double* d) {
    const double n2 = T.q[0] * T.q[0] + T.q[1] * T.q[1] + T.q[2] * T.q[2], w = T.q[3];
    double f;
    if (n2 < PG_EPS * PG_EPS) f = 2.0 / w - 2.0 / 3.0 * n2 / (w * w * w);
    else {
        const double n = sqrt(n2);
        if (fabs(w) < PG_EPS) f = (w > 0 ? M_PI : -M_PI) / n;
        else f = 2.0 * atan(n / w) / n;
    }
    const double wx = f * T.q[0], wy = f * T.q[1], wz = f * T.q[2];
    const double th2 = wx * wx + wy * wy + wz * wz, th = sqrt(th2);
    double C;
    if (th < PG_EPS) C = 1.0 / 12.0;
    else { const double h = 0.5 * th; C = (1.0 - th * cos(h) / (2.0 * sin(h))) / th2; }
    const double* t = T.t;
    const double wt[3] = {wy * t[2] - wz * t[1], wz * t[0] - wx * t[2], wx * t[1] - wy * t[0]};
    const double wwt[3] = {wy * wt[2] - wz * wt[1], wz * wt[0] - wx * wt[2], wx * wt[1] - wy * wt[0]};
    for (int k = 0; k < 3; k++) d[k] = t[k] - 0.5 * wt[k] + C * wwt[k];
    d[3] = wx; d[4] = wy; d[5] = wz;
}

// g2o_types.h:161-167
__device__ __forceinline__ void pg_edge_error(const Se3& Minv, const Se3& v0, const Se3& v1, double* e) {
    pg_log(pg_mul(pg_mul(Minv, v0), pg_inv(v1)), e);
}

// e^T e of edge k
__device__ __forceinline__ double pg_edge_chi2(const double* poses, const double* minv, const int32_t* e0, const int32_t* e1, int k) {
    double e[6], c = 0;
    pg_edge_error(pg_load(minv + 7 * k), pg_load(poses + 7 * e0[k]), pg_load(poses + 7 * e1[k]), e);
    for (int a = 0; a < 6; a++) c += e[a] * e[a];
    return c;
}

// g2o BaseBinaryEdge::linearizeOplus, numeric branch, for id = (12 edge + 6 side + coordinate) < 12 E: column `coordinate` of J[edge][side] (6x6, row
// major) by central differences with delta 1e-9 on the left-multiplied update, zeros when that side's vertex is fixed (fixedv[vertex] != 0, any
// integer type); the id with side = coordinate = 0 also writes the edge's error into err[6 edge ..].
template <typename Fixed>
__device__ __forceinline__ void pg_jacobian_column(int id, const double* poses, const double* minv, const int32_t* e0, const int32_t* e1,
                                                   const Fixed* fixedv, double* J /*E x 2 x 36*/, double* err /*E x 6*/) {
    const int k = id / 12, rem = id - 12 * k, side = rem / 6, d = rem - 6 * side;
    const int vi[2] = {e0[k], e1[k]};
    const Se3 Mi = pg_load(minv + 7 * k);
    const Se3 v0 = pg_load(poses + 7 * vi[0]), v1 = pg_load(poses + 7 * vi[1]);
    if (rem == 0) {
        double e[6]; pg_edge_error(Mi, v0, v1, e);
        for (int a = 0; a < 6; a++) err[6 * k + a] = e[a];
    }
    double* Jc = J + ((size_t)k * 2 + side) * 36;
    if (fixedv[vi[side]]) {
        for (int r = 0; r < 6; r++) Jc[r * 6 + d] = 0.0;
        return;
    }
    double add[6], ep[6], em[6];
#pragma unroll
    for (int a = 0; a < 6; a++) add[a] = (a == d) ? 1e-9 : 0.0;
    Se3 vp = pg_mul(pg_exp(add), side ? v1 : v0);
    pg_edge_error(Mi, side ? v0 : vp, side ? vp : v1, ep);
#pragma unroll
    for (int a = 0; a < 6; a++) add[a] = (a == d) ? -1e-9 : 0.0;
    vp = pg_mul(pg_exp(add), side ? v1 : v0);
    pg_edge_error(Mi, side ? v0 : vp, side ? vp : v1, em);
    const double scalar = 1.0 / (2 * 1e-9);
    for (int r = 0; r < 6; r++) Jc[r * 6 + d] = scalar * (ep[r] - em[r]);
}

// entry (r, c) of Jr^T Jc and entry r of Jr^T e, 6x6 row-major blocks, summed over the six error rows in order
__device__ __forceinline__ double pg_jtj(const double* Jr, const double* Jc, int r, int c) {
    double h = 0;
    for (int m = 0; m < 6; m++) h += Jr[m * 6 + r] * Jc[m * 6 + c];
    return h;
}
__device__ __forceinline__ double pg_jte(const double* Jr, const double* e, int r) {
    double h = 0;
    for (int m = 0; m < 6; m++) h += Jr[m * 6 + r] * e[m];
    return h;
}

// tile q of a lower triangle numbered row by row: q = ti (ti + 1) / 2 + tj, tj <= ti
__device__ __forceinline__ void pg_tri_decode(int q, int& ti, int& tj) {
    ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= q) ti++;
    tj = q - ti * (ti + 1) / 2;
}

// The dense Schur system before Z^T Z comes off: Hss + lambda I in rows < mS, the right-hand side bS as row mS.  Only the lower triangle of the
// columns < mS is kept (pg_schur_kept); every other entry of the padded matrix is 0.
__device__ __forceinline__ bool pg_schur_kept(int i, int j, int mS) { return i <= mS && j <= i && j < mS; }
__device__ __forceinline__ double pg_schur_entry(const double* Hss, const double* bS, int i, int j, int mS, int ldz, double lambda) {
    return i < mS ? Hss[(size_t)i * ldz + j] + (i == j ? lambda : 0.0) : bS[j];
}

// pose <- exp(x) * pose for a free key-frame in slot sl (chain position t < nT: x = xT[6 t ..], b = column mS of C; else separator sl - nT: xS, bS);
// returns its share x . (lambda x + b) of the gain's denominator
__device__ __forceinline__ double pg_update_pose(double* pose, int sl, int nT, const double* xT, const double* xS, const double* C, const double* bS,
                                                 int ldz, int mS, double lambda) {
    double x[6], s = 0;
    for (int q = 0; q < 6; q++) {
        double bq;
        if (sl < nT) { x[q] = xT[6 * sl + q]; bq = C[(size_t)(6 * sl + q) * ldz + mS]; }
        else { x[q] = xS[6 * (sl - nT) + q]; bq = bS[6 * (sl - nT) + q]; }
        s += x[q] * (lambda * x[q] + bq);
    }
    pg_store(pg_mul(pg_exp(x), pg_load(pose)), pose);
    return s;
}

// p <- Tn^-1 (To p): a map point moves rigidly with its key-frame from pose To to pose Tn (src/loopclosing.cpp:486-502, :621-633)
__device__ __forceinline__ void pg_move_point(Se3 To, Se3 Tn, double* p) {
    pg_qnorm(To.q); pg_qnorm(Tn.q);
    Tn = pg_inv(Tn);
    double pc[3], pw[3];
    pg_rot(To.q, p, pc);
    pc[0] += To.t[0]; pc[1] += To.t[1]; pc[2] += To.t[2];
    pg_rot(Tn.q, pc, pw);
    p[0] = pw[0] + Tn.t[0]; p[1] = pw[1] + Tn.t[1]; p[2] = pw[2] + Tn.t[2];
}

// Fixed-order sum (mode 0) or maximum (mode 1) of one value per thread of an NT-thread workgroup (NT a power of two, sm = NT doubles of LDS); every
// thread receives it.  Opens with a barrier, so sm may still be in use by the previous reduction when it is called.
template <int NT>
__device__ __forceinline__ double pg_block_reduce(double v, double* sm, int mode) {
    const int tid = threadIdx.x;
    __syncthreads();
    sm[tid] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) sm[tid] = mode ? fmax(sm[tid], sm[tid + s]) : sm[tid] + sm[tid + s];
        __syncthreads();
    }
    return sm[0];
}

// 1 / sqrt(s) to double precision: v_rsq_f64 seed (~2^-23) + two cubic Newton steps — a fraction of the sqrt + divide sequences,
// and this value sits on the serial dependency chain of the sweep
__device__ __forceinline__ double pg_rsqrt(double s) {
    double y = __builtin_amdgcn_rsq(s);
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const double e = fma(-s * y, y, 1.0);
        y = fma(y * e, fma(0.375, e, 0.5), y);
    }
    return y;
}

// Block Cholesky of Htt + lambda I fused with the forward substitution of the ldz right-hand-side columns (one per lane).
//   W_t = B_t L_{t-1}^-T,  L_t L_t^T = D_t + lambda I - W_t W_t^T,  Z_t = L_t^-1 (C_t - W_t Z_{t-1})
// Lw[t] = { L_t lower 6x6 with the INVERSE diagonal on the diagonal (36), W_t (36) }.
// Columns [col] of the chain steps [t0, t1), one lane per column; no step couples two chain runs (B = 0 at a run's start).  The loads of step t+1 are
// issued before the arithmetic of step t (they do not depend on the chain).  Returns true when a pivot was not positive.
__device__ __forceinline__ bool pg_sweep(const double* __restrict__ D, const double* __restrict__ B, const double* __restrict__ C,
                                         double* __restrict__ Z, double* __restrict__ Lw, int t0, int t1, int ldz, double lambda, int col) {
    const bool act = col < ldz;
    const int cc = act ? col : 0;
    double L[6][6], W[6][6], zp[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        zp[i] = 0;
#pragma unroll
        for (int j = 0; j < 6; j++) { L[i][j] = (i == j) ? 1.0 : 0.0; W[i][j] = 0; }
    }
    // The block data of a step is wave-uniform; loading it through an opaque per-lane zero keeps the prefetch in VGPRs
    // (as scalar loads the 57 doubles do not fit the SGPR file next to the live step and the prefetch degenerates).
    int vzero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));
    double nB[36], nD[21], nr[6];
    auto fetch = [&](int t) {
        const double* Bt = B + (size_t)t * 36 + vzero;
        const double* Dt = D + (size_t)t * 36 + vzero;
#pragma unroll
        for (int i = 0; i < 36; i++) nB[i] = Bt[i];
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) nD[i * (i + 1) / 2 + j] = Dt[i * 6 + j];
#pragma unroll
        for (int i = 0; i < 6; i++) nr[i] = C[(size_t)(6 * t + i) * ldz + cc];
    };
    if (t0 < t1) fetch(t0);
    bool bad = false;
    for (int t = t0; t < t1; t++) {
        double Bt[36], Dt[21], rr[6];
#pragma unroll
        for (int i = 0; i < 36; i++) Bt[i] = nB[i];
#pragma unroll
        for (int i = 0; i < 21; i++) Dt[i] = nD[i];
#pragma unroll
        for (int i = 0; i < 6; i++) rr[i] = nr[i];
        if (t + 1 < t1) fetch(t + 1);
        // W = B L^-T  (L holds 1/diag on its diagonal)
#pragma unroll
        for (int i = 0; i < 6; i++) {
#pragma unroll
            for (int j = 0; j < 6; j++) {
                double s = Bt[i * 6 + j];
#pragma unroll
                for (int k = 0; k < j; k++) s -= W[i][k] * L[j][k];
                W[i][j] = s * L[j][j];
            }
        }
        // A = D + lambda I - W W^T (lower), factor in place into L
#pragma unroll
        for (int i = 0; i < 6; i++) {
#pragma unroll
            for (int j = 0; j <= i; j++) {
                double s = Dt[i * (i + 1) / 2 + j] + ((i == j) ? lambda : 0.0);
#pragma unroll
                for (int k = 0; k < 6; k++) s -= W[i][k] * W[j][k];
                L[i][j] = s;
            }
        }
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double s = L[j][j];
#pragma unroll
            for (int k = 0; k < j; k++) s -= L[j][k] * L[j][k];
            if (!(s > 0)) { bad = true; s = 1.0; }
            const double inv = pg_rsqrt(s);
            L[j][j] = inv;
#pragma unroll
            for (int i = j + 1; i < 6; i++) {
                double v = L[i][j];
#pragma unroll
                for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k];
                L[i][j] = v * inv;
            }
        }
        // this lane's right-hand side
        double z[6];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            double s = rr[i];
#pragma unroll
            for (int k = 0; k < 6; k++) s -= W[i][k] * zp[k];
#pragma unroll
            for (int k = 0; k < i; k++) s -= L[i][k] * z[k];
            z[i] = s * L[i][i];
        }
        if (act) {
#pragma unroll
            for (int i = 0; i < 6; i++) Z[(size_t)(6 * t + i) * ldz + col] = z[i];
        }
#pragma unroll
        for (int i = 0; i < 6; i++) zp[i] = z[i];
        if (col == 0) {
            double* o = Lw + (size_t)t * 72;
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int j = 0; j < 6; j++) { o[i * 6 + j] = (j <= i) ? L[i][j] : 0.0; o[36 + i * 6 + j] = W[i][j]; }
        }
    }
    return bad;
}

// xT_t = L_t^-T (y_t - W_{t+1}^T xT_{t+1}), the backward chain of one segment per workgroup (W = 0 across segment boundaries).
// Six lanes of one wave: lane i owns row i of the step (its row of W_{t+1}^T x and of the back substitution), values exchanged by readlane.
__device__ __forceinline__ void pg_back(const double* __restrict__ Lw, const double* __restrict__ y, double* __restrict__ xT, int t0, int t1, int lane) {
    const int i = lane < 6 ? lane : 5;
    double xn[6] = {0, 0, 0, 0, 0, 0};
    double nLc[6], nWc[6], ny = 0;                 // column i of L_t (rows k), column i of W_{t+1} (rows k), y_t[i]
    auto fetch = [&](int t) {
        const double* L = Lw + (size_t)t * 72;
#pragma unroll
        for (int k = 0; k < 6; k++) nLc[k] = L[k * 6 + i];
        if (t + 1 < t1) {
            const double* Wn = Lw + (size_t)(t + 1) * 72 + 36;
#pragma unroll
            for (int k = 0; k < 6; k++) nWc[k] = Wn[k * 6 + i];
        } else {
#pragma unroll
            for (int k = 0; k < 6; k++) nWc[k] = 0;
        }
        ny = y[6 * t + i];
    };
    if (t0 < t1) fetch(t1 - 1);
    for (int t = t1 - 1; t >= t0; t--) {
        double Lc[6], Wc[6];
#pragma unroll
        for (int k = 0; k < 6; k++) { Lc[k] = nLc[k]; Wc[k] = nWc[k]; }
        double r = ny;
        if (t > t0) fetch(t - 1);
#pragma unroll
        for (int k = 0; k < 6; k++) r -= Wc[k] * xn[k];
        // back substitution L^T x = r: x[5] first; lane i subtracts L[k][i] x[k] for k > i as the x[k] become known
        double x[6];
#pragma unroll
        for (int k = 5; k >= 0; k--) {
            const double mine = r * Lc[k];         // valid in lane k (Lc[k] = L[k][i] = inverse diagonal when i == k)
            const int lo = __builtin_amdgcn_readlane((int)(__double_as_longlong(mine) & 0xffffffffll), k);
            const int hi = __builtin_amdgcn_readlane((int)(__double_as_longlong(mine) >> 32), k);
            x[k] = __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
            if (k > 0) r -= (i < k) ? Lc[k] * x[k] : 0.0;
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 6; k++) xT[6 * t + k] = x[k];
        }
#pragma unroll
        for (int k = 0; k < 6; k++) xn[k] = x[k];
    }
}

}  // namespace myslam_hip
