// tri_solve.h — the solve of triangulation() (reference include/myslam/algorithm.h:16-33) as a device function: the ONE copy that
// match_tri.hip (k_triangulate, the one-pair matcher's tail) and tracker.hip (the key-frame turn, Frontend::TriangulateNewPoints) inline.  Both
// units are built without FMA contraction, so the two give the same bits.
#pragma once

namespace myslam_hip {

// one-sided Jacobi SVD of the 4x4 DLT matrix (f64), fully unrolled pair loop (no runtime register indexing)
__device__ __forceinline__ void tri_solve(const double (&P)[2][12], const double (&pt)[2][2], double* xyz, double& ratio) {
    double A[4][4], V[4][4];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            A[2 * i][c] = pt[i][0] * P[i][8 + c] - P[i][c];            // algorithm.h:23
            A[2 * i + 1][c] = pt[i][1] * P[i][8 + c] - P[i][4 + c];    // algorithm.h:24
        }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) V[i][j] = (i == j) ? 1.0 : 0.0;
    // Per column pair: one sqrt, one division and one reciprocal square root (f64 sqrt / division cost ~25 instructions each on this
    // hardware; the textbook form zeta -> t -> c needs two of each, plus two more for a normalised convergence measure).  The rotation
    // angle is the same: tan(theta) = 2 gamma / (d + sign(d) hypot(d, 2 gamma)) with d = beta - alpha; convergence is tested on squares.
    for (int sweep = 0; sweep < 60; sweep++) {
        double off2 = 0;                                     // largest gamma^2 / (alpha beta) of the sweep, kept as a pair of products
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                double alpha = 0, beta = 0, gamma = 0;
#pragma unroll
                for (int i = 0; i < 4; i++) { alpha += A[i][p] * A[i][p]; beta += A[i][q] * A[i][q]; gamma += A[i][p] * A[i][q]; }
                const double ab = alpha * beta, g2 = gamma * gamma;
                // |gamma| > 1e-30 + 1e-17 sqrt(alpha beta)  (the pair is numerically orthogonal otherwise), on squares
                if (g2 > 1e-60 && g2 > 1e-34 * ab) {
                    rotated = true;
                    if (g2 > off2 * ab) off2 = g2 / (ab + 1e-300);
                    const double d = beta - alpha, tg = 2.0 * gamma;
                    const double hyp = sqrt(d * d + tg * tg);
                    const double t = tg / (d + (d >= 0 ? hyp : -hyp));
                    const double c = rsqrt(1.0 + t * t), s = c * t;
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const double ap = A[i][p], aq = A[i][q];
                        A[i][p] = c * ap - s * aq; A[i][q] = s * ap + c * aq;
                        const double vp = V[i][p], vq = V[i][q];
                        V[i][p] = c * vp - s * vq; V[i][q] = s * vp + c * vq;
                    }
                }
            }
        if (!rotated || off2 < 1e-30) break;                 // off = sqrt(off2) < 1e-15
    }
    double sv[4];
#pragma unroll
    for (int j = 0; j < 4; j++) sv[j] = sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j] + A[3][j] * A[3][j]);
    // smallest and second smallest singular value; V column of the smallest
    double s_min = sv[0], v0 = V[0][0], v1 = V[1][0], v2 = V[2][0], v3 = V[3][0];
#pragma unroll
    for (int j = 1; j < 4; j++)
        if (sv[j] < s_min) { s_min = sv[j]; v0 = V[0][j]; v1 = V[1][j]; v2 = V[2][j]; v3 = V[3][j]; }
    double s_2nd = 1e300;
    bool skipped = false;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (!skipped && sv[j] == s_min) { skipped = true; continue; }
        s_2nd = fmin(s_2nd, sv[j]);
    }
    xyz[0] = v0 / v3; xyz[1] = v1 / v3; xyz[2] = v2 / v3;              // algorithm.h:27
    ratio = s_min / s_2nd;                                             // algorithm.h:29
}

}  // namespace myslam_hip
