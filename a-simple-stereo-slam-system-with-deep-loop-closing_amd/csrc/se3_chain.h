// se3_chain.h — SE3 on 4 x 4 row-major doubles, the operations of chain.py (mm / T_of / T_inv / p7_of) in its order, every product and sum rounded
// on its own: what the hosts compute with plain f64 arithmetic, bit for bit.  Shared by tracker.hip (poses of a turn) and map_archive.hip (the
// odometry edges).  Units that include it are built with -ffp-contract=off as well.
#pragma once
#include <hip/hip_runtime.h>

namespace myslam_hip {

__device__ __forceinline__ double dmul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double dadd(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double dsub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double ddiv(double a, double b) { return __ddiv_rn(a, b); }

__device__ void se3_mm(const double* A, const double* B, double* C) {          // chain.mm: sum over k in ascending order
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double c = dmul(A[4 * i], B[j]);
            for (int k = 1; k < 4; k++) c = dadd(c, dmul(A[4 * i + k], B[4 * k + j]));
            C[4 * i + j] = c;
        }
}

__device__ void se3_T_of(const double* p, double* T) {                         // chain.T_of / q_to_R
    const double n = __dsqrt_rn(dadd(dadd(dadd(dmul(p[0], p[0]), dmul(p[1], p[1])), dmul(p[2], p[2])), dmul(p[3], p[3])));
    const double x = ddiv(p[0], n), y = ddiv(p[1], n), z = ddiv(p[2], n), w = ddiv(p[3], n);
    T[0] = dsub(1.0, dmul(2.0, dadd(dmul(y, y), dmul(z, z)))); T[1] = dmul(2.0, dsub(dmul(x, y), dmul(z, w))); T[2] = dmul(2.0, dadd(dmul(x, z), dmul(y, w)));
    T[4] = dmul(2.0, dadd(dmul(x, y), dmul(z, w))); T[5] = dsub(1.0, dmul(2.0, dadd(dmul(x, x), dmul(z, z)))); T[6] = dmul(2.0, dsub(dmul(y, z), dmul(x, w)));
    T[8] = dmul(2.0, dsub(dmul(x, z), dmul(y, w))); T[9] = dmul(2.0, dadd(dmul(y, z), dmul(x, w))); T[10] = dsub(1.0, dmul(2.0, dadd(dmul(x, x), dmul(y, y))));
    T[3] = p[4]; T[7] = p[5]; T[11] = p[6];
    T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
}

__device__ void se3_inv(const double* T, double* Ti) {                         // chain.T_inv: R^T, mv(-R^T, t)
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) Ti[4 * i + j] = T[4 * j + i];
        double r = dmul(-T[i], T[3]);
        r = dadd(r, dmul(-T[4 + i], T[7]));
        r = dadd(r, dmul(-T[8 + i], T[11]));
        Ti[4 * i + 3] = r;
    }
    Ti[12] = 0.0; Ti[13] = 0.0; Ti[14] = 0.0; Ti[15] = 1.0;
}

__device__ void se3_p7_of(const double* T, double* p) {                        // chain.p7_of / R_to_q
    const double R00 = T[0], R01 = T[1], R02 = T[2], R10 = T[4], R11 = T[5], R12 = T[6], R20 = T[8], R21 = T[9], R22 = T[10];
    const double t = dadd(dadd(R00, R11), R22);
    double q[4];
    if (t > 0) {
        const double s = dmul(__dsqrt_rn(dadd(t, 1.0)), 2.0);
        q[0] = ddiv(dsub(R21, R12), s); q[1] = ddiv(dsub(R02, R20), s); q[2] = ddiv(dsub(R10, R01), s); q[3] = dmul(0.25, s);
    } else if (R00 > R11 && R00 > R22) {
        const double s = dmul(__dsqrt_rn(dsub(dsub(dadd(1.0, R00), R11), R22)), 2.0);
        q[0] = dmul(0.25, s); q[1] = ddiv(dadd(R01, R10), s); q[2] = ddiv(dadd(R02, R20), s); q[3] = ddiv(dsub(R21, R12), s);
    } else if (R11 > R22) {
        const double s = dmul(__dsqrt_rn(dsub(dsub(dadd(1.0, R11), R00), R22)), 2.0);
        q[0] = ddiv(dadd(R01, R10), s); q[1] = dmul(0.25, s); q[2] = ddiv(dadd(R12, R21), s); q[3] = ddiv(dsub(R02, R20), s);
    } else {
        const double s = dmul(__dsqrt_rn(dsub(dsub(dadd(1.0, R22), R00), R11)), 2.0);
        q[0] = ddiv(dadd(R02, R20), s); q[1] = ddiv(dadd(R12, R21), s); q[2] = dmul(0.25, s); q[3] = ddiv(dsub(R10, R01), s);
    }
    const bool neg = !(q[3] >= 0);
    for (int k = 0; k < 4; k++) p[k] = neg ? -q[k] : q[k];
    p[4] = T[3]; p[5] = T[7]; p[6] = T[11];
}

}  // namespace myslam_hip
