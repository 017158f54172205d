// se3_quat.h — Sophus-style SE3 on a unit quaternion (x, y, z, w) and a translation, for host and device: rotate, renormalise, product (renormalised
// after every product as Sophus does), inverse, and the 7-double pose layout.  Only +, -, *, / and sqrt, which round alike on both sides; exp / log
// and everything built on them stay device-only in pg_shared.h (host libm differs from the device's).  Includes no HIP header, so
// tests/cpp/se3_quat_test.cpp compiles it with g++ alone.
#pragma once
#include <math.h>

#include "sorted_rows.h"       // MYSLAM_HD

namespace myslam_hip {

struct Se3 { double q[4]; double t[3]; };      // q = (x, y, z, w)

MYSLAM_HD void pg_rot(const double* q, const double* v, double* o) {
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
    o[0] = v[0] + q[3] * uv[0] + (q[1] * uv[2] - q[2] * uv[1]);
    o[1] = v[1] + q[3] * uv[1] + (q[2] * uv[0] - q[0] * uv[2]);
    o[2] = v[2] + q[3] * uv[2] + (q[0] * uv[1] - q[1] * uv[0]);
}

MYSLAM_HD void pg_qnorm(double* q) {
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
}

MYSLAM_HD Se3 pg_mul(const Se3& a, const Se3& b) {
    Se3 r;
    r.q[3] = a.q[3] * b.q[3] - a.q[0] * b.q[0] - a.q[1] * b.q[1] - a.q[2] * b.q[2];
    r.q[0] = a.q[3] * b.q[0] + a.q[0] * b.q[3] + a.q[1] * b.q[2] - a.q[2] * b.q[1];
    r.q[1] = a.q[3] * b.q[1] - a.q[0] * b.q[2] + a.q[1] * b.q[3] + a.q[2] * b.q[0];
    r.q[2] = a.q[3] * b.q[2] + a.q[0] * b.q[1] - a.q[1] * b.q[0] + a.q[2] * b.q[3];
    pg_qnorm(r.q);
    double rt[3];
    pg_rot(a.q, b.t, rt);
    r.t[0] = a.t[0] + rt[0]; r.t[1] = a.t[1] + rt[1]; r.t[2] = a.t[2] + rt[2];
    return r;
}

MYSLAM_HD Se3 pg_inv(const Se3& a) {
    Se3 r;
    r.q[0] = -a.q[0]; r.q[1] = -a.q[1]; r.q[2] = -a.q[2]; r.q[3] = a.q[3];
    double rt[3];
    pg_rot(r.q, a.t, rt);
    r.t[0] = -rt[0]; r.t[1] = -rt[1]; r.t[2] = -rt[2];
    return r;
}

// the 7 doubles of a pose: qx qy qz qw tx ty tz, taken as they are (pg_qnorm is the caller's step)
MYSLAM_HD Se3 pg_load(const double* p) {
    Se3 T;
    T.q[0] = p[0]; T.q[1] = p[1]; T.q[2] = p[2]; T.q[3] = p[3]; T.t[0] = p[4]; T.t[1] = p[5]; T.t[2] = p[6];
    return T;
}
MYSLAM_HD void pg_store(const Se3& T, double* p) {
    p[0] = T.q[0]; p[1] = T.q[1]; p[2] = T.q[2]; p[3] = T.q[3]; p[4] = T.t[0]; p[5] = T.t[1]; p[6] = T.t[2];
}

}  // namespace myslam_hip
