// csrc/se3_quat.h on the host: the SE3 functions myslam_loop_local_fusion (csrc/pgo.hip) shares with the kernels.  Reads a file of doubles
// { n_active, cur, n_active x 7 active poses, 7 corrected pose }, writes the n_active x 7 fused poses of LoopClosing::LoopLocalFusion
// (src/loopclosing.cpp:470-482, the loop of myslam_loop_local_fusion restated), and checks on every pose it read, with no tolerance, that
// pg_inv(pg_inv(T)) returns T's quaternion and pg_store(pg_load(p)) returns p.  Built with AddressSanitizer + UBSan by tests/test_se3_quat.py;
// exit status 0 and "SE3 QUAT OK" = every check held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "se3_quat.h"

using namespace myslam_hip;

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) { printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static Se3 load_unit(const double* p) { Se3 T = pg_load(p); pg_qnorm(T.q); return T; }

int main(int argc, char** argv) {
    CHECK(argc == 3);
    FILE* f = fopen(argv[1], "rb");
    CHECK(f);
    double head[2];
    CHECK(fread(head, sizeof(double), 2, f) == 2);
    const int n = (int)head[0], cur = (int)head[1];
    CHECK(n >= 1 && n <= 64 && cur >= 0 && cur < n);
    std::vector<double> in((size_t)7 * (n + 1)), out((size_t)7 * n);
    CHECK(fread(in.data(), sizeof(double), in.size(), f) == in.size());
    fclose(f);
    const double* corrected = in.data() + 7 * n;

    for (int a = 0; a <= n; a++) {                          // every pose of the input, the corrected one included, as it is and normalised
        const double* p = in.data() + 7 * a;
        double back[7];
        pg_store(pg_load(p), back);
        CHECK(memcmp(back, p, sizeof(back)) == 0);
        for (const Se3& T : {pg_load(p), load_unit(p)}) {
            const Se3 TT = pg_inv(pg_inv(T));
            CHECK(memcmp(TT.q, T.q, sizeof(T.q)) == 0);
        }
    }

    const Se3 Tc_inv = pg_inv(load_unit(in.data() + 7 * cur)), Tcc = load_unit(corrected);
    for (int a = 0; a < n; a++)
        pg_store((a == cur) ? Tcc : pg_mul(pg_mul(load_unit(in.data() + 7 * a), Tc_inv), Tcc), out.data() + 7 * a);
    f = fopen(argv[2], "wb");
    CHECK(f);
    CHECK(fwrite(out.data(), sizeof(double), out.size(), f) == out.size());
    CHECK(fclose(f) == 0);
    printf("SE3 QUAT OK (%d poses)\n", n);
    return 0;
}
