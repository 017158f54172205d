// lk.hip — pyramidal Lucas-Kanade tracker on gfx950, the operator the reference calls as
//   cv::calcOpticalFlowPyrLK(prev, next, prevPts, nextPts, status, err, Size(11,11), 3,
//                            TermCriteria(COUNT+EPS, 30, 0.01), OPTFLOW_USE_INITIAL_FLOW)
// in Frontend::TrackLastFrame (src/frontend.cpp:150-153) and Frontend::FindFeaturesInRight (:358-361)  [SURVEY.md §8(f) rank 1].
//
// Arithmetic (OpenCV lkpyramid.cpp, restated by the test oracle): pyrDown 5x5 [1 4 6 4 1]/16 REFLECT_101, 3x3 Scharr
// derivatives as shorts (zero outside the image), W_BITS = 14 fixed-point bilinear patch extraction, 2x2 normal equations.
// The window sums are exact integer sums converted to float once (the restatement's definition), so the tracker is bit-exact
// against the oracle; every float expression uses explicit non-fused IEEE operations.
//
// One wave per point, all pyramid levels inside the wave (coarse to fine), no global scratch: the (win+3)^2 patch of I, its
// Scharr derivatives and the (win+1)^2 window of J live in LDS; the template patch (I, Ix, Iy at the window pixels) stays in
// registers (2 window pixels per lane).  Sums over the window are DPP wave reductions of 32-bit halves (exact).
#include <limits.h>
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "common.h"

namespace myslam_hip {

constexpr int LK_MAXL = 6;          // pyramid levels supported (the reference uses maxLevel = 3)
constexpr int LK_MAXWIN = 15;       // window sizes up to 15x15 fit 4 window pixels per lane (11x11 -> 2 per lane)
constexpr int LK_WPL = 4;

struct LkGeom {
    int levels;                     // top level index actually used
    int w[LK_MAXL + 1], h[LK_MAXL + 1];
    size_t off[LK_MAXL + 1];        // byte offset of level l >= 1 inside one image's pyramid block
    size_t bytes;                   // pyramid block bytes per image (levels >= 1)
};

// cvFloor with the rule for what does not fit an int stated: NaN, +-inf and every value outside [-2^31, 2^31) give INT_MIN, which fails
// each bounds test of the tracker (the point is reported lost); the bare conversion of such a value is undefined in C++
__device__ __forceinline__ int lk_floor(float v) {
    if (!(v >= -2147483648.f && v < 2147483648.f)) return INT_MIN;
    return (int)floorf(v);
}

// cv::pyrDown 8UC1: one thread per destination pixel
// `sel` (the multi-stream tracker, tracker.hip; NULL everywhere else): image b lives in the sel[b]-th of two equally laid out buffers that are
// srcSel / dstSel bytes apart; sel[b] < 0 = image b is skipped
__global__ __launch_bounds__(256) void k_pyr_down(const uint8_t* __restrict__ src, int sw, int sh, int sstep, size_t sstride,
                                                  uint8_t* __restrict__ dst, int dw, int dh, size_t dstride, const int32_t* __restrict__ sel,
                                                  size_t srcSel, size_t dstSel) {
    const int b = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= dw || y >= dh) return;
    if (sel) {
        const int k = sel[b];
        if (k < 0) return;
        src += (size_t)k * srcSel; dst += (size_t)k * dstSel;
    }
    const uint8_t* S = src + (size_t)b * sstride;
    int xs[5];
#pragma unroll
    for (int i = 0; i < 5; i++) xs[i] = reflect101(2 * x + i - 2, sw);
    int s = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const uint8_t* row = S + (size_t)reflect101(2 * y + j - 2, sh) * sstep;
        const int r = row[xs[0]] + 4 * row[xs[1]] + 6 * row[xs[2]] + 4 * row[xs[3]] + row[xs[4]];
        s += (j == 0 || j == 4) ? r : (j == 2 ? 6 * r : 4 * r);
    }
    dst[(size_t)b * dstride + (size_t)y * dw + x] = (uint8_t)((s + 128) >> 8);
}

// exact wave sum of per-lane int32 partials whose total may exceed 32 bits: sum the high part and the low byte separately (wave_sum_lane63,
// wave_ops.h: the total in lane 63, broadcast to the wave)
__device__ __forceinline__ long long lk_wave_sum64(int v) {
    const int hi = __builtin_amdgcn_readlane(wave_sum_lane63(v >> 8), 63), lo = __builtin_amdgcn_readlane(wave_sum_lane63(v & 0xff), 63);
    return (long long)hi * 256 + lo;
}

struct LkArgs {
    const uint8_t* prev; const uint8_t* next; int rows, cols, pstep, nstep; size_t pstride, nstride;
    const uint8_t* pyrP; const uint8_t* pyrN;        // levels >= 1 of every image
    LkGeom g;
    const float* prev_pts; float* next_pts; const int32_t* counts; int n_fixed, cap;
    int win, max_iters; float eps2, min_eig;
    uint8_t* status; float* err;
    // the multi-stream tracker (tracker.hip; NULL everywhere else): pair b tracks from buffer 1 - sel[b] into buffer sel[b] of two equally laid
    // out (image, pyramid) buffers imgSel / pyrSel bytes apart; prev == next and pyrP == pyrN name buffer 0 then
    const int32_t* sel; size_t imgSel, pyrSel;
};

__global__ __launch_bounds__(256) void k_lk_track(LkArgs a) {
    constexpr int PI_MAX = LK_MAXWIN + 3, PJ_MAX = LK_MAXWIN + 1;
    __shared__ uint8_t s_I[4][PI_MAX * PI_MAX];
    __shared__ short s_dx[4][PJ_MAX * PJ_MAX], s_dy[4][PJ_MAX * PJ_MAX];
    __shared__ uint8_t s_J[4][PJ_MAX * PJ_MAX];
    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pi = blockIdx.x * 4 + wave;
    const int n = a.counts ? min(a.counts[b], a.cap) : a.n_fixed;          // counts above cap are read as cap
    if (pi >= n) return;                                            // wave-uniform
    const uint8_t *prev0 = a.prev, *next0 = a.next, *pyrP = a.pyrP, *pyrN = a.pyrN;
    if (a.sel) {                                                    // block-uniform
        const int k = a.sel[b];
        if (k < 0) return;
        prev0 += (size_t)(1 - k) * a.imgSel; next0 += (size_t)k * a.imgSel;
        pyrP += (size_t)(1 - k) * a.pyrSel; pyrN += (size_t)k * a.pyrSel;
    }
    const int win = a.win, ww = win * win, pI = win + 3, pJ = win + 1;
    const float halfWin = (float)(win - 1) * 0.5f;
    const float* pp = a.prev_pts + ((size_t)b * a.cap + pi) * 2;
    float* np_ = a.next_pts + ((size_t)b * a.cap + pi) * 2;
    const float p0x = pp[0], p0y = pp[1];
    float outx = np_[0], outy = np_[1];                             // nextPts[ptidx], carried across levels
    int status = 1; float errv = 0.f;
    uint8_t* sI = s_I[wave]; short* sdx = s_dx[wave]; short* sdy = s_dy[wave]; uint8_t* sJ = s_J[wave];
    constexpr int W_BITS = 14;
    const float FLT_SCALE = 1.f / (1 << 20);

    for (int level = a.g.levels; level >= 0; level--) {
        const int lw = a.g.w[level], lh = a.g.h[level];
        const uint8_t* I; const uint8_t* J; int istep, jstep;
        if (level == 0) { I = prev0 + (size_t)b * a.pstride; J = next0 + (size_t)b * a.nstride; istep = a.pstep; jstep = a.nstep; }
        else { I = pyrP + (size_t)b * a.g.bytes + a.g.off[level]; J = pyrN + (size_t)b * a.g.bytes + a.g.off[level]; istep = jstep = lw; }
        const float sc = (float)(1. / (1 << level));
        float prx = __fmul_rn(p0x, sc), pry = __fmul_rn(p0y, sc);
        float nx, ny;
        if (level == a.g.levels) { nx = __fmul_rn(outx, sc); ny = __fmul_rn(outy, sc); }          // OPTFLOW_USE_INITIAL_FLOW
        else { nx = __fmul_rn(outx, 2.f); ny = __fmul_rn(outy, 2.f); }
        outx = nx; outy = ny;
        prx = __fsub_rn(prx, halfWin); pry = __fsub_rn(pry, halfWin);
        const int ipx = lk_floor(prx), ipy = lk_floor(pry);
        if (ipx < -win || ipx >= lw || ipy < -win || ipy >= lh) {
            if (level == 0) { status = 0; errv = 0.f; }
            continue;
        }
        // ---- stage the (win+3)^2 patch of I (origin ipx-1, ipy-1), REFLECT_101 ----
        __builtin_amdgcn_wave_barrier();
        for (int i = lane; i < pI * pI; i += 64) {
            const int r = i / pI, c = i - r * pI;
            sI[i] = I[(size_t)reflect101(ipy - 1 + r, lh) * istep + reflect101(ipx - 1 + c, lw)];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ---- Scharr derivatives at the (win+1)^2 positions the bilinear taps touch; zero outside the image ----
        for (int i = lane; i < pJ * pJ; i += 64) {
            const int r = i / pJ, c = i - r * pJ;
            const int X = ipx + c, Y = ipy + r;
            int dx = 0, dy = 0;
            if (X >= 0 && X < lw && Y >= 0 && Y < lh) {
                const uint8_t* q = sI + r * pI + c;                 // top-left of the 3x3 neighbourhood
                const int a0 = q[0], a1 = q[1], a2 = q[2], b0 = q[pI], b2 = q[pI + 2], c0 = q[2 * pI], c1 = q[2 * pI + 1], c2 = q[2 * pI + 2];
                const int b1 = q[pI + 1];
                const int t00 = (a0 + c0) * 3 + b0 * 10, t02 = (a2 + c2) * 3 + b2 * 10;
                const int t10 = c0 - a0, t11 = c1 - a1, t12 = c2 - a2;
                (void)b1;
                dx = t02 - t00;
                dy = (t12 + t10) * 3 + t11 * 10;
            }
            sdx[i] = (short)dx; sdy[i] = (short)dy;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ---- template patch: I, Ix, Iy at the window pixels (registers), normal matrix ----
        float fa = __fsub_rn(prx, (float)ipx), fb = __fsub_rn(pry, (float)ipy);
        int iw00 = __float2int_rn(__fmul_rn(__fmul_rn(__fsub_rn(1.f, fa), __fsub_rn(1.f, fb)), (float)(1 << W_BITS)));
        int iw01 = __float2int_rn(__fmul_rn(__fmul_rn(fa, __fsub_rn(1.f, fb)), (float)(1 << W_BITS)));
        int iw10 = __float2int_rn(__fmul_rn(__fmul_rn(__fsub_rn(1.f, fa), fb), (float)(1 << W_BITS)));
        int iw11 = (1 << W_BITS) - iw00 - iw01 - iw10;
        int Ip[LK_WPL], Ix[LK_WPL], Iy[LK_WPL];
        int s11 = 0, s12 = 0, s22 = 0;
#pragma unroll
        for (int k = 0; k < LK_WPL; k++) {
            const int i = lane + 64 * k;
            Ip[k] = Ix[k] = Iy[k] = 0;
            if (i < ww) {
                const int y = i / win, x = i - y * win;
                const uint8_t* q = sI + (y + 1) * pI + x + 1;
                Ip[k] = (q[0] * iw00 + q[1] * iw01 + q[pI] * iw10 + q[pI + 1] * iw11 + (1 << (W_BITS - 6))) >> (W_BITS - 5);
                const short* dxp = sdx + y * pJ + x; const short* dyp = sdy + y * pJ + x;
                Ix[k] = (dxp[0] * iw00 + dxp[1] * iw01 + dxp[pJ] * iw10 + dxp[pJ + 1] * iw11 + (1 << (W_BITS - 1))) >> W_BITS;
                Iy[k] = (dyp[0] * iw00 + dyp[1] * iw01 + dyp[pJ] * iw10 + dyp[pJ + 1] * iw11 + (1 << (W_BITS - 1))) >> W_BITS;
                s11 += Ix[k] * Ix[k]; s12 += Ix[k] * Iy[k]; s22 += Iy[k] * Iy[k];
            }
        }
        const float A11 = __fmul_rn((float)lk_wave_sum64(s11), FLT_SCALE), A12 = __fmul_rn((float)lk_wave_sum64(s12), FLT_SCALE);
        const float A22 = __fmul_rn((float)lk_wave_sum64(s22), FLT_SCALE);
        float D = __fsub_rn(__fmul_rn(A11, A22), __fmul_rn(A12, A12));
        const float dA = __fsub_rn(A11, A22);
        const float minEig = __fdiv_rn(__fsub_rn(__fadd_rn(A22, A11), __fsqrt_rn(__fadd_rn(__fmul_rn(dA, dA), __fmul_rn(__fmul_rn(4.f, A12), A12)))),
                                       (float)(2 * win * win));
        if (minEig < a.min_eig || D < 1.19209290e-07f) {
            if (level == 0) status = 0;
            continue;
        }
        D = __fdiv_rn(1.f, D);
        nx = __fsub_rn(nx, halfWin); ny = __fsub_rn(ny, halfWin);
        float pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < a.max_iters; j++) {
            const int inx = lk_floor(nx), iny = lk_floor(ny);
            if (inx < -win || inx >= lw || iny < -win || iny >= lh) {
                if (level == 0) status = 0;
                break;
            }
            __builtin_amdgcn_wave_barrier();
            for (int i = lane; i < pJ * pJ; i += 64) {
                const int r = i / pJ, c = i - r * pJ;
                sJ[i] = J[(size_t)reflect101(iny + r, lh) * jstep + reflect101(inx + c, lw)];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            fa = __fsub_rn(nx, (float)inx); fb = __fsub_rn(ny, (float)iny);
            iw00 = __float2int_rn(__fmul_rn(__fmul_rn(__fsub_rn(1.f, fa), __fsub_rn(1.f, fb)), (float)(1 << W_BITS)));
            iw01 = __float2int_rn(__fmul_rn(__fmul_rn(fa, __fsub_rn(1.f, fb)), (float)(1 << W_BITS)));
            iw10 = __float2int_rn(__fmul_rn(__fmul_rn(__fsub_rn(1.f, fa), fb), (float)(1 << W_BITS)));
            iw11 = (1 << W_BITS) - iw00 - iw01 - iw10;
            int sb1 = 0, sb2 = 0;
#pragma unroll
            for (int k = 0; k < LK_WPL; k++) {
                const int i = lane + 64 * k;
                if (i < ww) {
                    const int y = i / win, x = i - y * win;
                    const uint8_t* q = sJ + y * pJ + x;
                    const int diff = ((q[0] * iw00 + q[1] * iw01 + q[pJ] * iw10 + q[pJ + 1] * iw11 + (1 << (W_BITS - 6))) >> (W_BITS - 5)) - Ip[k];
                    sb1 += diff * Ix[k]; sb2 += diff * Iy[k];
                }
            }
            const float b1 = __fmul_rn((float)lk_wave_sum64(sb1), FLT_SCALE), b2 = __fmul_rn((float)lk_wave_sum64(sb2), FLT_SCALE);
            const float dx = __fmul_rn(__fsub_rn(__fmul_rn(A12, b2), __fmul_rn(A22, b1)), D);
            const float dy = __fmul_rn(__fsub_rn(__fmul_rn(A12, b1), __fmul_rn(A11, b2)), D);
            nx = __fadd_rn(nx, dx); ny = __fadd_rn(ny, dy);
            outx = __fadd_rn(nx, halfWin); outy = __fadd_rn(ny, halfWin);
            if (__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) <= a.eps2) break;
            if (j > 0 && fabsf(__fadd_rn(dx, pdx)) < 0.01f && fabsf(__fadd_rn(dy, pdy)) < 0.01f) {
                outx = __fsub_rn(outx, __fmul_rn(dx, 0.5f)); outy = __fsub_rn(outy, __fmul_rn(dy, 0.5f));
                break;
            }
            pdx = dx; pdy = dy;
        }
        if (status && level == 0) {          // patch error at the final position; also the last bounds test (err is always requested)
            const float fx = __fsub_rn(outx, halfWin), fy = __fsub_rn(outy, halfWin);
            const int inx = lk_floor(fx), iny = lk_floor(fy);
            if (inx < -win || inx >= lw || iny < -win || iny >= lh) { status = 0; continue; }
            __builtin_amdgcn_wave_barrier();
            for (int i = lane; i < pJ * pJ; i += 64) {
                const int r = i / pJ, c = i - r * pJ;
                sJ[i] = J[(size_t)reflect101(iny + r, lh) * jstep + reflect101(inx + c, lw)];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            fa = __fsub_rn(fx, (float)inx); fb = __fsub_rn(fy, (float)iny);
            iw00 = __float2int_rn(__fmul_rn(__fmul_rn(__fsub_rn(1.f, fa), __fsub_rn(1.f, fb)), (float)(1 << W_BITS)));
            iw01 = __float2int_rn(__fmul_rn(__fmul_rn(fa, __fsub_rn(1.f, fb)), (float)(1 << W_BITS)));
            iw10 = __float2int_rn(__fmul_rn(__fmul_rn(__fsub_rn(1.f, fa), fb), (float)(1 << W_BITS)));
            iw11 = (1 << W_BITS) - iw00 - iw01 - iw10;
            int se = 0;
#pragma unroll
            for (int k = 0; k < LK_WPL; k++) {
                const int i = lane + 64 * k;
                if (i < ww) {
                    const int y = i / win, x = i - y * win;
                    const uint8_t* q = sJ + y * pJ + x;
                    const int diff = ((q[0] * iw00 + q[1] * iw01 + q[pJ] * iw10 + q[pJ + 1] * iw11 + (1 << (W_BITS - 6))) >> (W_BITS - 5)) - Ip[k];
                    se += diff < 0 ? -diff : diff;
                }
            }
            errv = __fmul_rn((float)lk_wave_sum64(se), 1.f / (float)(32 * win * win));
        }
    }
    if (lane == 0) {
        np_[0] = outx; np_[1] = outy;
        a.status[(size_t)b * a.cap + pi] = (uint8_t)status;
        if (a.err) a.err[(size_t)b * a.cap + pi] = errv;
    }
}

}  // namespace myslam_hip

using namespace myslam_hip;

struct myslam_lk {
    hipStream_t stream = nullptr;
    int win = 11, max_level = 3, max_iters = 30; float eps = 0.01f, min_eig = 1e-4f;
    int rows = 0, cols = 0, batchCap = 0;
    LkGeom g{};
    Buf<uint8_t> d_pyrP, d_pyrN;
    // host-entry staging: [prev | next] images; [prev_pts 2c | next_pts 2c | err c] floats and c status bytes for c points
    Buf<uint8_t> d_img; Buf<float> d_pts; Buf<uint8_t> d_st;
    // myslam_lk_track_cached / myslam_lk_prefetch: two (image, pyramid) slots that remember WHICH image they hold (a caller's token): the
    // `next` image of one tracked frame is the `prev` image of the following one (Frontend::TrackLastFrame, frontend.cpp:150-153), and the
    // frame after that can be uploaded while the current one is still being optimised
    struct Slot { Buf<uint8_t> img, pyr; uint64_t tok = 0; int rows = 0, cols = 0, step = 0; };
    Slot slot[2]; int lastNext = 0;
    // the cached call's points travel as ONE pinned upload [prev_pts | next_pts] and ONE pinned download [next_pts | err | status]
    PinBuf<uint8_t> h_pin; Buf<uint8_t> d_stage;
};

static int lk_plan(myslam_lk* h, int rows, int cols) {
    LkGeom g{};
    g.w[0] = cols; g.h[0] = rows; g.off[0] = 0; g.bytes = 0; g.levels = 0;
    int w = cols, hh = rows;
    for (int l = 0; l <= h->max_level; l++) {        // buildOpticalFlowPyramid: stop when the NEXT level would not exceed the window
        if (l > 0) {
            g.w[l] = (g.w[l - 1] + 1) / 2; g.h[l] = (g.h[l - 1] + 1) / 2;
            g.off[l] = g.bytes; g.bytes += ((size_t)g.w[l] * g.h[l] + 255) & ~(size_t)255;
        }
        g.levels = l;
        w = (w + 1) / 2; hh = (hh + 1) / 2;
        if (w <= h->win || hh <= h->win) break;
    }
    h->g = g; h->rows = rows; h->cols = cols; h->batchCap = 0;
    return MYSLAM_OK;
}

static int lk_ensure(myslam_lk* h, int batch, int rows, int cols) {
    if (rows != h->rows || cols != h->cols) { MYSLAM_HIP_CHECK(hipStreamSynchronize(h->stream)); lk_plan(h, rows, cols); }
    if (batch > h->batchCap) {
        MYSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
        const size_t nb = std::max<size_t>(256, (size_t)batch * h->g.bytes);
        return regrow(h->batchCap, batch, [&]() -> int {
            int rc;
            if ((rc = h->d_pyrP.renew(nb))) return rc;
            return h->d_pyrN.renew(nb);
        });
    }
    return MYSLAM_OK;
}

// levels 1 .. of `batch` images (level 0 at src0, row pitch step0, image stride stride0) into pyr
// sel / selBytes: see k_pyr_down (the level-0 images are never selected: they are the caller's)
static void lk_pyramid(myslam_lk* h, const uint8_t* src0, int step0, size_t stride0, uint8_t* pyr, int batch, const int32_t* sel = nullptr,
                       size_t selBytes = 0) {
    const LkGeom& g = h->g;
    for (int l = 1; l <= g.levels; l++) {
        const uint8_t* src = (l == 1) ? src0 : pyr + g.off[l - 1];
        const int sstep = (l == 1) ? step0 : g.w[l - 1];
        const size_t sstride = (l == 1) ? stride0 : g.bytes;
        hipLaunchKernelGGL(k_pyr_down, dim3((g.w[l] + 63) / 64, (g.h[l] + 3) / 4, batch), dim3(256), 0, h->stream, src, g.w[l - 1], g.h[l - 1], sstep, sstride,
                           pyr + g.off[l], g.w[l], g.h[l], g.bytes, sel, (l == 1) ? (size_t)0 : selBytes, selBytes);
    }
}

static int lk_track_launch(myslam_lk* h, const uint8_t* d_prev, const uint8_t* d_next, const uint8_t* pyrP, const uint8_t* pyrN, int batch, int rows, int cols,
                           int pstep, int nstep, size_t pstride, size_t nstride, const float* d_prev_pts, float* d_next_pts, const int32_t* d_counts,
                           int n_fixed, int cap, uint8_t* d_status, float* d_err, const int32_t* d_sel = nullptr, size_t imgSel = 0, size_t pyrSel = 0) {
    LkArgs a{d_prev, d_next, rows, cols, pstep, nstep, pstride, nstride, pyrP, pyrN, h->g, d_prev_pts, d_next_pts, d_counts, n_fixed, cap,
             h->win, h->max_iters, h->eps * h->eps, h->min_eig, d_status, d_err, d_sel, imgSel, pyrSel};
    hipLaunchKernelGGL(k_lk_track, dim3((cap + 3) / 4, batch), dim3(256), 0, h->stream, a);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

static int lk_run(myslam_lk* h, const uint8_t* d_prev, const uint8_t* d_next, int batch, int rows, int cols, int pstep, int nstep,
                  size_t pstride, size_t nstride, const float* d_prev_pts, float* d_next_pts, const int32_t* d_counts, int n_fixed, int cap,
                  uint8_t* d_status, float* d_err) {
    int rc = lk_ensure(h, batch, rows, cols);
    if (rc) return rc;
    lk_pyramid(h, d_prev, pstep, pstride, h->d_pyrP, batch);
    lk_pyramid(h, d_next, nstep, nstride, h->d_pyrN, batch);
    return lk_track_launch(h, d_prev, d_next, h->d_pyrP, h->d_pyrN, batch, rows, cols, pstep, nstep, pstride, nstride, d_prev_pts, d_next_pts, d_counts, n_fixed,
                           cap, d_status, d_err);
}

// ---- cached form: slots that remember their image ----
static int lk_plan_cached(myslam_lk* h, int rows, int cols) {
    if (rows == h->rows && cols == h->cols) return MYSLAM_OK;
    MYSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
    lk_plan(h, rows, cols);
    h->slot[0].tok = h->slot[1].tok = 0;                     // another geometry: nothing cached is usable
    return MYSLAM_OK;
}

// image -> slot i (one contiguous copy with the caller's row pitch, then the pyramid levels), asynchronous on the handle's stream
static int lk_fill_slot(myslam_lk* h, int i, const uint8_t* img, uint64_t tok, int rows, int cols, int step) {
    myslam_lk::Slot& S = h->slot[i];
    const size_t ib = (size_t)rows * step, pb = std::max<size_t>(256, h->g.bytes);
    if (ib > S.img.size() || pb > S.pyr.size()) {
        MYSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
        S = myslam_lk::Slot();
        int rc;
        if ((rc = S.img.renew(ib)) || (rc = S.pyr.renew(pb))) return rc;
    }
    S.tok = 0;                                               // not valid until everything below is enqueued
    MYSLAM_HIP_CHECK(hipMemcpyAsync(S.img, img, ib - (size_t)(step - cols), hipMemcpyHostToDevice, h->stream));     // the last row ends at its last pixel
    lk_pyramid(h, S.img, step, ib, S.pyr, 1);
    MYSLAM_HIP_CHECK(hipGetLastError());
    S.tok = tok; S.rows = rows; S.cols = cols; S.step = step;
    return MYSLAM_OK;
}

static int lk_find_slot(const myslam_lk* h, uint64_t tok, int rows, int cols, int step) {
    if (!tok) return -1;
    for (int i = 0; i < 2; i++) if (h->slot[i].tok == tok && h->slot[i].rows == rows && h->slot[i].cols == cols && h->slot[i].step == step) return i;
    return -1;
}

// ---- launch helpers of the multi-stream tracker (tracker.hip, declared in frontend_launch.h): the kernels above, unchanged arithmetic ----
namespace myslam_hip {

int lk_bank_plan(myslam_lk* h, int rows, int cols, size_t* pyr_bytes, int* levels) {
    lk_plan(h, rows, cols);
    *pyr_bytes = std::max<size_t>(256, h->g.bytes); *levels = h->g.levels;
    return MYSLAM_OK;
}

int lk_bank_pyramid(myslam_lk* h, const uint8_t* d_img, int step, size_t stride, uint8_t* d_pyr, int batch, const int32_t* d_sel, size_t pyr_sel) {
    lk_pyramid(h, d_img, step, stride, d_pyr, batch, d_sel, pyr_sel);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

int lk_bank_track(myslam_lk* h, const uint8_t* d_img, int step, size_t stride, const uint8_t* d_pyr, int batch, const int32_t* d_sel, size_t img_sel,
                  size_t pyr_sel, const float* d_prev_pts, float* d_next_pts, const int32_t* d_counts, int cap, uint8_t* d_status) {
    return lk_track_launch(h, d_img, d_img, d_pyr, d_pyr, batch, h->rows, h->cols, step, step, stride, stride, d_prev_pts, d_next_pts, d_counts, 0, cap,
                           d_status, nullptr, d_sel, img_sel, pyr_sel);
}

}  // namespace myslam_hip

extern "C" {

int myslam_lk_create(myslam_lk** out, int win, int max_level, int max_iters, float eps, float min_eig_threshold) {
    if (!out || win < 3 || win > LK_MAXWIN || (win & 1) == 0 || max_level < 0 || max_level > LK_MAXL || max_iters < 1 || !(eps >= 0)) return MYSLAM_ERR_INVALID;
    if (need_device()) return MYSLAM_ERR_HIP;
    myslam_lk* h = new myslam_lk();
    h->win = win; h->max_level = max_level; h->max_iters = max_iters; h->eps = eps; h->min_eig = min_eig_threshold;
    *out = h;
    return MYSLAM_OK;
}

int myslam_lk_destroy(myslam_lk* h) {
    if (!h) return MYSLAM_ERR_INVALID;
    (void)hipStreamSynchronize(h->stream);
    delete h;
    return MYSLAM_OK;
}

int myslam_lk_set_stream(myslam_lk* h, void* s) {
    if (!h) return MYSLAM_ERR_INVALID;
    h->stream = (hipStream_t)s;
    return MYSLAM_OK;
}

int myslam_lk_track_batch(myslam_lk* h, const uint8_t* d_prev, const uint8_t* d_next, int batch, int rows, int cols, int step, size_t stride,
                          const float* d_prev_pts, float* d_next_pts, const int32_t* d_counts, int cap, uint8_t* d_status, float* d_err) {
    if (!h || !d_prev || !d_next || batch < 1 || rows < 1 || cols < 1 || step < cols || !d_prev_pts || !d_next_pts || !d_counts || cap < 1 || !d_status)
        return MYSLAM_ERR_INVALID;
    return lk_run(h, d_prev, d_next, batch, rows, cols, step, step, stride, stride, d_prev_pts, d_next_pts, d_counts, 0, cap, d_status, d_err);
}

int myslam_lk_track(myslam_lk* h, const uint8_t* prev, const uint8_t* next, int rows, int cols, int prev_step, int next_step,
                    const float* prev_pts, float* next_pts, int n, uint8_t* status, float* err) {
    if (!h || n < 0 || (n > 0 && (!prev_pts || !next_pts || !status))) return MYSLAM_ERR_INVALID;
    if (n == 0) return MYSLAM_OK;
    if (!prev || !next || rows < 1 || cols < 1 || prev_step < cols || next_step < cols) return MYSLAM_ERR_INVALID;
    // both images travel as ONE contiguous copy each with their own row pitch (a 2-D copy from pageable memory goes row by row: 5 ms
    // for a 1241 x 376 pair against 0.1 ms), the kernels read them with that pitch
    const size_t pb = ((size_t)rows * prev_step + 255) & ~(size_t)255, nb = (size_t)rows * next_step;
    int rc;
    if (pb + nb > h->d_img.size()) {
        MYSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
        if ((rc = h->d_img.renew(pb + nb))) return rc;
    }
    if ((size_t)n > std::min(h->d_pts.size() / 5, h->d_st.size())) {
        MYSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
        h->d_pts.release(); h->d_st.release();
        if ((rc = h->d_pts.renew(5 * (size_t)n)) || (rc = h->d_st.renew((size_t)n))) return rc;
    }
    const size_t ptsCap = h->d_pts.size() / 5;
    hipStream_t s = h->stream;
    MYSLAM_HIP_CHECK(hipMemcpyAsync(h->d_img, prev, (size_t)rows * prev_step - (size_t)(prev_step - cols), hipMemcpyHostToDevice, s));      // the last row ends at its last pixel
    MYSLAM_HIP_CHECK(hipMemcpyAsync(h->d_img + pb, next, (size_t)rows * next_step - (size_t)(next_step - cols), hipMemcpyHostToDevice, s));
    float* d_pp = h->d_pts; float* d_np = d_pp + 2 * ptsCap; float* d_err = d_np + 2 * ptsCap;
    MYSLAM_HIP_CHECK(hipMemcpyAsync(d_pp, prev_pts, sizeof(float) * 2 * n, hipMemcpyHostToDevice, s));
    MYSLAM_HIP_CHECK(hipMemcpyAsync(d_np, next_pts, sizeof(float) * 2 * n, hipMemcpyHostToDevice, s));
    rc = lk_run(h, h->d_img, h->d_img + pb, 1, rows, cols, prev_step, next_step, pb, nb, d_pp, d_np, nullptr, n, n, h->d_st, d_err);
    if (rc) return rc;
    MYSLAM_HIP_CHECK(hipMemcpyAsync(next_pts, d_np, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, s));
    MYSLAM_HIP_CHECK(hipMemcpyAsync(status, h->d_st, n, hipMemcpyDeviceToHost, s));
    if (err) MYSLAM_HIP_CHECK(hipMemcpyAsync(err, d_err, sizeof(float) * n, hipMemcpyDeviceToHost, s));
    MYSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return MYSLAM_OK;
}

int myslam_lk_prefetch(myslam_lk* h, const uint8_t* img, uint64_t token, int rows, int cols, int step) {
    if (!h || !img || !token || rows < 1 || cols < 1 || step < cols) return MYSLAM_ERR_INVALID;
    int rc = lk_plan_cached(h, rows, cols);
    if (rc) return rc;
    if (lk_find_slot(h, token, rows, cols, step) >= 0) return MYSLAM_OK;                  // already there
    return lk_fill_slot(h, 1 - h->lastNext, img, token, rows, cols, step);                // never the slot the next call tracks FROM
}

int myslam_lk_track_cached(myslam_lk* h, const uint8_t* prev, uint64_t prev_token, const uint8_t* next, uint64_t next_token, int rows, int cols,
                           int prev_step, int next_step, const float* prev_pts, float* next_pts, int n, uint8_t* status, float* err) {
    if (!h || n < 0 || (n > 0 && (!prev_pts || !next_pts || !status))) return MYSLAM_ERR_INVALID;
    if (n == 0) return MYSLAM_OK;
    if (!prev || !next || rows < 1 || cols < 1 || prev_step < cols || next_step < cols) return MYSLAM_ERR_INVALID;
    int rc = lk_plan_cached(h, rows, cols);
    if (rc) return rc;
    int sp = lk_find_slot(h, prev_token, rows, cols, prev_step), sn = lk_find_slot(h, next_token, rows, cols, next_step);
    if (sp >= 0 && sp == sn) sn = -1;                                                     // one token for both images: the second is uploaded
    if (sp < 0) { sp = sn < 0 ? 0 : 1 - sn; if ((rc = lk_fill_slot(h, sp, prev, prev_token, rows, cols, prev_step))) return rc; }
    if (sn < 0) { sn = 1 - sp; if ((rc = lk_fill_slot(h, sn, next, next_token, rows, cols, next_step))) return rc; }
    if ((size_t)21 * n + 16 > std::min(h->d_stage.size(), h->h_pin.size())) {
        MYSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
        h->d_stage.release(); h->h_pin.release();
        const size_t bytes = (size_t)21 * std::max(n, 512) + 16;
        if ((rc = h->d_stage.renew(bytes)) || (rc = h->h_pin.renew(bytes))) return rc;
    }
    hipStream_t s = h->stream;
    // device block: [prev_pts 8n][next_pts 8n][err 4n][status n]; upload = the first 16n bytes, download = the last 13n
    float* d_pp = reinterpret_cast<float*>(h->d_stage.get()); float* d_np = d_pp + 2 * (size_t)n; float* d_err = d_np + 2 * (size_t)n;
    uint8_t* d_st = reinterpret_cast<uint8_t*>(d_err + n);
    memcpy(h->h_pin, prev_pts, sizeof(float) * 2 * n); memcpy(h->h_pin + sizeof(float) * 2 * n, next_pts, sizeof(float) * 2 * n);
    MYSLAM_HIP_CHECK(hipMemcpyAsync(h->d_stage, h->h_pin, sizeof(float) * 4 * n, hipMemcpyHostToDevice, s));
    const myslam_lk::Slot &P = h->slot[sp], &N = h->slot[sn];
    if ((rc = lk_track_launch(h, P.img, N.img, P.pyr, N.pyr, 1, rows, cols, prev_step, next_step, P.img.size(), N.img.size(), d_pp, d_np, nullptr, n, n, d_st, d_err)))
        return rc;
    h->lastNext = sn;
    uint8_t* hp = h->h_pin + sizeof(float) * 2 * n;
    MYSLAM_HIP_CHECK(hipMemcpyAsync(hp, d_np, (size_t)13 * n, hipMemcpyDeviceToHost, s));
    MYSLAM_HIP_CHECK(hipStreamSynchronize(s));
    memcpy(next_pts, hp, sizeof(float) * 2 * n);
    if (err) memcpy(err, hp + sizeof(float) * 2 * n, sizeof(float) * n);
    memcpy(status, hp + sizeof(float) * 3 * n, n);
    return MYSLAM_OK;
}

}  // extern "C"
