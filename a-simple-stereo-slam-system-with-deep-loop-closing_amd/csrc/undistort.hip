// undistort.hip — Camera::UndistortImage (src/camera.cpp:36-48) as Frontend::GrabStereoImage calls it on both images
// (src/frontend.cpp:47-51) when Camera.bNeedUndistortion is 1: cv::undistort(src, dst, K, D), bilinear, border 0.
//
// The map is per-camera constant: it is built once per handle on the host in f64 (undistort_map.h) and uploaded packed at 4 bytes per pixel.
// The remap is a gather: one block per (output tile, share of the batch) keeps its tile's map words in registers for every image it
// processes, stages the tile's source band (known when the plan is built) in LDS with dword loads, interpolates in OpenCV's fixed point
// (weights (32 - fx)(32 - fy) 32 ... summing to 32768, out = (sum + 16384) >> 15: here the same integer with the common factor 32 taken out)
// and stores 16 output bytes per thread with one dwordx4 where the row is 16-byte aligned.
#include "common.h"
#include "undistort_map.h"

#include <algorithm>
#include <cmath>

using namespace myslam_hip;

namespace {

constexpr size_t UD_MAX_BAND = 64 * 1024;          // LDS bytes a block may stage (160 KiB per CU: two such blocks still fit)

__global__ __launch_bounds__(256) void k_undistort(const uint32_t* __restrict__ map, const UdTile* __restrict__ tiles, int tiles_x, int th,
                                                   const uint8_t* __restrict__ src, int sstep, size_t sstride, uint8_t* __restrict__ dst, int dstep,
                                                   size_t dstride, int rows, int cols, int batch) {
    extern __shared__ uint32_t band32[];
    const uint8_t* band = reinterpret_cast<const uint8_t*>(band32);
    const int t = threadIdx.x, nthr = blockDim.x;
    const int tile = blockIdx.x;
    const UdTile T = tiles[tile];
    const int r = t >> 3, c = (t & 7) * 16;
    const int ox = (tile % tiles_x) * UD_TW + c, oy = (tile / tiles_x) * th + r;
    const bool live = oy < rows && ox < cols;
    uint32_t m[16];
    {
        const uint4* mp = reinterpret_cast<const uint4*>(map + (size_t)tile * UD_TW * th + r * UD_TW + c);
#pragma unroll
        for (int q = 0; q < 4; q++) { const uint4 v = mp[q]; m[4 * q] = v.x; m[4 * q + 1] = v.y; m[4 * q + 2] = v.z; m[4 * q + 3] = v.w; }
    }
    const unsigned bw4 = (unsigned)T.bwp >> 2, nd = bw4 * (unsigned)T.bh;
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        const uint8_t* S = src + (size_t)b * sstride;
        __syncthreads();                                 // the previous image's band has been read
        for (unsigned k = t; k < nd; k += nthr) {
            const unsigned br = k / bw4;
            const int gy = T.by0 + (int)br, gx = T.bx0 + (int)(k - br * bw4) * 4;
            uint32_t v = 0;
            if ((unsigned)gy < (unsigned)rows) {
                const uint8_t* p = S + (size_t)gy * sstep + gx;
                if (gx >= 0 && gx + 3 < cols) {
                    // the two aligned dwords that hold bytes gx .. gx + 3 of this row (each holds at least one of them)
                    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
                    const uint32_t* pa = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
                    const unsigned sh = (unsigned)(a & 3);
                    const uint32_t lo = pa[0];
                    v = sh ? __builtin_amdgcn_alignbyte(pa[1], lo, sh) : lo;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        if ((unsigned)(gx + q) < (unsigned)cols) v |= (uint32_t)p[q] << (8 * q);
                }
            }
            band32[k] = v;
        }
        __syncthreads();
        if (!live) continue;
        uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t w = m[j];
            uint32_t px = 0;
            if (w != UD_ZERO) {
                const int fx = (int)(w & 31), fy = (int)((w >> 5) & 31);
                const uint8_t* q = band + (int)(w >> 21) * T.bwp + (int)((w >> 10) & 2047);
                const int p00 = q[0], p01 = q[1], p10 = q[T.bwp], p11 = q[T.bwp + 1];
                const int top = p00 * 32 + (p01 - p00) * fx, bot = p10 * 32 + (p11 - p10) * fx;     // p00 (32 - fx) + p01 fx
                px = (uint32_t)((top * 32 + (bot - top) * fy + 512) >> 10);
            }
            o[j >> 2] |= px << (8 * (j & 3));
        }
        uint8_t* D = dst + (size_t)b * dstride + (size_t)oy * dstep + ox;
        const uintptr_t a = reinterpret_cast<uintptr_t>(D);
        if (ox + 16 <= cols) {
            if ((a & 15) == 0) {
                *reinterpret_cast<uint4*>(D) = make_uint4(o[0], o[1], o[2], o[3]);
            } else if ((a & 3) == 0) {
#pragma unroll
                for (int q = 0; q < 4; q++) reinterpret_cast<uint32_t*>(D)[q] = o[q];
            } else if ((a & 1) == 0) {
#pragma unroll
                for (int q = 0; q < 8; q++) reinterpret_cast<uint16_t*>(D)[q] = (uint16_t)(o[q >> 1] >> (16 * (q & 1)));
            } else {
#pragma unroll
                for (int q = 0; q < 16; q++) D[q] = (uint8_t)(o[q >> 2] >> (8 * (q & 3)));
            }
        } else {
            for (int q = 0; q < cols - ox; q++) D[q] = (uint8_t)(o[q >> 2] >> (8 * (q & 3)));
        }
    }
}

}  // namespace

struct myslam_undistort {
    hipStream_t stream = nullptr;
    int rows = 0, cols = 0, th = 0, tiles_x = 0, tiles_y = 0;
    size_t band_bytes = 0;
    std::vector<int16_t> xy; std::vector<uint16_t> frac;           // OpenCV's CV_16SC2 / CV_16UC1 maps (myslam_undistort_get_map)
    Buf<uint32_t> d_map; Buf<UdTile> d_tiles;
    Buf<uint8_t> d_img;                                  // staging of myslam_undistort_image
    std::vector<uint8_t> hostOut;
};

namespace {

int ud_launch(myslam_undistort* h, const uint8_t* d_src, int batch, int src_step, size_t src_stride, uint8_t* d_dst, int dst_step, size_t dst_stride) {
    const int ntiles = h->tiles_x * h->tiles_y;
    const int split = std::max(1, std::min(batch, (2048 + ntiles - 1) / ntiles));          // ~8 blocks per CU; each block loops over its share
    hipLaunchKernelGGL(k_undistort, dim3(ntiles, split), dim3(8 * h->th), h->band_bytes, h->stream, h->d_map, h->d_tiles, h->tiles_x, h->th,
                       d_src, src_step, src_stride, d_dst, dst_step, dst_stride, h->rows, h->cols, batch);
    MYSLAM_HIP_CHECK(hipGetLastError());
    return MYSLAM_OK;
}

}  // namespace

extern "C" {

int myslam_undistort_create(myslam_undistort** out, int rows, int cols, const float* K, const float* D) {
    if (!out || !K || !D || rows < 1 || cols < 1 || cols > 30000 || rows > 30000) return MYSLAM_ERR_INVALID;
    for (int i = 0; i < 4; i++) if (!std::isfinite(K[i]) || !std::isfinite(D[i])) return MYSLAM_ERR_INVALID;
    if (need_device()) return MYSLAM_ERR_HIP;
    myslam_undistort* h = new myslam_undistort();
    h->rows = rows; h->cols = cols;
    ud_build_cv_maps(rows, cols, K, D, h->xy, h->frac);
    std::vector<uint32_t> map; std::vector<UdTile> tiles;
    int th = 32;
    while (th >= 1 && !ud_pack(rows, cols, th, h->xy, h->frac, UD_MAX_BAND, map, tiles, h->band_bytes)) th >>= 1;
    if (th < 1) { delete h; return MYSLAM_ERR_UNSUPPORTED; }       // a single tile row's source band exceeds the LDS budget
    h->th = th; h->tiles_x = (cols + UD_TW - 1) / UD_TW; h->tiles_y = (rows + th - 1) / th;
    h->band_bytes = (h->band_bytes + 15) & ~(size_t)15;
    if (h->d_map.renew(map.size()) != MYSLAM_OK || h->d_tiles.renew(tiles.size()) != MYSLAM_OK ||
        upload_table(h->d_map, map.data(), map.size() * 4) != MYSLAM_OK || upload_table(h->d_tiles, tiles.data(), tiles.size() * sizeof(UdTile)) != MYSLAM_OK) {
        delete h;
        return MYSLAM_ERR_HIP;
    }
    *out = h;
    return MYSLAM_OK;
}

int myslam_undistort_destroy(myslam_undistort* h) {
    if (!h) return MYSLAM_ERR_INVALID;
    (void)hipStreamSynchronize(h->stream);
    delete h;
    return MYSLAM_OK;
}

int myslam_undistort_set_stream(myslam_undistort* h, void* s) {
    if (!h) return MYSLAM_ERR_INVALID;
    h->stream = (hipStream_t)s;
    return MYSLAM_OK;
}

int myslam_undistort_get_map(const myslam_undistort* h, int16_t* xy, uint16_t* frac) {
    if (!h || (!xy && !frac)) return MYSLAM_ERR_INVALID;
    if (xy) memcpy(xy, h->xy.data(), h->xy.size() * sizeof(int16_t));
    if (frac) memcpy(frac, h->frac.data(), h->frac.size() * sizeof(uint16_t));
    return MYSLAM_OK;
}

int myslam_undistort_image(myslam_undistort* h, const uint8_t* src, int src_step, uint8_t* dst, int dst_step) {
    if (!h || !src || !dst || src_step < h->cols || dst_step < h->cols) return MYSLAM_ERR_INVALID;
    const int rows = h->rows, cols = h->cols;
    const size_t inBytes = (size_t)(rows - 1) * src_step + cols, inPad = (inBytes + 255) & ~(size_t)255, outBytes = (size_t)rows * cols;
    if (inPad + outBytes > h->d_img.size()) {
        MYSLAM_HIP_CHECK(hipStreamSynchronize(h->stream));
        const int rc = h->d_img.renew(inPad + outBytes);
        if (rc) return rc;
    }
    hipStream_t s = h->stream;
    MYSLAM_HIP_CHECK(hipMemcpyAsync(h->d_img, src, inBytes, hipMemcpyHostToDevice, s));       // one contiguous copy with the caller's pitch
    int rc = ud_launch(h, h->d_img, 1, src_step, inPad, h->d_img + inPad, cols, outBytes);
    if (rc) return rc;
    if (dst_step == cols) {                       // src == dst is fine: the source was uploaded before anything is written back
        MYSLAM_HIP_CHECK(hipMemcpyAsync(dst, h->d_img + inPad, outBytes, hipMemcpyDeviceToHost, s));
        MYSLAM_HIP_CHECK(hipStreamSynchronize(s));
    } else {                                      // a padded destination keeps the bytes between its rows
        h->hostOut.resize(outBytes);
        MYSLAM_HIP_CHECK(hipMemcpyAsync(h->hostOut.data(), h->d_img + inPad, outBytes, hipMemcpyDeviceToHost, s));
        MYSLAM_HIP_CHECK(hipStreamSynchronize(s));
        for (int y = 0; y < rows; y++) memcpy(dst + (size_t)y * dst_step, h->hostOut.data() + (size_t)y * cols, cols);
    }
    return MYSLAM_OK;
}

int myslam_undistort_batch(myslam_undistort* h, const uint8_t* d_src, int batch, int src_step, size_t src_stride, uint8_t* d_dst, int dst_step,
                           size_t dst_stride) {
    if (!h || !d_src || !d_dst || batch < 1 || src_step < h->cols || dst_step < h->cols) return MYSLAM_ERR_INVALID;
    const size_t inImg = (size_t)(h->rows - 1) * src_step + h->cols, outImg = (size_t)(h->rows - 1) * dst_step + h->cols;
    if (batch > 1 && dst_stride < outImg) return MYSLAM_ERR_INVALID;          // output images may not overlap each other
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src), s1 = s0 + (size_t)(batch - 1) * src_stride + inImg;
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(d_dst), d1 = d0 + (size_t)(batch - 1) * dst_stride + outImg;
    if (s0 < d1 && d0 < s1) return MYSLAM_ERR_INVALID;                        // a gather cannot run in place
    return ud_launch(h, d_src, batch, src_step, src_stride, d_dst, dst_step, dst_stride);
}

}  // extern "C"
