// gk_roi.hip — the coefficient masks of a shaped region of interest (ISO 15444-1 Annex H.3).
//
// A region is given on the image's samples; the encoder scales up (maxshift) every wavelet
// coefficient that takes part in reconstructing one of them.  Per decomposition level, in the
// interleaved coordinates of that level (even = low-pass, odd = high-pass, absolute parity), a
// region sample at k needs the coefficients of its synthesis cone:
//     5/3: |d| <= 1 for even k, |d| <= 2 for odd k;   9/7: |d| <= 3 for even k, |d| <= 4 for odd k,
// indices outside the tile-component reflected whole-sample symmetrically.  Reflection keeps the
// parity, so on the symmetrically extended mask the coefficient at j is in the region when a sample
// within R - 1 of it is (R = 2 / 4: every sample reaches that far), or, for odd j only, a sample at
// distance R (only odd samples reach R, and they have j's parity).  Two dimensions are the
// product: rows, then columns.  The low/low positions are the next level's sample mask, the other
// parities that level's HL / LH / HH masks.
//
// The masks are bytes (0 / 1) in two planes laid out like a component's two work planes (gk_common.h):
// level l reads its samples in plane (l odd ? A : B) at the tile's corner and writes the four
// bands in Mallat placement into the other, so GkBlock::band_off (less the component's planes)
// and GkBlock::stride address a block's mask as they address its coefficients.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gk_common.h"
#include "gk_launch.h"

// Level-0 mask of the whole image: inside a rectangle (x0, y0, x1, y1: half-open, image samples),
// or a non-zero byte of the caller's mask.  Four samples per thread, one dword store.
__global__ __launch_bounds__(256) void k_roi_fill(uint8_t* __restrict__ dst, uint32_t stride, uint32_t w, uint32_t h,
                                                  const uint32_t* __restrict__ rects, uint32_t nrects,
                                                  const uint8_t* __restrict__ mask, uint32_t mask_stride) {
    const uint32_t x4 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x4 >= w) return;
    for (uint32_t y = blockIdx.y; y < h; y += gridDim.y) {
        uint32_t v = 0;
        for (uint32_t r = 0; r < nrects; ++r) {
            const uint32_t rx0 = rects[4 * r], ry0 = rects[4 * r + 1], rx1 = rects[4 * r + 2], ry1 = rects[4 * r + 3];
            if (y < ry0 || y >= ry1) continue;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) v |= (x4 + k >= rx0 && x4 + k < rx1) ? 1u << (8 * k) : 0u;
        }
        if (mask) {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
                if (x4 + k < w && mask[(size_t)y * mask_stride + x4 + k]) v |= 1u << (8 * k);
        }
        // (the plane's rows are padded to a multiple of 64 samples: the whole dword lies in the row)
        *reinterpret_cast<uint32_t*>(dst + (size_t)y * stride + x4) = v;
    }
}

#define ROI_TX 64
#define ROI_TY 32
#define ROI_H 4   // the widest halo (9/7)

// whole-sample symmetric reflection of i into [0, n), n >= 1
__device__ __forceinline__ uint32_t roi_reflect(int32_t i, uint32_t n) {
    if (n == 1) return 0;
    const int32_t p = 2 * ((int32_t)n - 1);
    int32_t m = i % p;
    if (m < 0) m += p;
    return (uint32_t)(m < (int32_t)n ? m : p - m);
}

// One decomposition level of every tile of a class (grid.z = tile): w x h samples whose origin has
// the parities (px, py), at the tile's corner of src; the band masks go to dst, deinterleaved.
template <bool REVERSIBLE>
__global__ __launch_bounds__(256) void k_roi_level(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                   uint32_t stride, uint32_t w, uint32_t h, uint32_t px, uint32_t py,
                                                   GkTiles tb) {
    constexpr int R = REVERSIBLE ? 2 : 4;   // the odd samples' reach; even samples reach R - 1
    __shared__ uint8_t s_in[ROI_TY + 2 * ROI_H][ROI_TX + 2 * ROI_H + 4];
    __shared__ uint8_t s_mid[ROI_TY + 2 * ROI_H][ROI_TX + 4];
    const uint64_t toff = tb.offset(blockIdx.z, stride);
    const uint8_t* s = src + toff;
    uint8_t* d = dst + toff;
    const int32_t bx = (int32_t)(blockIdx.x * ROI_TX), by = (int32_t)(blockIdx.y * ROI_TY);
    const int tid = threadIdx.x;
    // the samples of the block and its halo, reflected at the tile-component's edges
    for (int i = tid; i < (ROI_TY + 2 * R) * (ROI_TX + 2 * R); i += 256) {
        const int ly = i / (ROI_TX + 2 * R), lx = i % (ROI_TX + 2 * R);
        const uint32_t gx = roi_reflect(bx + lx - R, w), gy = roi_reflect(by + ly - R, h);
        s_in[ly][lx] = s[(size_t)gy * stride + gx];
    }
    __syncthreads();
    // rows
    for (int i = tid; i < (ROI_TY + 2 * R) * ROI_TX; i += 256) {
        const int ly = i / ROI_TX, lx = i % ROI_TX;
        const uint8_t* row = &s_in[ly][lx + R];
        uint8_t v = 0;
#pragma unroll
        for (int k = -(R - 1); k <= R - 1; ++k) v |= row[k];
        if ((bx + lx + (int32_t)px) & 1) v |= row[-R] | row[R];
        s_mid[ly][lx] = v;
    }
    __syncthreads();
    // columns, and each coefficient to its band
    const uint32_t nlx = (w + 1 - px) / 2, nly = (h + 1 - py) / 2;   // low-pass columns / rows
    const int lx = tid & 63;
    const uint32_t jx = (uint32_t)(bx + lx);
    if (jx >= w) return;
    const uint32_t ax = jx + px;
    const uint32_t ox = (ax & 1) ? nlx + (ax >> 1) : (ax >> 1) - px;
    for (int ly = tid >> 6; ly < ROI_TY; ly += 4) {
        const uint32_t jy = (uint32_t)(by + ly);
        if (jy >= h) break;
        uint8_t v = 0;
#pragma unroll
        for (int k = -(R - 1); k <= R - 1; ++k) v |= s_mid[ly + R + k][lx];
        const uint32_t ay = jy + py;
        if (ay & 1) v |= s_mid[ly][lx] | s_mid[ly + 2 * R][lx];
        const uint32_t oy = (ay & 1) ? nly + (ay >> 1) : (ay >> 1) - py;
        d[(size_t)oy * stride + ox] = v ? 1 : 0;
    }
}

// flag |= 1 when any of the n bytes is set (gk_set_encode_roi: is a device mask empty?)
__global__ __launch_bounds__(256) void k_roi_any(const uint8_t* __restrict__ m, size_t n, uint32_t* __restrict__ flag) {
    uint32_t v = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) v |= m[i];
    if (__any(v != 0) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}
void gk_launch_roi_any(hipStream_t st, const uint8_t* m, size_t n, uint32_t* flag) {
    if (!n) return;
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_roi_any, dim3((uint32_t)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, st, m, n, flag);
}

void gk_launch_roi_fill(hipStream_t st, uint8_t* dst, uint32_t stride, uint32_t w, uint32_t h, const uint32_t* rects,
                        uint32_t nrects, const uint8_t* mask, uint32_t mask_stride) {
    if (!w || !h) return;
    hipLaunchKernelGGL(k_roi_fill, dim3((w + 1023) / 1024, h < 65535u ? h : 65535u), dim3(256), 0, st, dst, stride, w, h, rects, nrects, mask,
                       mask_stride);
}

void gk_launch_roi_level(hipStream_t st, bool reversible, const uint8_t* src, uint8_t* dst, uint32_t stride, uint32_t w,
                         uint32_t h, uint32_t px, uint32_t py, GkTiles tb) {
    if (!w || !h || !tb.count()) return;
    const dim3 grid((w + ROI_TX - 1) / ROI_TX, (h + ROI_TY - 1) / ROI_TY, tb.count());
    if (reversible) hipLaunchKernelGGL(k_roi_level<true>, grid, dim3(256), 0, st, src, dst, stride, w, h, px, py, tb);
    else hipLaunchKernelGGL(k_roi_level<false>, grid, dim3(256), 0, st, src, dst, stride, w, h, px, py, tb);
}
