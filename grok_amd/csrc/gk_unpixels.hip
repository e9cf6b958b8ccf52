// gk_unpixels.hip — the input stage of an encode from packed pixels: k_pixels (gk_pixels.hip)
// turned round, (H, W, C) pixels into the planes the front ends read, in one pass.
//
// Shape (gk_pixels.hip's idiom).  A thread owns GK_PAL_PIX (8) consecutive pixels of a row and a
// workgroup 256 * 8 columns of `rows` rows.  The lane loads the 8 * C * es contiguous bytes of its
// 8 pixels in 16-, 8- or 4-byte loads, whichever the row's base address allows (uniform per row).  A row of 8 / 16-bit pixels whose base is not
// dword-aligned takes the bytes up to the boundary one by one, the aligned dwords between, and
// the remaining bytes, and funnels them back into the lane's packed words (v_alignbyte_b32): no
// byte outside [row, row + w * C * es) is read, so the pixels may end where their last row does.
// The channels are separated in registers (v_perm_b32) and leave as one vector store of 8 samples
// per channel (8, 16 or 32 bytes) into planes of the same sample type (signed samples are the
// same bits); the planes are the engine's own, bases and row strides aligned to 32 bytes.  The
// last, partial group of a row goes sample by sample.  No LDS, no cross-lane traffic.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "gk_common.h"
#include "gk_launch.h"

namespace {
constexpr int PIX = GK_PAL_PIX;
typedef uint32_t U4 __attribute__((ext_vector_type(4)));
typedef uint32_t U2 __attribute__((ext_vector_type(2)));

// the 8 samples v of one channel into a plane row at d (whole group: one vector store)
template <typename T> __device__ __forceinline__ void store8(T* d, const uint32_t (&o)[PIX * sizeof(T) / 4]) {
    if (sizeof(T) == 1) { U2 q = {o[0], o[1]}; *(U2*)d = q; }
    else if (sizeof(T) == 2) { U4 q = {o[0], o[1], o[2], o[3]}; *(U4*)d = q; }
    else {
        U4 q0 = {o[0], o[1], o[2], o[3]}, q1 = {o[4], o[5], o[6], o[7]};
        *(U4*)d = q0; *((U4*)d + 1) = q1;
    }
}

// channel K of the lane's packed words in[] (8 pixels of C channels, memory order) as the dwords
// of 8 consecutive plane samples
template <typename T, int C, int K>
__device__ __forceinline__ void unpack(const uint32_t (&in)[PIX * C * sizeof(T) / 4], uint32_t (&o)[PIX * sizeof(T) / 4]) {
    constexpr int NO = PIX * (int)sizeof(T) / 4;
#pragma unroll
    for (int j = 0; j < NO; ++j) {
        if (sizeof(T) == 4) {
            o[j] = in[j * C + K];
        } else if (sizeof(T) == 2) {
            // samples i0 (pixel 2j) and i1 (pixel 2j + 1) of the channel: a half of a word each
            const int i0 = (2 * j) * C + K, i1 = (2 * j + 1) * C + K;
            const uint32_t b0 = 2u * (i0 & 1), b1 = 4u + 2u * (i1 & 1);
            o[j] = __builtin_amdgcn_perm(in[i1 / 2], in[i0 / 2], b0 | (b0 + 1) << 8 | b1 << 16 | (b1 + 1) << 24);
        } else {
            // four samples, a byte of a word each: two pairs (upper half zero), then the halves
            const int i0 = (4 * j) * C + K, i1 = i0 + C, i2 = i1 + C, i3 = i2 + C;
            const uint32_t lo = __builtin_amdgcn_perm(in[i1 / 4], in[i0 / 4], (uint32_t)(i0 & 3) | (4u + (i1 & 3)) << 8 | 0x0c0c0000u);
            const uint32_t hi = __builtin_amdgcn_perm(in[i3 / 4], in[i2 / 4], (uint32_t)(i2 & 3) | (4u + (i3 & 3)) << 8 | 0x0c0c0000u);
            o[j] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
        }
    }
}

template <typename T, int C, int K> struct UnpackAll {
    static __device__ __forceinline__ void run(const uint32_t (&in)[PIX * C * sizeof(T) / 4], T* plane0, size_t plane) {
        uint32_t o[PIX * sizeof(T) / 4];
        unpack<T, C, K>(in, o);
        store8<T>(plane0 + (size_t)K * plane, o);
        UnpackAll<T, C, K + 1>::run(in, plane0, plane);
    }
};
template <typename T, int C> struct UnpackAll<T, C, C> {
    static __device__ __forceinline__ void run(const uint32_t (&)[PIX * C * sizeof(T) / 4], T*, size_t) {}
};

// T: uint8_t / uint16_t / uint32_t (the sample's bits); C: channels per pixel (1..4)
template <typename T, int C>
__global__ __launch_bounds__(256) void k_unpixels(GkUnpixArgs a) {
    constexpr int LB = PIX * C * (int)sizeof(T);   // the lane's input bytes per row
    constexpr int NW = LB / 4;
    const uint32_t x = (blockIdx.x * 256 + threadIdx.x) * PIX;
    if (x >= a.w) return;
    const bool whole = x + PIX <= a.w;
    const uint32_t n = whole ? PIX : a.w - x;
    const uint32_t y0 = blockIdx.y * a.rows, y1 = min(a.h, y0 + a.rows);
    for (uint32_t y = y0; y < y1; ++y) {
        const uint8_t* row = (const uint8_t*)a.src + (size_t)y * a.row_bytes;
        const uint8_t* s = row + (size_t)x * C * sizeof(T);
        T* d = (T*)a.dst + (size_t)y * a.ds + x;   // channel 0's plane; channel k lies a.plane samples on
        const uint32_t mis = (uint32_t)(uintptr_t)row & 15u;   // uniform: the lane's offset is a multiple of 8
        if (whole && (sizeof(T) == 4 || (mis & 3u) == 0)) {
            uint32_t in[NW];
            if (LB % 16 == 0 && mis == 0) {
#pragma unroll
                for (int j = 0; j < NW; j += 4) { const U4 q = *(const U4*)(s + 4 * j); in[j] = q.x; in[j + 1] = q.y; in[j + 2] = q.z; in[j + 3] = q.w; }
            } else if ((mis & 7u) == 0) {
#pragma unroll
                for (int j = 0; j < NW; j += 2) { const U2 q = *(const U2*)(s + 4 * j); in[j] = q.x; in[j + 1] = q.y; }
            } else {
#pragma unroll
                for (int j = 0; j < NW; ++j) in[j] = *(const uint32_t*)(s + 4 * j);
            }
            UnpackAll<T, C, 0>::run(in, d, a.plane);
        } else if (whole) {
            // the row starts m = 1..3 bytes past a dword boundary (as every lane's run does): hb =
            // 4 - m bytes reach the boundary, then NW - 1 aligned dwords, then the last m bytes
            const uint32_t m = mis & 3u, hb = 4u - m;
            uint32_t w[NW + 1];
            w[0] = 0; w[NW] = 0;
#pragma unroll
            for (int b = 0; b < 3; ++b)
                if (b < (int)hb) w[0] |= (uint32_t)s[b] << (8 * (m + b));
#pragma unroll
            for (int j = 0; j + 1 < NW; ++j) w[j + 1] = *(const uint32_t*)(s + hb + 4 * j);
#pragma unroll
            for (int b = 0; b < 3; ++b)
                if (b < (int)m) w[NW] |= (uint32_t)s[4 * (NW - 1) + hb + b] << (8 * b);
            uint32_t in[NW];
#pragma unroll
            for (int j = 0; j < NW; ++j) in[j] = __builtin_amdgcn_alignbyte(w[j + 1], w[j], m);
            UnpackAll<T, C, 0>::run(in, d, a.plane);
        } else {
            const T* e = (const T*)s;
#pragma unroll
            for (int p = 0; p < PIX; ++p)
                if (p < (int)n) {
#pragma unroll
                    for (int k = 0; k < C; ++k) d[(size_t)k * a.plane + p] = e[p * C + k];
                }
        }
    }
}

// 5..16 channels: one channel at a time, samples loaded one by one at the pixel stride
template <typename T>
__global__ __launch_bounds__(256) void k_unpixels_any(GkUnpixArgs a) {
    constexpr int NO = PIX * (int)sizeof(T) / 4;
    const uint32_t x = (blockIdx.x * 256 + threadIdx.x) * PIX;
    if (x >= a.w) return;
    const bool whole = x + PIX <= a.w;
    const uint32_t n = whole ? PIX : a.w - x;
    const uint32_t y0 = blockIdx.y * a.rows, y1 = min(a.h, y0 + a.rows);
    for (uint32_t y = y0; y < y1; ++y) {
        const T* e = (const T*)((const uint8_t*)a.src + (size_t)y * a.row_bytes) + (size_t)x * a.nch;
        T* d = (T*)a.dst + (size_t)y * a.ds + x;
        for (uint32_t k = 0; k < a.nch; ++k, d += a.plane) {
            if (whole) {
                uint32_t v[PIX], o[NO];
#pragma unroll
                for (int p = 0; p < PIX; ++p) v[p] = e[(size_t)p * a.nch + k];
#pragma unroll
                for (int j = 0; j < NO; ++j) {
                    if (sizeof(T) == 4) o[j] = v[j];
                    else if (sizeof(T) == 2) o[j] = v[2 * j] | v[2 * j + 1] << 16;
                    else o[j] = v[4 * j] | v[4 * j + 1] << 8 | v[4 * j + 2] << 16 | v[4 * j + 3] << 24;
                }
                store8<T>(d, o);
            } else {
#pragma unroll
                for (int p = 0; p < PIX; ++p)
                    if (p < (int)n) d[p] = e[(size_t)p * a.nch + k];
            }
        }
    }
}

template <typename T>
void launch_un(hipStream_t st, const GkUnpixArgs& a, dim3 grid) {
    switch (a.nch) {
        case 1: hipLaunchKernelGGL((k_unpixels<T, 1>), grid, dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL((k_unpixels<T, 2>), grid, dim3(256), 0, st, a); break;
        case 3: hipLaunchKernelGGL((k_unpixels<T, 3>), grid, dim3(256), 0, st, a); break;
        case 4: hipLaunchKernelGGL((k_unpixels<T, 4>), grid, dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL((k_unpixels_any<T>), grid, dim3(256), 0, st, a); break;
    }
}
}  // namespace

void gk_launch_unpixels(hipStream_t st, int es, const GkUnpixArgs& args) {
    GkUnpixArgs a = args;
    if (!a.w || !a.h || !a.nch || a.nch > GK_PIX_MAX_CH) return;
    a.rows = std::max(4u, (a.h + 65534) / 65535);   // (grid.y limit)
    const dim3 grid((a.w + 256 * PIX - 1) / (256 * PIX), (a.h + a.rows - 1) / a.rows);
    if (es == 1) launch_un<uint8_t>(st, a, grid);
    else if (es == 2) launch_un<uint16_t>(st, a, grid);
    else launch_un<uint32_t>(st, a, grid);
}
