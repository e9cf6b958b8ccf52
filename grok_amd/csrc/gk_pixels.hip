// gk_pixels.hip — the output stage of a decode: forced precision (grk_decompress -p), grey to RGB
// (-f) and packed (H, W, C) pixels, in one pass over the decoded planes.
//
// Replaces, on the device, the end of GrkDecompress::postProcess (bin/jp2/grk_decompress.cpp
// :1444-1494: convert_gray_to_rgb, clip_component / scale_component, bin/common/convert.cpp
// :96-207) and the planar-to-interleaved pass of Grok's image writers.
//
// Shape (gk_colour.hip's idiom).  A thread owns GK_PAL_PIX (8) consecutive pixels of a row and a
// workgroup 256 * 8 columns of `rows` rows.  Per source channel the thread issues one vector load
// of 8 samples (8, 16 or 32 bytes; the engine's planes are aligned for it); a channel that names
// the plane of the channel before it (grey to RGB) reuses the loaded registers.  The channel's
// operation is chosen by a descriptor in the kernel arguments, so the choice is a scalar branch
// taken by the whole wave.  The 8 * C results are packed in registers (v_perm_b32 for 8 / 16-bit
// samples) into the lane's 8 * C * es contiguous output bytes and leave in 16-, 8- or 4-byte
// stores, whichever the row's base address allows (uniform per row); lane i + 1 continues where
// lane i ends, so a wave writes one contiguous run of 512 * C * es bytes whatever C is.  A row
// of 8 / 16-bit pixels whose base is not dword-aligned (three rows in four of a tight odd-width
// (H, W, 3) u8 image) takes the bytes up to the boundary one by one, aligned dwords shifted
// together from neighbouring packed words, and the remaining bytes; the last, partial group of
// a row is stored sample by sample.  Every path writes the same values.  No LDS, no cross-lane
// traffic.
//
// Arithmetic of the scale (scale_component): lrintf((float)v * scale) is one float32 product,
// rounded to nearest even by v_cvt_i32_f32 under the default rounding mode (__float2int_rn);
// contraction is off in that function, though a lone product has nothing to contract with.  The
// division by 2^s truncates toward zero: negative samples are biased by 2^s - 1 before the
// arithmetic shift.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "gk_common.h"
#include "gk_launch.h"

namespace {
constexpr int PIX = GK_PAL_PIX;

template <typename T, int N> struct Vec { typedef T type __attribute__((ext_vector_type(N))); };
typedef uint32_t U4 __attribute__((ext_vector_type(4)));
typedef uint32_t U2 __attribute__((ext_vector_type(2)));

template <typename SRC> __device__ __forceinline__ void load8(const SRC* s, bool whole, uint32_t n, int32_t out[PIX]) {
    typedef typename Vec<SRC, PIX>::type SV;
    if (whole) {
        const SV v = *(const SV*)s;
#pragma unroll
        for (int p = 0; p < PIX; ++p) out[p] = (int32_t)v[p];
    } else {
#pragma unroll
        for (int p = 0; p < PIX; ++p) out[p] = p < (int)n ? (int32_t)s[p] : 0;
    }
}

// the channel's operation on the thread's 8 samples: c is wave-uniform (kernel arguments)
__device__ __forceinline__ void apply_op(const GkPixChan& c, int32_t v[PIX]) {
#pragma clang fp contract(off)
    if (c.op == GK_PIX_CLAMP) {
#pragma unroll
        for (int p = 0; p < PIX; ++p) v[p] = min(max(v[p], c.lo), c.hi);
    } else if (c.op == GK_PIX_SCALE) {
#pragma unroll
        for (int p = 0; p < PIX; ++p) {
            const float f = (float)v[p] * c.scale;
            v[p] = __float2int_rn(f);
        }
    } else if (c.op == GK_PIX_SHIFT) {
        const int32_t bias = (int32_t)((1u << c.shift) - 1u);
#pragma unroll
        for (int p = 0; p < PIX; ++p) v[p] = (v[p] + ((v[p] >> 31) & bias)) >> c.shift;
    }
}

// sample i (pixel i / C, channel i % C) of the lane's packed output
template <int C> __device__ __forceinline__ uint32_t samp(const int32_t (&v)[C][PIX], int i) { return (uint32_t)v[i % C][i / C]; }

// the lane's 8 * C samples as dwords of DST elements, in memory order (little endian)
template <typename DST, int C> __device__ __forceinline__ void pack(const int32_t (&v)[C][PIX], uint32_t (&o)[PIX * C * sizeof(DST) / 4]) {
    constexpr int NW = PIX * C * (int)sizeof(DST) / 4;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        if (sizeof(DST) == 4) {
            o[j] = samp<C>(v, j);
        } else if (sizeof(DST) == 2) {
            // bytes 0-1 of sample 2j, then bytes 0-1 of sample 2j + 1
            o[j] = __builtin_amdgcn_perm(samp<C>(v, 2 * j + 1), samp<C>(v, 2 * j), 0x05040100u);
        } else {
            // byte 0 of four samples: two byte pairs (upper half zero), then the two halves
            const uint32_t lo = __builtin_amdgcn_perm(samp<C>(v, 4 * j + 1), samp<C>(v, 4 * j), 0x0c0c0400u);
            const uint32_t hi = __builtin_amdgcn_perm(samp<C>(v, 4 * j + 3), samp<C>(v, 4 * j + 2), 0x0c0c0400u);
            o[j] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
        }
    }
}

// SRC: uint8_t / uint16_t / int32_t planes; DST: uint8_t / uint16_t / int32_t pixels (signed 8 /
// 16-bit pixels take the same bits); C: channels per pixel
template <typename SRC, typename DST, int C>
__global__ __launch_bounds__(256) void k_pixels(GkPixArgs a) {
    constexpr int LB = PIX * C * (int)sizeof(DST);   // the lane's output bytes per row
    constexpr int NW = LB / 4;
    const uint32_t x = (blockIdx.x * 256 + threadIdx.x) * PIX;
    if (x >= a.w) return;
    const bool whole = x + PIX <= a.w;
    const uint32_t n = whole ? PIX : a.w - x;
    const uint32_t y0 = blockIdx.y * a.rows, y1 = min(a.h, y0 + a.rows);
    for (uint32_t y = y0; y < y1; ++y) {
        int32_t v[C][PIX];
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const GkPixChan& c = a.ch[k];
            if (k > 0 && c.same_prev) {   // (uniform) the plane of channel k - 1: its registers
#pragma unroll
                for (int p = 0; p < PIX; ++p) v[k][p] = v[k > 0 ? k - 1 : 0][p];
            } else {
                load8<SRC>((const SRC*)c.src + (size_t)y * c.ss + x, whole, n, v[k]);
            }
        }
        // (operations after every load: a replicated channel copies the samples as loaded)
#pragma unroll
        for (int k = 0; k < C; ++k) apply_op(a.ch[k], v[k]);
        uint8_t* row = (uint8_t*)a.dst + (size_t)y * a.row_bytes;
        uint8_t* d = row + (size_t)x * C * sizeof(DST);
        const uint32_t mis = (uint32_t)(uintptr_t)row & 15u;   // uniform: the lane's offset is a multiple of 8
        if (whole && (mis & 3u) == 0) {
            uint32_t o[NW];
            pack<DST, C>(v, o);
            if (LB % 16 == 0 && mis == 0) {
#pragma unroll
                for (int j = 0; j < NW; j += 4) { U4 q = {o[j], o[j + 1], o[j + 2], o[j + 3]}; *(U4*)(d + 4 * j) = q; }
            } else if ((mis & 7u) == 0) {
#pragma unroll
                for (int j = 0; j < NW; j += 2) { U2 q = {o[j], o[j + 1]}; *(U2*)(d + 4 * j) = q; }
            } else {
#pragma unroll
                for (int j = 0; j < NW; ++j) *(uint32_t*)(d + 4 * j) = o[j];
            }
        } else if (whole && sizeof(DST) < 4) {
            // the row starts m = 1..3 bytes past a dword boundary (as every lane's run does): 4 - m
            // bytes reach the boundary, then NW - 1 dwords funnelled from neighbouring packed
            // words (v_alignbyte_b32), then the last m bytes
            uint32_t o[NW];
            pack<DST, C>(v, o);
            const uint32_t hb = 4u - (mis & 3u);
#pragma unroll
            for (int b = 0; b < 3; ++b)
                if (b < (int)hb) d[b] = (uint8_t)(o[0] >> (8 * b));
#pragma unroll
            for (int j = 0; j + 1 < NW; ++j) *(uint32_t*)(d + hb + 4 * j) = __builtin_amdgcn_alignbyte(o[j + 1], o[j], hb);
#pragma unroll
            for (int b = 0; b < 3; ++b)
                if (b < 4 - (int)hb) d[4 * (NW - 1) + hb + b] = (uint8_t)(o[NW - 1] >> (8 * (hb + b)));
        } else {
            DST* e = (DST*)d;
#pragma unroll
            for (int p = 0; p < PIX; ++p)
                if (p < (int)n) {
#pragma unroll
                    for (int k = 0; k < C; ++k) e[p * C + k] = (DST)v[k][p];
                }
        }
    }
}

// 5..16 channels: one channel at a time, samples stored one by one at the pixel stride
template <typename SRC, typename DST>
__global__ __launch_bounds__(256) void k_pixels_any(GkPixArgs a) {
    const uint32_t x = (blockIdx.x * 256 + threadIdx.x) * PIX;
    if (x >= a.w) return;
    const bool whole = x + PIX <= a.w;
    const uint32_t n = whole ? PIX : a.w - x;
    const uint32_t y0 = blockIdx.y * a.rows, y1 = min(a.h, y0 + a.rows);
    for (uint32_t y = y0; y < y1; ++y) {
        DST* e = (DST*)((uint8_t*)a.dst + (size_t)y * a.row_bytes) + (size_t)x * a.nch;
        for (uint32_t k = 0; k < a.nch; ++k) {
            const GkPixChan& c = a.ch[k];
            int32_t v[PIX];
            load8<SRC>((const SRC*)c.src + (size_t)y * c.ss + x, whole, n, v);
            apply_op(c, v);
#pragma unroll
            for (int p = 0; p < PIX; ++p)
                if (p < (int)n) e[(size_t)p * a.nch + k] = (DST)v[p];
        }
    }
}

template <typename SRC, typename DST>
void launch_c(hipStream_t st, const GkPixArgs& a, dim3 grid) {
    switch (a.nch) {
        case 1: hipLaunchKernelGGL((k_pixels<SRC, DST, 1>), grid, dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL((k_pixels<SRC, DST, 2>), grid, dim3(256), 0, st, a); break;
        case 3: hipLaunchKernelGGL((k_pixels<SRC, DST, 3>), grid, dim3(256), 0, st, a); break;
        case 4: hipLaunchKernelGGL((k_pixels<SRC, DST, 4>), grid, dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL((k_pixels_any<SRC, DST>), grid, dim3(256), 0, st, a); break;
    }
}
#define GK_PIX_TYPE(t, T, ...)                                    \
    if ((t) == GK_U8) { typedef uint8_t T; __VA_ARGS__; }         \
    else if ((t) == GK_U16) { typedef uint16_t T; __VA_ARGS__; }  \
    else { typedef int32_t T; __VA_ARGS__; }
}  // namespace

void gk_launch_pixels(hipStream_t st, int stype, int dtype, const GkPixArgs& args) {
    GkPixArgs a = args;
    if (!a.w || !a.h || !a.nch || a.nch > GK_PIX_MAX_CH) return;
    a.rows = std::max(4u, (a.h + 65534) / 65535);   // (grid.y limit)
    const dim3 grid((a.w + 256 * PIX - 1) / (256 * PIX), (a.h + a.rows - 1) / a.rows);
    GK_PIX_TYPE(stype, S, GK_PIX_TYPE(dtype, D, launch_c<S, D>(st, a, grid)))
}
