// gk_icc.hip — colour management of the display stage: a JP2 file's ICC profile and the CIELab
// enumerated space to sRGB, on the device.
//
// k_icc_rgb  color_apply_icc_profile (bin/common/color.cpp:423-776) for the two profile classes
//            Part 1 allows in a colr box: v / (2^p - 1) -> tone curve -> 3 x 3 matrix -> clip to
//            [0, 1] -> sRGB encoding -> * (2^p - 1), rounded half up, at the image's precision p.
//            A grey profile is the curve and the encoding alone (its R = G = B).
// k_lab_rgb  color_cielab_to_rgb (:779-964): L*a*b* samples through their ranges and offsets to
//            CIELab, to XYZ under D50, to sRGB at 16 bits.
//
// Both are per-pixel maps of the k_ycc_rgb family (gk_colour.hip): a thread owns GK_PAL_PIX
// consecutive samples of a row, loaded as one vector from the engine's aligned planes and stored
// as one vector where the caller's rows are aligned, sample by sample in the last, partial
// vector of a row; every plane is read once and written once.
//
// Curves.  Samples of up to 8 bits index a linearisation table of 2^p entries per channel that
// the host builds from the profile's curves.  Wider samples evaluate the curve: a parametric one
// in registers, a `curv` table by lcms2's 16-bit fixed-point interpolation (integer arithmetic,
// the same on the host, here and in the tests' restatement).  All tables of a launch are one array,
// staged in LDS by every workgroup when it is at most GK_ICC_LDS_BYTES and read from global
// memory (L2-resident) otherwise.
//
// Arithmetic.  float32 up to GK_ICC_FLOAT_PREC bits, double above: the result is compared with a
// float64 restatement sample by sample, and float32's error of a few units in the last place of
// 2^p stays inside a band of 2^(p - 19) LSB around the rounding ties only up to about 12 bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "gk_common.h"
#include "gk_launch.h"

namespace {
constexpr int PIX = GK_PAL_PIX;

template <typename T, int N> struct Vec { typedef T type __attribute__((ext_vector_type(N))); };

template <typename SRC> __device__ __forceinline__ void load_row(const SRC* s, bool whole, uint32_t n, int32_t out[PIX]) {
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
template <typename DST> __device__ __forceinline__ void store_row(DST* d, bool vec, uint32_t n, const int32_t v[PIX]) {
    typedef typename Vec<DST, PIX>::type DV;
    if (vec) {
        DV o;
#pragma unroll
        for (int p = 0; p < PIX; ++p) o[p] = (DST)v[p];
        *(DV*)d = o;
    } else {
#pragma unroll
        for (int p = 0; p < PIX; ++p) if (p < (int)n) d[p] = (DST)v[p];
    }
}

__device__ __forceinline__ float gpow(float x, float y) { return powf(x, y); }
__device__ __forceinline__ double gpow(double x, double y) { return pow(x, y); }
// clip to [0, 1] (a NaN becomes 0), the sRGB encoding, and the level at `vmax`, rounded half up
template <typename R> __device__ __forceinline__ int32_t srgb_level(R v, R vmax) {
    v = v > (R)0 ? v : (R)0;
    v = v < (R)1 ? v : (R)1;
    const R e = v <= (R)0.0031308 ? (R)12.92 * v : (R)1.055 * gpow(v, (R)(1.0 / 2.4)) - (R)0.055;
    const int32_t q = (int32_t)(e * vmax + (R)0.5);
    return min(max(q, 0), (int32_t)vmax);
}
template <typename R> __device__ __forceinline__ R curve(const GkIccChan& c, const R* tab, int32_t v, int32_t imax, R vmax) {
    v = min(max(v, 0), imax);
    if (c.kind == GK_ICC_LUT) return tab[c.off + min((uint32_t)v, c.n - 1)];
    const R x = (R)v / vmax;
    if (c.kind == GK_ICC_IDENTITY) return x;
    if (c.kind == GK_ICC_PARA) return x >= (R)c.d ? gpow((R)c.a * x + (R)c.b, (R)c.g) + (R)c.e : (R)c.c * x + (R)c.f;
    // a `curv` table, read as lcms2 reads it (LinLerp1D, cmsintrp.c; GkIccCurve::lerp16): the sample as a
    // 16-bit word rounded half up, fixed-point interpolation between the 16-bit entries, a 16-bit result
    const uint32_t in = (uint32_t)((2ull * (uint32_t)v * 65535ull + (uint32_t)imax) / (2ull * (uint32_t)imax));
    uint32_t out;
    if (in == 0xffffu) {
        out = (uint32_t)tab[c.off + c.n - 1];
    } else {
        uint32_t v3 = (c.n - 1) * in;
        v3 = v3 + (v3 + 0x7fffu) / 0xffffu;
        const uint32_t cell = min(v3 >> 16, c.n - 2), rest = v3 & 0xffffu;
        const uint32_t y0 = (uint32_t)tab[c.off + cell], y1 = (uint32_t)tab[c.off + cell + 1];
        out = ((((y1 - y0) * rest + 0x8000u) >> 16) + y0) & 0xffffu;
    }
    return (R)out / (R)65535;
}

template <typename SRC, typename DST, typename R, bool LDS>
__global__ __launch_bounds__(256) void k_icc_rgb(GkIccArgs a) {
    extern __shared__ double lds_raw[];
    const R* tab = (const R*)a.table;
    if (LDS) {
        R* l = (R*)lds_raw;
        for (uint32_t i = threadIdx.x; i < a.table_elems; i += 256) l[i] = tab[i];
        __syncthreads();
        tab = l;
    }
    const uint32_t x = (blockIdx.x * 256 + threadIdx.x) * PIX;
    if (x >= a.w) return;
    const bool whole = x + PIX <= a.w;
    const uint32_t n = whole ? PIX : a.w - x;
    const bool vst = whole && a.vec_store;
    const int32_t imax = (int32_t)((1u << a.prec) - 1);
    const R vmax = (R)imax;
    const uint32_t y0 = blockIdx.y * a.rows, y1 = min(a.h, y0 + a.rows);
    for (uint32_t y = y0; y < y1; ++y) {
        int32_t v[3][PIX];
        if (a.nch == 1) {
            load_row<SRC>((const SRC*)a.src[0] + (size_t)y * a.ss[0] + x, whole, n, v[0]);
            for (int p = 0; p < PIX; ++p) v[0][p] = srgb_level<R>(curve<R>(a.ch[0], tab, v[0][p], imax, vmax), vmax);
            store_row<DST>((DST*)a.dst[0] + (size_t)y * a.ds[0] + x, vst, n, v[0]);
            continue;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) load_row<SRC>((const SRC*)a.src[k] + (size_t)y * a.ss[k] + x, whole, n, v[k]);
        for (int p = 0; p < PIX; ++p) {
            R lin[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) lin[k] = curve<R>(a.ch[k], tab, v[k][p], imax, vmax);
#pragma unroll
            for (int k = 0; k < 3; ++k)
                v[k][p] = srgb_level<R>((R)a.m[k][0] * lin[0] + (R)a.m[k][1] * lin[1] + (R)a.m[k][2] * lin[2], vmax);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) store_row<DST>((DST*)a.dst[k] + (size_t)y * a.ds[k] + x, vst, n, v[k]);
    }
}

// lcms2's D50 white (cmsD50_XYZ)
__constant__ double LAB_WHITE[3] = {0.9642, 1.0, 0.8249};
__device__ __forceinline__ double lab_f1(double t) {
    return t <= 24.0 / 116.0 ? (108.0 / 841.0) * (t - 16.0 / 116.0) : t * t * t;
}
template <typename SRC, typename DST>
__global__ __launch_bounds__(256) void k_lab_rgb(GkLabArgs a) {
    const uint32_t x = (blockIdx.x * 256 + threadIdx.x) * PIX;
    if (x >= a.w) return;
    const bool whole = x + PIX <= a.w;
    const uint32_t n = whole ? PIX : a.w - x;
    const bool vst = whole && a.vec_store;
    const uint32_t y0 = blockIdx.y * a.rows, y1 = min(a.h, y0 + a.rows);
    for (uint32_t y = y0; y < y1; ++y) {
        int32_t v[3][PIX];
#pragma unroll
        for (int k = 0; k < 3; ++k) load_row<SRC>((const SRC*)a.src[k] + (size_t)y * a.ss[k] + x, whole, n, v[k]);
        for (int p = 0; p < PIX; ++p) {
            double lab[3], xyz[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) lab[k] = a.lo[k] + (double)v[k][p] * a.range[k] / a.vmax;
            const double fy = (lab[0] + 16.0) / 116.0;
            xyz[0] = lab_f1(fy + 0.002 * lab[1]) * LAB_WHITE[0];
            xyz[1] = lab_f1(fy) * LAB_WHITE[1];
            xyz[2] = lab_f1(fy - 0.005 * lab[2]) * LAB_WHITE[2];
#pragma unroll
            for (int k = 0; k < 3; ++k)
                v[k][p] = srgb_level<double>(a.m[k][0] * xyz[0] + a.m[k][1] * xyz[1] + a.m[k][2] * xyz[2], 65535.0);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) store_row<DST>((DST*)a.dst[k] + (size_t)y * a.ds[k] + x, vst, n, v[k]);
    }
}

inline uint32_t rows_per_group(uint32_t units) { return std::max(4u, (units + 65534) / 65535); }   // (grid.y limit)

#define GK_ICC_TYPE(t, T, ...)                                    \
    if ((t) == GK_U8) { typedef uint8_t T; __VA_ARGS__; }         \
    else if ((t) == GK_U16) { typedef uint16_t T; __VA_ARGS__; }  \
    else { typedef int32_t T; __VA_ARGS__; }

template <typename S, typename D>
void launch_icc(hipStream_t st, const GkIccArgs& a, dim3 grid, bool dbl, size_t lds) {
    if (dbl) {
        if (lds) hipLaunchKernelGGL((k_icc_rgb<S, D, double, true>), grid, dim3(256), lds, st, a);
        else hipLaunchKernelGGL((k_icc_rgb<S, D, double, false>), grid, dim3(256), 0, st, a);
    } else {
        if (lds) hipLaunchKernelGGL((k_icc_rgb<S, D, float, true>), grid, dim3(256), lds, st, a);
        else hipLaunchKernelGGL((k_icc_rgb<S, D, float, false>), grid, dim3(256), 0, st, a);
    }
}
}  // namespace

int gk_launch_icc_rgb(hipStream_t st, int stype, int dtype, const GkIccArgs& args) {
    GkIccArgs a = args;
    if (!a.w || !a.h || (a.nch != 1 && a.nch != 3) || !a.prec || a.prec > 16) return 0;
    const bool dbl = a.prec > GK_ICC_FLOAT_PREC;
    const size_t bytes = (size_t)a.table_elems * (dbl ? 8 : 4);
    const size_t lds = (bytes && bytes <= GK_ICC_LDS_BYTES) ? bytes : 0;
    // rows per workgroup: enough samples behind one table staging
    a.rows = lds ? std::max<uint32_t>(8, (uint32_t)(bytes / 1024)) : 4;
    a.rows = std::max(a.rows, rows_per_group(a.h));
    const dim3 grid((a.w + 256 * PIX - 1) / (256 * PIX), (a.h + a.rows - 1) / a.rows);
    GK_ICC_TYPE(stype, S, GK_ICC_TYPE(dtype, D, launch_icc<S, D>(st, a, grid, dbl, lds)))
    return lds ? 1 : 0;
}

void gk_launch_lab_rgb(hipStream_t st, int stype, int dtype, const GkLabArgs& args) {
    GkLabArgs a = args;
    if (!a.w || !a.h) return;
    a.rows = rows_per_group(a.h);
    const dim3 grid((a.w + 256 * PIX - 1) / (256 * PIX), (a.h + a.rows - 1) / a.rows);
    GK_ICC_TYPE(stype, S, GK_ICC_TYPE(dtype, D, hipLaunchKernelGGL((k_lab_rgb<S, D>), grid, dim3(256), 0, st, a)))
}
