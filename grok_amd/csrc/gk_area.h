// gk_area.h — the view's exact area average (tests/view_ref.py), the one definition
// that k_view (gk_view.hip) and k_render / k_levels (gk_render.hip) share.
//
// The source holds rw x rh packed int32 pixels of C channels, rows rw * C samples apart.  In units
// of 1 / ow a source column is ow long and an output column rw: output column i covers
// [i rw, (i + 1) rw), source column s covers [s ow, (s + 1) ow), and the weight wx(i, s) is the
// length of their overlap; rows alike with rh and oh.  A column's weights sum to rw and a row's to
// rh, so
//     out = floor((2 sum(wy wx v) + rw rh) / (2 rw rh))
// per channel in signed 64-bit integers: floor division, halves round up.  The engine refuses a
// source with (rw rh) << prec >= 2^62, so 2 sum + rw rh stays inside an int64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int GK_AREA_TILE = 16;   // a 256-thread block owns a 16 x 16 tile of the output before orientation
constexpr int GK_AREA_CG = 4;      // channels accumulated per walk over a pixel's footprint

// floor((2 a + d) / (2 d)), d > 0
__device__ __forceinline__ int64_t gk_round_div(int64_t a, int64_t d) {
    const int64_t num = 2 * a + d, den = 2 * d;
    int64_t q = num / den;
    if (num - q * den < 0) --q;
    return q;
}

// The footprint of output pixel (i, j): source columns [s0, s1] and rows [t0, t1] overlap it
struct GkAreaSpan {
    uint64_t xa, xb, ya, yb;
    uint32_t s0, s1, t0, t1;
    int64_t den;   // rw rh
};
__device__ __forceinline__ GkAreaSpan gk_area_span(uint32_t rw, uint32_t rh, uint32_t ow, uint32_t oh, uint32_t i, uint32_t j) {
    GkAreaSpan p;
    p.xa = (uint64_t)i * rw; p.xb = p.xa + rw; p.ya = (uint64_t)j * rh; p.yb = p.ya + rh;
    p.s0 = (uint32_t)(p.xa / ow); p.s1 = min((uint32_t)((p.xb - 1) / ow), rw - 1);
    p.t0 = (uint32_t)(p.ya / oh); p.t1 = min((uint32_t)((p.yb - 1) / oh), rh - 1);
    p.den = (int64_t)((uint64_t)rw * rh);
    return p;
}
// acc[k] = sum(wy wx v) of channel c0 + k over the footprint, k < GK_AREA_CG and c0 + k < C
__device__ __forceinline__ void gk_area_sum(const int32_t* src, const GkAreaSpan& p, uint32_t rw, uint32_t ow, uint32_t oh, uint32_t C,
                                            uint32_t c0, int64_t acc[GK_AREA_CG]) {
#pragma unroll
    for (int k = 0; k < GK_AREA_CG; ++k) acc[k] = 0;
    for (uint32_t t = p.t0; t <= p.t1; ++t) {
        const uint64_t ta = (uint64_t)t * oh;
        const int64_t wy = (int64_t)(min(p.yb, ta + oh) - max(p.ya, ta));
        const int32_t* row = src + (size_t)t * rw * C + c0;
        int64_t racc[GK_AREA_CG] = {0, 0, 0, 0};
        for (uint32_t s = p.s0; s <= p.s1; ++s) {
            const uint64_t sa = (uint64_t)s * ow;
            const int64_t wx = (int64_t)(min(p.xb, sa + ow) - max(p.xa, sa));
            const int32_t* q = row + (size_t)s * C;
#pragma unroll
            for (int k = 0; k < GK_AREA_CG; ++k)
                if (c0 + k < C) racc[k] += wx * (int64_t)q[k];
        }
#pragma unroll
        for (int k = 0; k < GK_AREA_CG; ++k) acc[k] += wy * racc[k];
    }
}
// The int32 samples of channels c0 .. c0 + 3 of output pixel (i, j), as the view returns them:
// equal sizes copy the samples, anything else is the rounded area average
__device__ __forceinline__ void gk_area_pixel(const int32_t* src, uint32_t rw, uint32_t rh, uint32_t ow, uint32_t oh, uint32_t C,
                                              uint32_t i, uint32_t j, uint32_t c0, int32_t v[GK_AREA_CG]) {
    if (rw == ow && rh == oh) {   // (uniform)
        const int32_t* s = src + ((size_t)j * rw + i) * C + c0;
#pragma unroll
        for (int k = 0; k < GK_AREA_CG; ++k) v[k] = (c0 + k < C) ? s[k] : 0;
        return;
    }
    const GkAreaSpan p = gk_area_span(rw, rh, ow, oh, i, j);
    int64_t acc[GK_AREA_CG];
    gk_area_sum(src, p, rw, ow, oh, C, c0, acc);
#pragma unroll
    for (int k = 0; k < GK_AREA_CG; ++k) v[k] = (c0 + k < C) ? (int32_t)gk_round_div(acc[k], p.den) : 0;
}
