// gk_view.hip — the last stage of gk_decode_view_pixels: the decoded region, rw x rh packed int32
// pixels on the reduced canvas, resampled to exactly ow x oh pixels, mirrored and rotated, and
// written as the caller's packed pixels.
//
// The rule (tests/view_ref.py is the same arithmetic in numpy) is an exact area
// average in integers; gk_area.h states it and holds its one definition.
//
// Shape.  A 256-thread block owns a 16 x 16 tile of the output in pre-rotation coordinates, so its
// source footprint is one compact rectangle (at the reduce level the engine chooses a pixel's span
// is at most 3 x 3 source samples; a stream that ran out of resolutions only makes the loops run
// longer).  The lanes of a 16-lane group run along the axis that becomes the written image's x:
// the tile's columns for rotate 0 / 180, its rows for 90 / 270.  Either way a group's stores are
// one contiguous run of 16 pixels and the block's stores one compact 16 x 16 tile of the written
// image.  For 90 / 270 the loads of a group then walk down 16 output rows; the lines they touch
// are the ones the block's other groups read (the same compact footprint), so they are served by
// the CU's vector L1.  That is why there is no LDS transpose here: it would trade those L1 hits for
// LDS traffic and a barrier in a pass that moves far fewer bytes than the decode in front of it.
// This was decided from the code, not measured.
//
// A lane accumulates four channels at a time (all of them up to RGBA; 5..16 channels walk the
// footprint once per group of four) and stores DST samples at the mirrored / rotated position.
// Every source index is checked against rw / rh and every written position against pix_w / pix_h.
// No atomics, no LDS, no inline assembly.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gk_common.h"
#include "gk_launch.h"
#include "gk_area.h"

namespace {
constexpr int TILE = GK_AREA_TILE;
constexpr int CG = GK_AREA_CG;   // channels accumulated per walk over the footprint

template <typename DST>
__global__ __launch_bounds__(256) void k_view(GkViewArgs a) {
    const uint32_t lo = threadIdx.x & (TILE - 1), hi = threadIdx.x >> 4;
    // the fast lane index along the written image's x
    const uint32_t bx = blockIdx.x % a.tiles_x, by = blockIdx.x / a.tiles_x;
    const uint32_t i = bx * TILE + (a.swap ? hi : lo);   // output column before orientation
    const uint32_t j = by * TILE + (a.swap ? lo : hi);   // output row before orientation
    if (i >= a.ow || j >= a.oh) return;
    // orientation: mirror left-right, then rotate clockwise
    const uint32_t im = a.mirror ? a.ow - 1 - i : i;
    uint32_t px, py;
    switch (a.rot) {
        case 1: px = a.oh - 1 - j; py = im; break;              // 90
        case 2: px = a.ow - 1 - im; py = a.oh - 1 - j; break;   // 180
        case 3: px = j; py = a.ow - 1 - im; break;              // 270
        default: px = im; py = j; break;
    }
    if (px >= a.pix_w || py >= a.pix_h) return;
    DST* d = (DST*)((uint8_t*)a.dst + (size_t)py * a.row_bytes) + (size_t)px * a.nch;
    const int32_t* src = (const int32_t*)a.src;
    const uint32_t C = a.nch;
    if (a.rw == a.ow && a.rh == a.oh) {   // (uniform) equal sizes copy the samples
        const int32_t* s = src + ((size_t)j * a.rw + i) * C;
        for (uint32_t k = 0; k < C; ++k) d[k] = (DST)s[k];
        return;
    }
    // the spans, the weights and the rounding: gk_area.h, shared with k_render and k_levels
    const GkAreaSpan p = gk_area_span(a.rw, a.rh, a.ow, a.oh, i, j);
    for (uint32_t c0 = 0; c0 < C; c0 += CG) {
        int64_t acc[CG];
        gk_area_sum(src, p, a.rw, a.ow, a.oh, C, c0, acc);
#pragma unroll
        for (int k = 0; k < CG; ++k)
            if (c0 + k < C) d[c0 + k] = (DST)gk_round_div(acc[k], p.den);
    }
}
}  // namespace

int gk_launch_view(hipStream_t st, int dtype, const GkViewArgs& args) {
    GkViewArgs a = args;
    if (!a.ow || !a.oh || !a.rw || !a.rh || !a.nch || a.nch > GK_PIX_MAX_CH || a.ow > a.rw || a.oh > a.rh || a.rot > 3) return -1;
    a.swap = a.rot & 1;
    a.pix_w = a.swap ? a.oh : a.ow;
    a.pix_h = a.swap ? a.ow : a.oh;
    a.tiles_x = (a.ow + TILE - 1) / TILE;
    const uint64_t tiles = (uint64_t)a.tiles_x * ((a.oh + TILE - 1) / TILE);   // (one grid axis: no 65535-row limit)
    if (tiles > GK_VIEW_MAX_TILES) return -1;
    const dim3 grid((uint32_t)tiles);
    if (dtype == GK_U8) hipLaunchKernelGGL((k_view<uint8_t>), grid, dim3(256), 0, st, a);
    else if (dtype == GK_U16) hipLaunchKernelGGL((k_view<uint16_t>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_view<int32_t>), grid, dim3(256), 0, st, a);
    return 0;
}
