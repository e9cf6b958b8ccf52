// gk_render.hip — the display stage of the pixel calls (gk_set_decode_render) and the statistics
// of a view (gk_decode_levels).  Both start from what k_view starts from: rw x rh packed int32
// pixels on the reduced canvas in the engine's own buffer, resampled to ow x oh by the exact area
// average of gk_area.h (the one definition k_view uses too).
//
// k_render.  The geometry of k_view: a 256-thread block owns a 16 x 16 tile of the output in
// pre-rotation coordinates and the lanes of a 16-lane group run along the axis that becomes the
// written image's x (gk_view.hip explains why).  A lane computes the area-averaged int32 of four
// channels at a time, then the rule of DESIGN.md §3 (tests/render_ref.py is the same arithmetic in
// numpy), all in 64-bit integers:
//     u = clamp(v, lo, hi),  t = floor((2 * 255 (u - lo) + (hi - lo)) / (2 (hi - lo)))      lo < hi
//     inverted window: t = 255 - t;   curve: t = curve[t]
//     WINDOW: out_k = t_k    MAP: out_c = map[3 t + c]    BLEND: out_c = min(255, (2 sum_k t_k tint_k,c + 255) / 510)
// u - lo < 2^32, so the numerator stays below 2^42 and the division is unsigned.  The curve (256
// bytes) and the map (768) are read-only and shared by every lane: a block copies them from the
// engine's device blob into LDS once, one dword a lane, and every lookup is an LDS byte read.
// The per-channel windows and tints are kernel arguments.  Output is always unsigned 8-bit; every
// source index is checked against rw / rh and every written position against pix_w / pix_h.
//
// k_levels.  The same footprint walk.  Per pixel and channel the int32 the view would return goes
// into (a) min / max / sum, folded across the wave with shuffles, across the block's four waves
// through LDS, and added to the global result by one lane a channel (at most one vector atomic
// per block and quantity; a min or max the result has already passed issues none: with the
// atomics issued per wave the pass over 1024 x 1024 pixels measured 0.57 ms, folded per block
// 0.17 ms), and (b) an
// LDS-private histogram of uint32 counters, at most 4 channels x 4096 bins = 64 KiB a block (two
// blocks share a CU's 160 KiB); more channels walk the footprint again, as k_view's loop does.  A
// block holds 256 pixels, so a counter cannot wrap.  After a barrier the block adds its non-zero
// bins to the engine's uint64 histogram with 64-bit global atomics.  A constant image puts every
// increment of a block on one LDS address: that is correct (LDS atomics serialise) and its cost is
// measured, not guessed (profiles/render_bench.txt).  No lane leaves before the last barrier.
// Plain HIP C++, no inline assembly.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "gk_common.h"
#include "gk_launch.h"
#include "gk_area.h"

namespace {
constexpr int TILE = GK_AREA_TILE;
constexpr int CG = GK_AREA_CG;

// the tile's pixel of this lane before orientation; false: outside the output
__device__ __forceinline__ bool tile_pixel(const GkViewArgs& a, uint32_t& i, uint32_t& j) {
    const uint32_t lo = threadIdx.x & (TILE - 1), hi = threadIdx.x >> 4;
    const uint32_t bx = blockIdx.x % a.tiles_x, by = blockIdx.x / a.tiles_x;
    i = bx * TILE + (a.swap ? hi : lo);
    j = by * TILE + (a.swap ? lo : hi);
    return i < a.ow && j < a.oh;
}

// the window of DESIGN.md §3: lo < hi
__device__ __forceinline__ uint32_t level(int32_t v, const GkRenderChan& c) {
    const int64_t u = min(max((int64_t)v, (int64_t)c.lo), (int64_t)c.hi);
    const uint64_t span = (uint64_t)((int64_t)c.hi - (int64_t)c.lo);
    const uint64_t num = 510ull * (uint64_t)(u - (int64_t)c.lo) + span;
    const uint32_t t = (uint32_t)(num / (2 * span));
    return c.inv ? 255u - t : t;
}

__global__ __launch_bounds__(256) void k_render(GkRenderArgs r) {
    __shared__ uint32_t tab32[GK_RENDER_TABLE_BYTES / 4];
    const GkViewArgs& a = r.v;
    {   // the tables, once a block: the curve's 64 dwords, the map's 192
        const uint32_t w = threadIdx.x;
        const bool need = w < 64 ? r.has_curve != 0 : r.mode == GK_RMODE_MAP;
        if (need) tab32[w] = ((const uint32_t*)r.tables)[w];
    }
    __syncthreads();
    const uint8_t* curve = (const uint8_t*)tab32;
    const uint8_t* map = curve + 256;
    uint32_t i, j;
    if (!tile_pixel(a, i, j)) return;   // (after the block's only barrier)
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
    uint8_t* d = (uint8_t*)a.dst + (size_t)py * a.row_bytes + (size_t)px * r.out_ch;
    const int32_t* src = (const int32_t*)a.src;
    const uint32_t C = a.nch;
    uint32_t sum[3] = {0, 0, 0};   // BLEND: at most 16 * 255 * 255
    for (uint32_t c0 = 0; c0 < C; c0 += CG) {
        int32_t v[CG];
        gk_area_pixel(src, a.rw, a.rh, a.ow, a.oh, C, i, j, c0, v);
#pragma unroll
        for (int k = 0; k < CG; ++k) {
            if (c0 + k >= C) continue;
            const GkRenderChan& ch = r.ch[c0 + k];
            uint32_t t = level(v[k], ch);
            if (r.has_curve) t = curve[t];
            if (r.mode == GK_RMODE_WINDOW) {
                d[c0 + k] = (uint8_t)t;
            } else if (r.mode == GK_RMODE_MAP) {
                d[0] = map[3 * t]; d[1] = map[3 * t + 1]; d[2] = map[3 * t + 2];
            } else {
                sum[0] += t * ch.tint[0]; sum[1] += t * ch.tint[1]; sum[2] += t * ch.tint[2];
            }
        }
    }
    if (r.mode == GK_RMODE_BLEND) {
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = (uint8_t)min(255u, (2 * sum[c] + 255u) / 510u);
    }
}

__device__ __forceinline__ int32_t wave_min(int32_t v) {
    for (int o = warpSize / 2; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int32_t wave_max(int32_t v) {
    for (int o = warpSize / 2; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
    for (int o = warpSize / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the block's partial results of one channel group: a wave's leader writes its wave's, then lane k
// of the block folds channel k's.  It lives at the start of the dynamic LDS, before the histogram
// of the same group is zeroed over it.
struct LevelsPartial {
    long long sum[4][CG];   // [wave][channel]
    int32_t mn[4][CG], mx[4][CG];
};

__global__ __launch_bounds__(256) void k_levels(GkLevelsArgs q) {
    extern __shared__ __align__(8) uint32_t lds_hist[];   // max(sizeof(LevelsPartial), min(nch, CG) * bins counters)
    LevelsPartial* part = (LevelsPartial*)lds_hist;
    const GkViewArgs& a = q.v;
    uint32_t i, j;
    const bool valid = tile_pixel(a, i, j);
    const int32_t* src = (const int32_t*)a.src;
    const uint32_t C = a.nch, bins = q.bins;
    const uint32_t wave = threadIdx.x / warpSize;
    const bool leader = (threadIdx.x & (warpSize - 1)) == 0;
    for (uint32_t c0 = 0; c0 < C; c0 += CG) {
        const uint32_t ng = min((uint32_t)CG, C - c0);
        int32_t v[CG] = {0, 0, 0, 0};
        if (valid) gk_area_pixel(src, a.rw, a.rh, a.ow, a.oh, C, i, j, c0, v);
        if (c0) __syncthreads();   // the flush of the group before
        // min / max / sum: across the wave with shuffles, across the block through LDS, then one lane
        // a channel adds the block's to the global result
#pragma unroll
        for (int k = 0; k < CG; ++k) {
            if ((uint32_t)k >= ng) continue;   // (uniform)
            const int32_t mn = wave_min(valid ? v[k] : INT32_MAX);
            const int32_t mx = wave_max(valid ? v[k] : INT32_MIN);
            const long long sm = wave_sum(valid ? (long long)v[k] : 0);
            if (leader) { part->mn[wave][k] = mn; part->mx[wave][k] = mx; part->sum[wave][k] = sm; }
        }
        __syncthreads();
        if (threadIdx.x < ng) {
            const uint32_t k = threadIdx.x;
            int32_t mn = part->mn[0][k], mx = part->mx[0][k];
            long long sm = part->sum[0][k];
            for (int w = 1; w < 4; ++w) { mn = min(mn, part->mn[w][k]); mx = max(mx, part->mx[w][k]); sm += part->sum[w][k]; }
            GkLevelsStat* s = q.stats + c0 + k;
            // min only falls and max only rises, so a value already passed (even a stale read of
            // it) needs no atomic: after the first blocks almost none is issued
            if (mn < __hip_atomic_load(&s->min, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&s->min, mn);
            if (mx > __hip_atomic_load(&s->max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&s->max, mx);
            atomicAdd(&s->sum, (unsigned long long)sm);
        }
        if (!bins) continue;   // (uniform)
        __syncthreads();       // the partials are read
        for (uint32_t e = threadIdx.x; e < ng * bins; e += 256) lds_hist[e] = 0;
        __syncthreads();
        if (valid) {
#pragma unroll
            for (int k = 0; k < CG; ++k) {
                if ((uint32_t)k >= ng) continue;
                const int64_t b = ((int64_t)v[k] - (int64_t)q.origin[c0 + k]) >> q.shift[c0 + k];   // floor
                atomicAdd(&lds_hist[(uint32_t)k * bins + (uint32_t)min(max(b, (int64_t)0), (int64_t)bins - 1)], 1u);
            }
        }
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < ng * bins; e += 256) {
            const uint32_t n = lds_hist[e];
            if (n) atomicAdd(q.hist + (size_t)c0 * bins + e, (unsigned long long)n);
        }
    }
}

// the launcher's part of GkViewArgs, as gk_launch_view sets it; false: the arguments break the rules
bool view_geometry(GkViewArgs& a, uint64_t& tiles) {
    if (!a.ow || !a.oh || !a.rw || !a.rh || !a.nch || a.nch > GK_PIX_MAX_CH || a.ow > a.rw || a.oh > a.rh || a.rot > 3) return false;
    a.swap = a.rot & 1;
    a.pix_w = a.swap ? a.oh : a.ow;
    a.pix_h = a.swap ? a.ow : a.oh;
    a.tiles_x = (a.ow + TILE - 1) / TILE;
    tiles = (uint64_t)a.tiles_x * ((a.oh + TILE - 1) / TILE);   // (one grid axis: no 65535-row limit)
    return tiles <= GK_VIEW_MAX_TILES;
}
}  // namespace

int gk_launch_render(hipStream_t st, const GkRenderArgs& args) {
    GkRenderArgs r = args;
    uint64_t tiles = 0;
    if (!view_geometry(r.v, tiles)) return -1;
    if (r.mode < GK_RMODE_WINDOW || r.mode > GK_RMODE_BLEND || (r.mode == GK_RMODE_MAP && r.v.nch != 1)) return -1;
    if ((r.has_curve || r.mode == GK_RMODE_MAP) && (!r.tables || ((uintptr_t)r.tables & 3))) return -1;
    for (uint32_t k = 0; k < r.v.nch; ++k)
        if (r.ch[k].lo >= r.ch[k].hi) return -1;
    r.out_ch = r.mode == GK_RMODE_WINDOW ? r.v.nch : 3;
    hipLaunchKernelGGL(k_render, dim3((uint32_t)tiles), dim3(256), 0, st, r);
    return 0;
}

int gk_launch_levels(hipStream_t st, const GkLevelsArgs& args) {
    GkLevelsArgs q = args;
    uint64_t tiles = 0;
    q.v.rot = 0; q.v.mirror = 0;
    if (!view_geometry(q.v, tiles)) return -1;
    if (!q.stats || q.bins > GK_LEVELS_BINS_MAX || (q.bins && !q.hist)) return -1;
    for (uint32_t k = 0; k < q.v.nch; ++k)
        if (q.shift[k] > 31) return -1;
    const size_t lds = std::max(sizeof(LevelsPartial), (size_t)std::min<uint32_t>(q.v.nch, CG) * q.bins * sizeof(uint32_t));   // <= 64 KiB
    if (lds > 32768 && hipFuncSetAttribute((const void*)k_levels, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_levels, dim3((uint32_t)tiles), dim3(256), lds, st, q);
    return 0;
}
