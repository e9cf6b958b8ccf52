// gk_colour.hip — JP2 palette expansion on decode (pclr + cmap boxes), and the display stage
// (sYCC / e-sYCC / CMYK to RGB, chroma upsampling: second half of the file).
//
// FileFormatDecompress::apply_palette_clr (FileFormatDecompress.cpp:1299-1436) walks the index
// plane once per output channel and writes int32 planes.  k_jp2_palette reads each index sample
// once, clamps it to [0, NE - 1] (:1417-1421) and writes every channel mapped from that
// component in the same pass, in the caller's sample type; directly mapped channels (MTYP 0,
// a memcpy at :1400-1404) are copied by the same launch.
//
// Table layout.  One entry holds the NPC columns of one palette index, each column in the
// table's element type (1, 2 or 4 bytes by the widest column precision), padded to a whole
// number of dwords and then to an ODD number of dwords.  ds_read_b32 serves a wave in two
// groups of 32 lanes over 32 four-byte banks, bank = (address / 4) mod 32; with an odd entry
// stride the map index -> bank is a bijection modulo 32, so lanes whose indices differ modulo
// 32 never meet on a bank whatever the column, and equal indices broadcast.  A column-major
// table (one sub-table per column) has the same property but costs one LDS read per channel;
// here a 3 x 8-bit or 2 x 16-bit entry is one dword and a single read yields all channels
// (kernel MODE 0).  Tables of up to GK_PAL_LDS_BYTES are staged in LDS by every
// workgroup; larger ones (NE <= 1024, NPC <= 255: up to 1 MiB) are gathered from global
// memory in the same layout, where they stay L2-resident.
//
// Every thread handles GK_PAL_PIX consecutive samples of a row: one vector load of the
// indices, one vector store per channel when the output rows are aligned for it (the engine's
// own staging always is), scalar stores otherwise; the last, partial vector of a row is done
// sample by sample.  A workgroup covers 256 * GK_PAL_PIX columns of `rows` rows so that the
// table is staged once for many samples.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "gk_common.h"
#include "gk_launch.h"

namespace {
constexpr int PIX = GK_PAL_PIX;

template <typename T, int N> struct Vec { typedef T type __attribute__((ext_vector_type(N))); };

template <typename LT> __device__ __forceinline__ uint32_t entry_col(const uint32_t* e, uint32_t col) {
    const uint32_t byte = col * (uint32_t)sizeof(LT);
    const uint32_t w = e[byte >> 2];
    if (sizeof(LT) == 4) return w;
    return (w >> ((byte & 3) * 8)) & (sizeof(LT) == 1 ? 0xffu : 0xffffu);
}

// MODE 0: table in LDS, one dword per entry; 1: table in LDS; 2: table in global memory
template <typename SRC, typename DST, typename LT, int MODE>
__global__ __launch_bounds__(256) void k_jp2_palette(GkPalArgs a) {
    extern __shared__ uint32_t lds_tab[];
    const uint32_t* tab = a.table;
    if (MODE != 2) {
        const uint32_t nw = a.ne * a.entry_words;
        for (uint32_t i = threadIdx.x; i < nw; i += 256) lds_tab[i] = a.table[i];
        __syncthreads();
        tab = lds_tab;
    }
    typedef typename Vec<SRC, PIX>::type SV;
    typedef typename Vec<DST, PIX>::type DV;
    const uint32_t x = (blockIdx.x * 256 + threadIdx.x) * PIX;
    if (x >= a.w) return;
    const bool whole = x + PIX <= a.w;
    const uint32_t n = whole ? PIX : a.w - x;
    const uint32_t y0 = blockIdx.y * a.rows, y1 = min(a.h, y0 + a.rows);
    const int32_t top = (int32_t)a.ne - 1;
    for (uint32_t y = y0; y < y1; ++y) {
        uint32_t idx[PIX];
        if (a.npal) {
            const SRC* s = (const SRC*)a.idx + (size_t)y * a.idx_stride + x;
            if (whole) {
                const SV v = *(const SV*)s;
#pragma unroll
                for (int p = 0; p < PIX; ++p) idx[p] = (uint32_t)min(max((int32_t)v[p], 0), top);
            } else {
#pragma unroll
                for (int p = 0; p < PIX; ++p) idx[p] = p < (int)n ? (uint32_t)min(max((int32_t)s[p], 0), top) : 0u;
            }
        }
        uint32_t word[PIX];
        if (MODE == 0 && a.npal) {
#pragma unroll
            for (int p = 0; p < PIX; ++p) word[p] = tab[idx[p]];
        }
        for (uint32_t k = 0; k < a.nchan; ++k) {
            const GkPalChan ch = a.chans[k];
            DST out[PIX];
            if (ch.direct) {   // MTYP 0: the component's own samples
                const SRC* s = (const SRC*)ch.src + (size_t)y * ch.src_stride + x;
                if (whole) {
                    const SV v = *(const SV*)s;
#pragma unroll
                    for (int p = 0; p < PIX; ++p) out[p] = (DST)v[p];
                } else {
#pragma unroll
                    for (int p = 0; p < PIX; ++p) out[p] = p < (int)n ? (DST)s[p] : (DST)0;
                }
            } else if (MODE == 0) {
                const uint32_t sh = ch.col * (uint32_t)sizeof(LT) * 8;
#pragma unroll
                for (int p = 0; p < PIX; ++p) out[p] = (DST)((word[p] >> sh) & (sizeof(LT) == 1 ? 0xffu : 0xffffu));
            } else {
#pragma unroll
                for (int p = 0; p < PIX; ++p) out[p] = (DST)entry_col<LT>(tab + (size_t)idx[p] * a.entry_words, ch.col);
            }
            DST* d = (DST*)ch.dst + (size_t)y * ch.dst_stride + x;
            if (whole && a.vec_store) {
                DV v;
#pragma unroll
                for (int p = 0; p < PIX; ++p) v[p] = out[p];
                *(DV*)d = v;
            } else {
#pragma unroll
                for (int p = 0; p < PIX; ++p) if (p < (int)n) d[p] = out[p];
            }
        }
    }
}

template <typename SRC, typename DST, typename LT>
void launch_lt(hipStream_t st, const GkPalArgs& a, int mode, dim3 grid, size_t lds) {
    if (mode == 0) hipLaunchKernelGGL((k_jp2_palette<SRC, DST, LT, 0>), grid, dim3(256), lds, st, a);
    else if (mode == 1) hipLaunchKernelGGL((k_jp2_palette<SRC, DST, LT, 1>), grid, dim3(256), lds, st, a);
    else hipLaunchKernelGGL((k_jp2_palette<SRC, DST, LT, 2>), grid, dim3(256), 0, st, a);
}
template <typename SRC, typename DST>
void launch_sd(hipStream_t st, const GkPalArgs& a, int mode, dim3 grid, size_t lds) {
    if (a.elem_bytes == 1) launch_lt<SRC, DST, uint8_t>(st, a, mode, grid, lds);
    else if (a.elem_bytes == 2) launch_lt<SRC, DST, uint16_t>(st, a, mode, grid, lds);
    else launch_lt<SRC, DST, uint32_t>(st, a, mode == 0 ? 1 : mode, grid, lds);
}
template <typename SRC>
void launch_s(hipStream_t st, int dtype, const GkPalArgs& a, int mode, dim3 grid, size_t lds) {
    if (dtype == GK_U8) launch_sd<SRC, uint8_t>(st, a, mode, grid, lds);
    else if (dtype == GK_U16) launch_sd<SRC, uint16_t>(st, a, mode, grid, lds);
    else launch_sd<SRC, int32_t>(st, a, mode, grid, lds);
}
}  // namespace

uint32_t gk_pal_entry_words(uint32_t npc, uint32_t elem_bytes) {
    return ((npc * elem_bytes + 3) / 4) | 1u;
}

int gk_launch_jp2_palette(hipStream_t st, int stype, int dtype, const GkPalArgs& args) {
    GkPalArgs a = args;
    if (!a.w || !a.h || !a.nchan) return -1;
    const size_t bytes = (size_t)a.ne * a.entry_words * 4;
    const int mode = !a.npal ? 2 : bytes > GK_PAL_LDS_BYTES ? 2 : (a.entry_words == 1 && a.elem_bytes < 4) ? 0 : 1;
    // rows per workgroup: enough samples behind one table staging (a dword per 64 samples at most)
    a.rows = mode == 2 ? 8 : (uint32_t)std::min<size_t>(64, std::max<size_t>(8, bytes / 1024));
    a.rows = std::max(a.rows, (a.h + 65534) / 65535);   // (grid.y limit)
    const dim3 grid((a.w + 256 * PIX - 1) / (256 * PIX), (a.h + a.rows - 1) / a.rows);
    const size_t lds = mode == 2 ? 0 : bytes;
    if (stype == GK_U8) launch_s<uint8_t>(st, dtype, a, mode, grid, lds);
    else if (stype == GK_U16) launch_s<uint16_t>(st, dtype, a, mode, grid, lds);
    else launch_s<int32_t>(st, dtype, a, mode, grid, lds);
    return mode;
}

// ---------------------------------------------------------------------------
// Display stage: what Grok's CLI does to the decoded image (GrkDecompress::postProcess,
// grk_decompress.cpp:1300-1506), on the device.
//
// k_ycc_rgb  color_sycc_to_rgb / color_esycc_to_rgb (bin/common/color.cpp:86-418, 1027-1086)
// k_cmyk_rgb color_cmyk_to_rgb (:970-1024)
// k_upsample upsample_image_components (bin/common/convert.cpp:209-360)
//
// All three are gathers: no LDS, no cross-lane traffic.  As in k_jp2_palette a thread owns
// GK_PAL_PIX consecutive samples of a row (16 bytes per lane of 16-bit samples, 8 of 8-bit, two
// 16-byte accesses of int32), loaded and stored as one vector where the rows are aligned (the
// engine's source planes always are) and sample by sample in the last, partial vector of a row.
// In the subsampled sYCC modes the thread's block is PIX columns of one row (4:2:2) or of a row
// pair (4:2:0): the PIX / 2 (+ 1 with an odd origin) chroma samples under it are loaded once,
// their three integer terms computed once, and used for the 2 or 4 pixels they cover.
//
// Arithmetic.  The reference is host code compiled without contraction: sYCC and e-sYCC in
// double, CMYK in float, each product and sum rounded on its own, the cast truncating.  hipcc
// contracts a * b + c into an FMA in device code by default, so every function below that does
// floating-point arithmetic carries `#pragma clang fp contract(off)` (the pragma rather than
// per-operation intrinsics: HIP's __dmul_rn / __dadd_rn are plain operators to the compiler and
// would be contracted all the same).
//
// Which chroma sample a pixel takes (sycc422_to_rgb :170-254, sycc420_to_rgb :256-377), with
// ofx / ofy the parities of the image origin, rx = x - ofx, ry = y - ofy:
//   4:2:2  x < ofx: Cb = Cr = 0 as passed in (-offset after the subtraction, not neutral),
//          else chroma[y][rx / 2]; an unpaired last column takes the next sample, which is the
//          same expression.
//   4:2:0  y < ofy: the whole row takes 0; else chroma[ry / 2][rx / 2] and 0 for x < ofx, except
//          - ofx = ofy = 1 (:316-320): column 0 takes 0 in the first row of a pair but
//            chroma[ry / 2][0] in the second, and an unpaired last row (:344-357) ignores ofx:
//            chroma[ry / 2][x / 2] from column 0 on;
//          - ofy = 1, ofx = 0: column 0 of the first row of each pair takes 0.
//          (For ofx != ofy the reference's loops leave the planes; DESIGN.md says what is kept.)
namespace {
struct Rgb { int32_t r, g, b; };

// the chroma terms of sycc_to_rgb (:91-107): (int32_t)(1.402 * cr), (int32_t)(0.344 * cb + 0.714 * cr),
// (int32_t)(1.772 * cb) after the offset subtraction
__device__ __forceinline__ Rgb sycc_terms(int32_t cb, int32_t cr, int32_t offset) {
#pragma clang fp contract(off)
    cb -= offset;
    cr -= offset;
    Rgb t;
    t.r = (int32_t)(1.402 * (double)cr);
    const double g0 = 0.344 * (double)cb, g1 = 0.714 * (double)cr;
    t.g = (int32_t)(g0 + g1);
    t.b = (int32_t)(1.772 * (double)cb);
    return t;
}
__device__ __forceinline__ int32_t clamp_upb(int32_t v, int32_t upb) { return v < 0 ? 0 : (v > upb ? upb : v); }
__device__ __forceinline__ Rgb sycc_px(int32_t y, const Rgb& t, int32_t upb) {
    Rgb o;
    o.r = clamp_upb(y + t.r, upb);
    o.g = clamp_upb(y - t.g, upb);
    o.b = clamp_upb(y + t.b, upb);
    return o;
}
// color_esycc_to_rgb (:1047-1078): left to right in double, + 0.5, truncated, clamped
__device__ __forceinline__ Rgb esycc_px(int32_t yi, int32_t cbi, int32_t cri, const GkYccArgs& a) {
#pragma clang fp contract(off)
    if (a.flip_cb) cbi -= a.offset;
    if (a.flip_cr) cri -= a.offset;
    const double y = (double)yi, cb = (double)cbi, cr = (double)cri;
    double t, m;
    Rgb o;
    m = 0.0000368 * cb; t = y - m; m = 1.40199 * cr; t = t + m; t = t + 0.5;
    o.r = clamp_upb((int32_t)t, a.upb);
    t = 1.0003 * y; m = 0.344125 * cb; t = t - m; m = 0.7141128 * cr; t = t - m; t = t + 0.5;
    o.g = clamp_upb((int32_t)t, a.upb);
    t = 0.999823 * y; m = 1.77204 * cb; t = t + m; m = 0.000008 * cr; t = t - m; t = t + 0.5;
    o.b = clamp_upb((int32_t)t, a.upb);
    return o;
}

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
template <typename DST> __device__ __forceinline__ void store_rgb(const GkYccArgs& a, uint32_t y, uint32_t x, bool vec, uint32_t n,
                                                                  const Rgb px[PIX]) {
    int32_t v[PIX];
#pragma unroll
    for (int p = 0; p < PIX; ++p) v[p] = px[p].r;
    store_row<DST>((DST*)a.dst[0] + (size_t)y * a.ds[0] + x, vec, n, v);
#pragma unroll
    for (int p = 0; p < PIX; ++p) v[p] = px[p].g;
    store_row<DST>((DST*)a.dst[1] + (size_t)y * a.ds[1] + x, vec, n, v);
#pragma unroll
    for (int p = 0; p < PIX; ++p) v[p] = px[p].b;
    store_row<DST>((DST*)a.dst[2] + (size_t)y * a.ds[2] + x, vec, n, v);
}

// One row unit per iteration: a row (4:4:4, e-sYCC, 4:2:2) or, in 4:2:0, the rows sharing one
// chroma row: unit u < ofy is row 0 alone, unit u >= ofy rows ofy + 2 (u - ofy) and the next.
template <typename SRC, typename DST, int MODE>
__global__ __launch_bounds__(256) void k_ycc_rgb(GkYccArgs a) {
    const uint32_t x = (blockIdx.x * 256 + threadIdx.x) * PIX;
    if (x >= a.w) return;
    const bool whole = x + PIX <= a.w;
    const uint32_t n = whole ? PIX : a.w - x;
    const bool vst = whole && a.vec_store;
    const uint32_t units = MODE == GK_YCC_420 ? a.ofy + (a.h - a.ofy + 1) / 2 : a.h;
    const uint32_t u0 = blockIdx.y * a.rows, u1 = min(units, u0 + a.rows);
    for (uint32_t u = u0; u < u1; ++u) {
        int32_t ya[PIX];
        Rgb px[PIX];
        if (MODE == GK_YCC_444 || MODE == GK_YCC_ESYCC) {
            int32_t cb[PIX], cr[PIX];
            load_row<SRC>((const SRC*)a.y + (size_t)u * a.ys + x, whole, n, ya);
            load_row<SRC>((const SRC*)a.cb + (size_t)u * a.cs + x, whole, n, cb);
            load_row<SRC>((const SRC*)a.cr + (size_t)u * a.cs + x, whole, n, cr);
#pragma unroll
            for (int p = 0; p < PIX; ++p)
                px[p] = MODE == GK_YCC_444 ? sycc_px(ya[p], sycc_terms(cb[p], cr[p], a.offset), a.upb) : esycc_px(ya[p], cb[p], cr[p], a);
            store_rgb<DST>(a, u, x, vst, n, px);
            continue;
        }
        // subsampled: rows of the unit, its chroma row, and whether the columns pair from ofx
        uint32_t y, crow;
        bool zero_row = false, two = false;
        if (MODE == GK_YCC_422) { y = u; crow = u; }
        else if (u < a.ofy) { y = 0; crow = 0; zero_row = true; }
        else { crow = u - a.ofy; y = a.ofy + 2 * crow; two = y + 1 < a.h; }
        // 4:2:0 with both parities odd: the unpaired last row pairs its columns from 0
        const uint32_t ofx = (MODE == GK_YCC_420 && a.ofx && a.ofy && !two && !zero_row) ? 0u : a.ofx;
        Rgb t[PIX];       // chroma terms per column
        const Rgb tz = sycc_terms(0, 0, a.offset);
        if (zero_row) {
#pragma unroll
            for (int p = 0; p < PIX; ++p) t[p] = tz;
        } else {
            typedef typename Vec<SRC, PIX / 2>::type HV;
            const SRC* pb = (const SRC*)a.cb + (size_t)crow * a.cs;
            const SRC* pr = (const SRC*)a.cr + (size_t)crow * a.cs;
            if (whole && !ofx) {
                const HV vb = *(const HV*)(pb + x / 2), vr = *(const HV*)(pr + x / 2);
#pragma unroll
                for (int q = 0; q < PIX / 2; ++q) t[2 * q] = t[2 * q + 1] = sycc_terms((int32_t)vb[q], (int32_t)vr[q], a.offset);
            } else {
#pragma unroll
                for (int p = 0; p < PIX; ++p) {
                    const uint32_t xp = x + p;
                    if (xp >= a.w) t[p] = tz;
                    else if (xp < ofx) t[p] = tz;
                    else if (p > 0 && x + p - 1 >= ofx && ((xp - ofx) & 1)) t[p] = t[p - 1];
                    else { const uint32_t cc = (xp - ofx) >> 1; t[p] = sycc_terms((int32_t)pb[cc], (int32_t)pr[cc], a.offset); }
                }
            }
        }
        load_row<SRC>((const SRC*)a.y + (size_t)y * a.ys + x, whole, n, ya);
#pragma unroll
        for (int p = 0; p < PIX; ++p) px[p] = sycc_px(ya[p], t[p], a.upb);
        // column 0 of the first row of a pair takes Cb = Cr = 0 when the origin's row is odd (:316-320)
        if (MODE == GK_YCC_420 && x == 0 && two && a.ofy) px[0] = sycc_px(ya[0], tz, a.upb);
        store_rgb<DST>(a, y, x, vst, n, px);
        if (two) {
            load_row<SRC>((const SRC*)a.y + (size_t)(y + 1) * a.ys + x, whole, n, ya);
#pragma unroll
            for (int p = 0; p < PIX; ++p) px[p] = sycc_px(ya[p], t[p], a.upb);
            // ... and its second row the first chroma sample of the row (:319) when both parities are odd
            if (x == 0 && a.ofx && a.ofy) {
                const SRC* pb = (const SRC*)a.cb + (size_t)crow * a.cs;
                const SRC* pr = (const SRC*)a.cr + (size_t)crow * a.cs;
                px[0] = sycc_px(ya[0], sycc_terms((int32_t)pb[0], (int32_t)pr[0], a.offset), a.upb);
            }
            store_rgb<DST>(a, y + 1, x, vst, n, px);
        }
    }
}

template <typename SRC, typename DST>
__global__ __launch_bounds__(256) void k_cmyk_rgb(GkCmykArgs a) {
#pragma clang fp contract(off)
    const uint32_t x = (blockIdx.x * 256 + threadIdx.x) * PIX;
    if (x >= a.w) return;
    const bool whole = x + PIX <= a.w;
    const uint32_t n = whole ? PIX : a.w - x;
    const bool vst = whole && a.vec_store;
    const uint32_t y0 = blockIdx.y * a.rows, y1 = min(a.h, y0 + a.rows);
    for (uint32_t y = y0; y < y1; ++y) {
        int32_t in[4][PIX];
#pragma unroll
        for (int k = 0; k < 4; ++k) load_row<SRC>((const SRC*)a.src[k] + (size_t)y * a.ss + x, whole, n, in[k]);
        float K[PIX];
#pragma unroll
        for (int p = 0; p < PIX; ++p) { const float k = (float)in[3][p] * a.scale[3]; K[p] = 1.0F - k; }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int32_t v[PIX];
#pragma unroll
            for (int p = 0; p < PIX; ++p) {
                float c = (float)in[k][p] * a.scale[k];
                c = 1.0F - c;
                const float m = 255.0F * c;
                v[p] = (int32_t)(m * K[p]);
            }
            store_row<DST>((DST*)a.dst[k] + (size_t)y * a.ds[k] + x, vst, n, v);
        }
    }
}

template <typename SRC, typename DST>
__global__ __launch_bounds__(256) void k_upsample(GkUpArgs a) {
    const uint32_t x = (blockIdx.x * 256 + threadIdx.x) * PIX;
    if (x >= a.w) return;
    const bool whole = x + PIX <= a.w;
    const uint32_t n = whole ? PIX : a.w - x;
    const bool vst = whole && a.vec_store;
    // source column and phase of the thread's first sample at or after xoff
    const uint32_t xs = max(x, a.xoff);
    const uint32_t q0 = (xs - a.xoff) / a.dx, r0 = (xs - a.xoff) % a.dx;
    const uint32_t y0 = blockIdx.y * a.rows, y1 = min(a.h, y0 + a.rows);
    for (uint32_t y = y0; y < y1; ++y) {
        int32_t v[PIX];
        if (y < a.yoff) {
#pragma unroll
            for (int p = 0; p < PIX; ++p) v[p] = 0;
        } else {
            const SRC* s = (const SRC*)a.src + (size_t)((y - a.yoff) / a.dy) * a.ss;
            // whole vectors of the two common grids take one vector load: a copy (dx = 1) and
            // 2:1 from an even origin; every other case gathers sample by sample
            if (whole && a.xoff == 0 && a.dx == 1) {
                load_row<SRC>(s + x, true, n, v);
                store_row<DST>((DST*)a.dst + (size_t)y * a.ds + x, vst, n, v);
                continue;
            }
            if (whole && a.xoff == 0 && a.dx == 2) {
                typedef typename Vec<SRC, PIX / 2>::type HV;
                const HV hv = *(const HV*)(s + x / 2);
#pragma unroll
                for (int p = 0; p < PIX; ++p) v[p] = (int32_t)hv[p >> 1];
                store_row<DST>((DST*)a.dst + (size_t)y * a.ds + x, vst, n, v);
                continue;
            }
            uint32_t q = q0, r = r0;
            int32_t cur = 0;
            bool have = false;
#pragma unroll
            for (int p = 0; p < PIX; ++p) {
                if (x + p < a.xoff || p >= (int)n) { v[p] = 0; continue; }
                if (!have) { cur = (int32_t)s[q]; have = true; }
                v[p] = cur;
                if (++r == a.dx) { r = 0; ++q; have = false; }
            }
        }
        store_row<DST>((DST*)a.dst + (size_t)y * a.ds + x, vst, n, v);
    }
}

inline uint32_t rows_per_group(uint32_t units) { return std::max(4u, (units + 65534) / 65535); }   // (grid.y limit)

template <typename SRC, typename DST>
void launch_ycc(hipStream_t st, const GkYccArgs& a, dim3 grid) {
    switch (a.mode) {
        case GK_YCC_444: hipLaunchKernelGGL((k_ycc_rgb<SRC, DST, GK_YCC_444>), grid, dim3(256), 0, st, a); break;
        case GK_YCC_422: hipLaunchKernelGGL((k_ycc_rgb<SRC, DST, GK_YCC_422>), grid, dim3(256), 0, st, a); break;
        case GK_YCC_420: hipLaunchKernelGGL((k_ycc_rgb<SRC, DST, GK_YCC_420>), grid, dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL((k_ycc_rgb<SRC, DST, GK_YCC_ESYCC>), grid, dim3(256), 0, st, a); break;
    }
}
// T names the destination element type in the body
#define GK_DISPLAY_DST(t, T, ...)                                 \
    if ((t) == GK_U8) { typedef uint8_t T; __VA_ARGS__; }         \
    else if ((t) == GK_U16) { typedef uint16_t T; __VA_ARGS__; }  \
    else { typedef int32_t T; __VA_ARGS__; }
}  // namespace

void gk_launch_ycc_rgb(hipStream_t st, int stype, int dtype, const GkYccArgs& args) {
    GkYccArgs a = args;
    if (!a.w || !a.h) return;
    const uint32_t units = a.mode == GK_YCC_420 ? a.ofy + (a.h - a.ofy + 1) / 2 : a.h;
    a.rows = rows_per_group(units);
    const dim3 grid((a.w + 256 * PIX - 1) / (256 * PIX), (units + a.rows - 1) / a.rows);
    GK_DISPLAY_DST(stype, S, GK_DISPLAY_DST(dtype, D, launch_ycc<S, D>(st, a, grid)))
}

void gk_launch_cmyk_rgb(hipStream_t st, int stype, int dtype, const GkCmykArgs& args) {
    GkCmykArgs a = args;
    if (!a.w || !a.h) return;
    a.rows = rows_per_group(a.h);
    const dim3 grid((a.w + 256 * PIX - 1) / (256 * PIX), (a.h + a.rows - 1) / a.rows);
    GK_DISPLAY_DST(stype, S, GK_DISPLAY_DST(dtype, D, hipLaunchKernelGGL((k_cmyk_rgb<S, D>), grid, dim3(256), 0, st, a)))
}

void gk_launch_upsample(hipStream_t st, int stype, int dtype, const GkUpArgs& args) {
    GkUpArgs a = args;
    if (!a.w || !a.h) return;
    a.rows = rows_per_group(a.h);
    const dim3 grid((a.w + 256 * PIX - 1) / (256 * PIX), (a.h + a.rows - 1) / a.rows);
    GK_DISPLAY_DST(stype, S, GK_DISPLAY_DST(dtype, D, hipLaunchKernelGGL((k_upsample<S, D>), grid, dim3(256), 0, st, a)))
}
