// gk_colour.hip — JP2 palette expansion on decode (pclr + cmap boxes).
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
