// gk_rgbycc.hip — the input stage of an encode under gk_set_encode_convert: R, G, B (packed
// pixels or three equal planes) to sYCC with the chroma planes on their own grid (4:4:4, 4:2:2,
// 4:2:0), the forward of k_ycc_rgb (gk_colour.hip), in one pass.  Grok has no forward conversion
// (its CLI takes subsampled raw YUV); the arithmetic is the engine's own, in integers:
//   Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
//   Cb = floor((-11059 SR - 21709 SG + 32768 SB + 2^(s-1)) / 2^s) + offset, clamped to [0, upb]
//   Cr = floor(( 32768 SR - 27439 SG -  5329 SB + 2^(s-1)) / 2^s) + offset, clamped to [0, upb]
// SR, SG, SB the sums over the chroma sample's box of n = 1, 2 or 4 pixels, s = 16 + log2(n).
//
// Shape (gk_unpixels.hip's idiom).  A thread owns GK_PAL_PIX (8) consecutive pixels of a row, in
// 4:2:0 of a row pair, aligned to the chroma boxes: column ofx + 8t, row ofy + 2u (ofx / ofy: the
// parity of the image origin on a subsampled axis).  The column and row in front of the first box
// belong to none: lane 0 and the first row of workgroups write their luma.  Packed pixels are
// loaded as k_unpixels loads them (16-, 8- or 4-byte loads by the row's alignment,
// realigned dwords for rows 1..3 bytes off; no byte outside a row's w * 3 * es is read), planes in vector
// loads where their address allows.  Y leaves as one vector store of 8 samples (sample by sample
// when ofx shifts the group off its alignment), Cb / Cr as vector stores of 8 or 4, into planes
// of the same sample type whose bases and row strides are aligned to 32 bytes.  Partial groups at
// the right edge go sample by sample.  No LDS, no cross-lane traffic.
//
// Chroma is summed in int32 up to 13 bits (|numerator| <= 32768 * 4 * 8191 + 2^17 < 2^31), in
// int64 above (2^33 at 16 bits, n = 4); the branch is uniform.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "gk_common.h"
#include "gk_launch.h"

namespace {
constexpr int PIX = GK_PAL_PIX;
typedef uint32_t U4 __attribute__((ext_vector_type(4)));
typedef uint32_t U2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t luma(uint32_t r, uint32_t g, uint32_t b) {
    return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16;
}

// the chroma pair of a box of n pixels whose sums are sr, sg, sb
template <typename ACC>
__device__ __forceinline__ void chroma(uint32_t sr, uint32_t sg, uint32_t sb, uint32_t n, int32_t offset, int32_t upb,
                                       uint32_t& cb, uint32_t& cr) {
    const uint32_t s = 16u + (n >> 1);   // n = 1, 2, 4
    const ACC half = (ACC)1 << (s - 1), r = (ACC)sr, g = (ACC)sg, b = (ACC)sb;
    const ACC vb = ((ACC)-11059 * r - (ACC)21709 * g + (ACC)32768 * b + half) >> s;   // (arithmetic: floor)
    const ACC vr = ((ACC)32768 * r - (ACC)27439 * g - (ACC)5329 * b + half) >> s;
    cb = (uint32_t)min(max((int32_t)vb + offset, 0), upb);
    cr = (uint32_t)min(max((int32_t)vr + offset, 0), upb);
}

// sample i of words holding consecutive samples of T in memory order
template <typename T, int NW> __device__ __forceinline__ uint32_t sample(const uint32_t (&w)[NW], int i) {
    if (sizeof(T) == 4) return w[i];
    if (sizeof(T) == 2) return (w[i / 2] >> (16 * (i & 1))) & 0xffffu;
    return (w[i / 4] >> (8 * (i & 3))) & 0xffu;
}

// N samples (each within T's range) as one vector store at d, aligned to N * sizeof(T) bytes (32: 16)
template <typename T, int N> __device__ __forceinline__ void store_n(T* d, const uint32_t (&v)[N]) {
    constexpr int NO = N * (int)sizeof(T) / 4;
    uint32_t o[NO];
#pragma unroll
    for (int j = 0; j < NO; ++j) {
        if (sizeof(T) == 4) o[j] = v[j];
        else if (sizeof(T) == 2) o[j] = v[2 * j] | v[2 * j + 1] << 16;
        else o[j] = v[4 * j] | v[4 * j + 1] << 8 | v[4 * j + 2] << 16 | v[4 * j + 3] << 24;
    }
    if constexpr (NO == 1) *(uint32_t*)d = o[0];
    else if constexpr (NO == 2) { U2 q = {o[0], o[1]}; *(U2*)d = q; }
    else if constexpr (NO == 4) { U4 q = {o[0], o[1], o[2], o[3]}; *(U4*)d = q; }
    else {
        U4 q0 = {o[0], o[1], o[2], o[3]}, q1 = {o[4], o[5], o[6], o[7]};
        *(U4*)d = q0; *((U4*)d + 1) = q1;
    }
}

// A lane's run of LB contiguous bytes of packed pixels (8 pixels: LB is a multiple of 8) as dwords:
// k_unpixels's loads (gk_unpixels.hip), kept apart from it because sharing them changed that
// kernel's register allocation.  mis: the low four bits of the address of the row's
// first run, so the choice between the paths is uniform (lane i + 1 starts where lane i ends: a
// multiple of 8 bytes keeps alignment to 8, a multiple of 16 to 16).  No byte outside the lane's
// LB bytes is read.
// the run at s starts on a dword (32-bit samples always do): 16-, 8- or 4-byte loads
template <int LB>
__device__ __forceinline__ void load_run(const uint8_t* s, uint32_t mis, uint32_t (&in)[LB / 4]) {
    constexpr int NW = LB / 4;
    if (LB % 16 == 0 && mis == 0) {
#pragma unroll
        for (int j = 0; j + 3 < NW; j += 4) { const U4 q = *(const U4*)(s + 4 * j); in[j] = q.x; in[j + 1] = q.y; in[j + 2] = q.z; in[j + 3] = q.w; }
    } else if ((mis & 7u) == 0) {
#pragma unroll
        for (int j = 0; j < NW; j += 2) { const U2 q = *(const U2*)(s + 4 * j); in[j] = q.x; in[j + 1] = q.y; }
    } else {
#pragma unroll
        for (int j = 0; j < NW; ++j) in[j] = *(const uint32_t*)(s + 4 * j);
    }
}

// the run starts m = mis & 3 = 1..3 bytes past a dword boundary (8 / 16-bit samples): hb = 4 - m
// bytes reach the boundary one by one, then NW - 1 aligned dwords, then the last m bytes, funnelled
// back into the lane's packed words (v_alignbyte_b32)
template <int LB>
__device__ __forceinline__ void load_run_realigned(const uint8_t* s, uint32_t mis, uint32_t (&in)[LB / 4]) {
    constexpr int NW = LB / 4;
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
#pragma unroll
    for (int j = 0; j < NW; ++j) in[j] = __builtin_amdgcn_alignbyte(w[j + 1], w[j], m);
}

// one sample of pixel (x, y), channel k
template <typename T, bool PACKED>
__device__ __forceinline__ uint32_t ld1(const GkRgbYccArgs& a, uint32_t y, uint32_t x, int k) {
    if (PACKED) return ((const T*)((const uint8_t*)a.src[0] + (size_t)y * a.row_bytes))[(size_t)x * 3 + k];
    return ((const T*)a.src[k])[(size_t)y * a.ss[k] + x];
}

// the 8 whole pixels from column x of row y: v[k][p]; x0: the column of the row's first group
template <typename T, bool PACKED>
__device__ __forceinline__ void load8(const GkRgbYccArgs& a, uint32_t y, uint32_t x, uint32_t x0, uint32_t (&v)[3][PIX]) {
    if (PACKED) {
        constexpr int LB = PIX * 3 * (int)sizeof(T), NW = LB / 4;   // the lane's bytes: 24, 48, 96
        const uint8_t* s = (const uint8_t*)a.src[0] + (size_t)y * a.row_bytes + (size_t)x * 3 * sizeof(T);
        // (uniform: the row's first run, at column ofx, and a lane's run is a multiple of 8 bytes)
        const uint32_t mis = (uint32_t)(uintptr_t)((const uint8_t*)a.src[0] + (size_t)y * a.row_bytes + (size_t)x0 * 3 * sizeof(T)) & 15u;
        uint32_t in[NW];
        if (sizeof(T) == 4 || (mis & 3u) == 0) load_run<LB>(s, mis, in);
        else load_run_realigned<LB>(s, mis, in);
#pragma unroll
        for (int p = 0; p < PIX; ++p) {
            v[0][p] = sample<T, NW>(in, 3 * p); v[1][p] = sample<T, NW>(in, 3 * p + 1); v[2][p] = sample<T, NW>(in, 3 * p + 2);
        }
    } else {
        constexpr int NW = PIX * (int)sizeof(T) / 4;   // 2, 4, 8
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const T* s = (const T*)a.src[k] + (size_t)y * a.ss[k] + x;
            if (((uintptr_t)s & (NW == 2 ? 7u : 15u)) == 0) {
                uint32_t in[NW];
                if constexpr (NW == 2) { const U2 q = *(const U2*)s; in[0] = q.x; in[1] = q.y; }
                else {
#pragma unroll
                    for (int j = 0; j < NW; j += 4) { const U4 q = *((const U4*)s + j / 4); in[j] = q.x; in[j + 1] = q.y; in[j + 2] = q.z; in[j + 3] = q.w; }
                }
#pragma unroll
                for (int p = 0; p < PIX; ++p) v[k][p] = sample<T, NW>(in, p);
            } else {
#pragma unroll
                for (int p = 0; p < PIX; ++p) v[k][p] = s[p];
            }
        }
    }
}

template <typename T, bool PACKED>
__device__ __forceinline__ void luma_at(const GkRgbYccArgs& a, uint32_t y, uint32_t x) {
    ((T*)a.y)[(size_t)y * a.ys + x] = (T)luma(ld1<T, PACKED>(a, y, x, 0), ld1<T, PACKED>(a, y, x, 1), ld1<T, PACKED>(a, y, x, 2));
}

template <typename T, int MODE, bool PACKED, typename ACC>
__device__ __forceinline__ void convert(const GkRgbYccArgs& a) {
    constexpr int DX = MODE == GK_YCC_444 ? 1 : 2, DY = MODE == GK_YCC_420 ? 2 : 1;
    constexpr int NC = PIX / DX;   // chroma samples of a whole group
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    const uint32_t ofx = DX == 2 ? a.ofx : 0u, ofy = DY == 2 ? a.ofy : 0u;
    const uint32_t x = ofx + t * PIX;
    const bool lead = ofx && t == 0;   // this lane also writes the luma of column 0, in front of the first box
    if (x >= a.w && !lead) return;
    const uint32_t n = x >= a.w ? 0u : min((uint32_t)PIX, a.w - x);
    const int32_t offset = 1 << (a.prec - 1), upb = (int32_t)((1u << a.prec) - 1u);
    T* const Y = (T*)a.y;
    T* const CB = (T*)a.cb;
    T* const CR = (T*)a.cr;
    if (ofy && blockIdx.y == 0) {   // row 0, above the first box: luma only
        for (uint32_t p = 0; p < n; ++p) luma_at<T, PACKED>(a, 0, x + p);
        if (lead) luma_at<T, PACKED>(a, 0, 0);
    }
    const uint32_t nu = DY == 2 ? a.ch : a.h;   // row units: chroma rows
    const uint32_t u0 = blockIdx.y * a.rows, u1 = min(nu, u0 + a.rows);
    for (uint32_t u = u0; u < u1; ++u) {
        const uint32_t y = ofy + u * DY;
        const uint32_t nr = (DY == 2 && y + 1 < a.h) ? 2u : 1u;   // (the last row may stand alone)
        if (lead)
            for (uint32_t r = 0; r < nr; ++r) luma_at<T, PACKED>(a, y + r, 0);
        const size_t co = (size_t)u * a.cs + (x - ofx) / DX;
        if (n == PIX) {
            uint32_t sr[NC], sg[NC], sb[NC];
#pragma unroll
            for (int j = 0; j < NC; ++j) sr[j] = sg[j] = sb[j] = 0;
#pragma unroll
            for (int r = 0; r < DY; ++r)
                if (r < (int)nr) {
                    uint32_t v[3][PIX], yy[PIX];
                    load8<T, PACKED>(a, y + r, x, ofx, v);
#pragma unroll
                    for (int p = 0; p < PIX; ++p) {
                        yy[p] = luma(v[0][p], v[1][p], v[2][p]);
                        sr[p / DX] += v[0][p]; sg[p / DX] += v[1][p]; sb[p / DX] += v[2][p];
                    }
                    T* d = Y + (size_t)(y + r) * a.ys + x;
                    if (ofx == 0) store_n<T, PIX>(d, yy);
                    else {
#pragma unroll
                        for (int p = 0; p < PIX; ++p) d[p] = (T)yy[p];
                    }
                }
            uint32_t cb[NC], cr[NC];
#pragma unroll
            for (int j = 0; j < NC; ++j) chroma<ACC>(sr[j], sg[j], sb[j], DX * nr, offset, upb, cb[j], cr[j]);
            store_n<T, NC>(CB + co, cb);
            store_n<T, NC>(CR + co, cr);
        } else if (n) {
            for (uint32_t r = 0; r < nr; ++r)
                for (uint32_t p = 0; p < n; ++p) luma_at<T, PACKED>(a, y + r, x + p);
            for (uint32_t j = 0; j * DX < n; ++j) {
                uint32_t sr = 0, sg = 0, sb = 0, cnt = 0, cb, cr;
                for (uint32_t r = 0; r < nr; ++r)
                    for (uint32_t q = 0; q < (uint32_t)DX; ++q) {
                        const uint32_t xx = x + j * DX + q;
                        if (xx >= a.w) continue;
                        sr += ld1<T, PACKED>(a, y + r, xx, 0); sg += ld1<T, PACKED>(a, y + r, xx, 1); sb += ld1<T, PACKED>(a, y + r, xx, 2);
                        ++cnt;
                    }
                chroma<ACC>(sr, sg, sb, cnt, offset, upb, cb, cr);
                CB[co + j] = (T)cb; CR[co + j] = (T)cr;
            }
        }
    }
}

// T: uint8_t / uint16_t / uint32_t (the sample's bits, unsigned); MODE: GK_YCC_444 / 422 / 420;
// PACKED: (H, W, 3) pixels at src[0], else three planes
template <typename T, int MODE, bool PACKED>
__global__ __launch_bounds__(256) void k_rgb_ycc(GkRgbYccArgs a) {
    if (sizeof(T) == 1 || a.prec <= 13) convert<T, MODE, PACKED, int32_t>(a);
    else convert<T, MODE, PACKED, int64_t>(a);
}

template <typename T, int MODE>
void launch_pk(hipStream_t st, const GkRgbYccArgs& a, dim3 grid) {
    if (a.packed) hipLaunchKernelGGL((k_rgb_ycc<T, MODE, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_rgb_ycc<T, MODE, false>), grid, dim3(256), 0, st, a);
}
template <typename T>
void launch_mode(hipStream_t st, const GkRgbYccArgs& a, dim3 grid) {
    if (a.mode == GK_YCC_444) launch_pk<T, GK_YCC_444>(st, a, grid);
    else if (a.mode == GK_YCC_422) launch_pk<T, GK_YCC_422>(st, a, grid);
    else launch_pk<T, GK_YCC_420>(st, a, grid);
}
}  // namespace

void gk_launch_rgb_ycc(hipStream_t st, int es, const GkRgbYccArgs& args) {
    GkRgbYccArgs a = args;
    if (!a.w || !a.h || a.mode > GK_YCC_420 || !a.prec || a.prec > 16) return;
    const uint32_t ofx = a.mode == GK_YCC_444 ? 0u : a.ofx;
    const uint32_t nu = a.mode == GK_YCC_420 ? a.ch : a.h;   // row units (4:2:0: row pairs)
    a.rows = std::max(4u, (nu + 65534) / 65535);   // (grid.y limit)
    const uint32_t groups = std::max(1u, (a.w - std::min(a.w, ofx) + PIX - 1) / PIX);   // (lane 0 is always there: column 0)
    const dim3 grid((groups + 255) / 256, std::max(1u, (nu + a.rows - 1) / a.rows));
    if (es == 1) launch_mode<uint8_t>(st, a, grid);
    else if (es == 2) launch_mode<uint16_t>(st, a, grid);
    else launch_mode<uint32_t>(st, a, grid);
}
