// gk_launch.h — host-side launch wrappers for the kernels in gk_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gk_common.h"

// Dispatch on the caller's sample type (GkSample): T names the element type in the body.
#define GK_SAMPLE_DISPATCH(t, T, ...)                            \
    switch (t) {                                                 \
        case GK_U8: { typedef uint8_t T; __VA_ARGS__; break; }   \
        case GK_S8: { typedef int8_t T; __VA_ARGS__; break; }    \
        case GK_U16: { typedef uint16_t T; __VA_ARGS__; break; } \
        case GK_S16: { typedef int16_t T; __VA_ARGS__; break; }  \
        default: { typedef int32_t T; __VA_ARGS__; break; }      \
    }

// DC shift / MCT between the caller's planes (sample type stype, GkSample) and the int32 work planes
void gk_launch_dc_rct_fwd(hipStream_t st, int stype, const void* r, const void* g, const void* b, uint32_t sin,
                          int32_t* y, int32_t* u, int32_t* v, uint32_t sout, uint32_t w, uint32_t h, int32_t shift);
void gk_launch_dc_fwd(hipStream_t st, int stype, const void* in, uint32_t sin, int32_t* out, uint32_t sout, uint32_t w,
                      uint32_t h, int32_t shift);
void gk_launch_rct_inv_dc(hipStream_t st, const int32_t* y, const int32_t* u, const int32_t* v, uint32_t sin, int stype,
                          void* r, void* g, void* b, uint32_t sout, uint32_t w, uint32_t h, int32_t shift,
                          int32_t mn, int32_t mx);
void gk_launch_dc_inv(hipStream_t st, const int32_t* in, uint32_t sin, int stype, void* out, uint32_t sout, uint32_t w,
                      uint32_t h, int32_t shift, int32_t mn, int32_t mx);
// one DWT level of cs.n components (planes cs.cstride apart), every tile of tb
// components per workgroup of a DWT level launch (gk_kernels.hip)
uint32_t gk_dwt_cpw(uint32_t wgs, uint32_t n, bool multi);
void gk_launch_dwt53_fwd(hipStream_t st, const int32_t* src, uint32_t sstride, int32_t* dst, uint32_t dstride,
                         uint32_t w, uint32_t h, GkTiles tb = GkTiles(), GkComps cs = GkComps());
void gk_launch_dwt53_inv(hipStream_t st, const int32_t* src, uint32_t sstride, int32_t* dst, uint32_t dstride,
                         uint32_t w, uint32_t h, GkTiles tb = GkTiles(), GkComps cs = GkComps());
// level 1 fused with the sample stage: nc = 3 (DC + RCT of three components) or 1 (DC of one)
void gk_launch_dwt53_fwd_l1(hipStream_t st, int stype, int nc, GkPtr3 in, uint32_t sin, int32_t* dst, uint64_t cstride,
                            uint32_t dstride, uint32_t w, uint32_t h, GkTiles tb, int32_t shift);
void gk_launch_dwt53_inv_l1(hipStream_t st, int stype, int nc, const int32_t* src, uint64_t cstride, uint32_t sstride,
                            GkPtr3 out, uint32_t ostride, GkWin win, uint32_t w, uint32_t h, GkTiles tb, int32_t shift,
                            int32_t mn, int32_t mx);
void gk_launch_gather(hipStream_t st, const uint8_t* src, uint8_t* dst, const uint64_t* seg, uint32_t nseg);
// T1 encode of `count` blocks: positions [base, base + count) of `order` (block ids), or blocks
// [base, base + count) without one; count = ~0u: all nblocks
void gk_launch_t1_cm(hipStream_t st, const int32_t* coef, const GkBlock* blocks, const uint64_t* sym_off, uint8_t* sym,
                     uint32_t* pass_end, uint32_t* cm_info, uint32_t nblocks, int* err, const int16_t* nmse_tab,
                     int32_t* pass_nmse, const uint32_t* order = nullptr, uint32_t base = 0, uint32_t count = 0xffffffffu,
                     bool index = false, const uint8_t* roi = nullptr, uint64_t roi_mod = 0);
void gk_launch_t1_mq(hipStream_t st, const uint8_t* sym, const uint64_t* sym_off, const uint32_t* pass_end,
                     const uint32_t* cm_info, const GkBlock* blocks, uint8_t* bytes, GkPass* passes, uint32_t* info,
                     uint32_t nblocks, int* err, const int32_t* pass_nmse, uint32_t* pass_counter,
                     const uint32_t* order = nullptr, uint32_t base = 0, uint32_t count = 0xffffffffu,
                     uint32_t nsolo = 0);   // nsolo: the first positions coded by solo waves, one block each
// roi (the three T1 encode front ends; never with index): the coefficient masks of a shaped region of
// interest (gk_roi.hip), a byte per coefficient in two planes laid out like a component's work
// planes: block B's mask lies at roi + B.band_off % roi_mod (roi_mod: the elements of one
// component's plane pair), row stride B.stride.  Only the marked coefficients of a component
// with an ROI shift are scaled up; without roi every coefficient of such a component is.
// per-block coded bit-plane count (weight of the chunked CM / MQ overlap)
void gk_launch_t1_weight(hipStream_t st, const int32_t* coef, const GkBlock* blocks, uint32_t* weight, uint32_t nblocks,
                         const uint8_t* roi = nullptr, uint64_t roi_mod = 0);
uint32_t gk_t1dec_lanes();
// The Part-1 decoder's per-lane scratch slab in 64-bit words (gk_t1dec.hip indexes it, the engine
// allocates it): the state rows, then one plane of 64 rows per bit-plane of the largest numbps
// (mp) among the blocks of the lane's wave
#define GK_T1DEC_WS_FIXED 272
#define GK_T1DEC_WS_PLANE 64
static inline uint64_t gk_t1dec_lane_words(uint32_t mp) { return GK_T1DEC_WS_FIXED + (uint64_t)mp * GK_T1DEC_WS_PLANE; }
// counters of the last k_t1_dec2 launch made with GK_T1_STATS set: max steps per wave, steps,
// symbols (lane-parallel waves), decisions of the solo waves and of the busiest one
void gk_t1dec_stats(uint64_t out[5]);
// solo waves (gk_t1dec.hip solo_block) for a decode: how many the spare SIMDs hold (a multiple
// of 12), a forced block count (one per wave; -1: the host packs), the host's cost ratio
struct GkSoloPlan { uint32_t waves; int forced; float ratio; };
GkSoloPlan gk_t1dec_solo_plan(uint32_t nblocks, uint32_t lanes);
// the first nsolo waves of `order` are solo waves (a multiple of 12)
void gk_launch_t1_dec(hipStream_t st, const uint8_t* bytes, const GkBlock* blocks, const uint32_t* order,
                      uint64_t* scratch, const uint64_t* wave_off, uint32_t nblocks, uint32_t nsolo);
void gk_launch_t1_recon(hipStream_t st, const GkBlock* blocks, const uint32_t* ids, const uint32_t* pos,
                        const uint64_t* scratch, const uint64_t* wave_off, int32_t* coef, uint32_t nblocks,
                        uint32_t maxnp, bool index = false);   // maxnp: the blocks' largest numbps
// index (transcode; the decoders' and encoders' last argument): the coefficient planes hold signed
// quantisation indices (int32, ROI shift included) instead of dequantised / unquantised samples
// one DWT level of any parity, either filter, one line per thread (gk_dwt_any.hip): forward
// reads the input region of `in` and leaves the Mallat level in `out`, inverse the reverse
void gk_launch_dwt_any(hipStream_t st, bool irrev, bool forward, int32_t* in, int32_t* out, uint32_t stride, uint32_t w,
                       uint32_t h, uint32_t px, uint32_t py, GkTiles tb, GkComps cs, bool partial = false);
// irreversible path (gk_dwt97.hip)
// code-blocks with mode switches (gk_t1ms.hip)
void gk_launch_t1_enc_ms(hipStream_t st, const int32_t* coef, const GkBlock* blocks, uint8_t* bytes, GkPass* passes,
                         uint32_t* info, uint32_t nblocks, int* err, const int16_t* nmse_tab, uint32_t* pass_counter,
                         uint8_t* state, uint32_t sty, bool index = false, const uint8_t* roi = nullptr,
                         uint64_t roi_mod = 0);
void gk_launch_t1_dec_ms(hipStream_t st, const uint8_t* bytes, const GkBlock* blocks, const uint32_t* seglen, int32_t* coef,
                         uint32_t nblocks, uint8_t* state, uint32_t sty, bool index = false);
size_t gk_t1ms_state_bytes(uint32_t nblocks);
void gk_launch_dc_ict_fwd(hipStream_t st, int stype, const void* r, const void* g, const void* b, uint32_t sin, float* y,
                          float* u, float* v, uint32_t sout, uint32_t w, uint32_t h, int32_t shift);
void gk_launch_dc_fwd_f(hipStream_t st, int stype, const void* in, uint32_t sin, float* out, uint32_t sout, uint32_t w,
                        uint32_t h, int32_t shift);
void gk_launch_ict_inv_dc(hipStream_t st, const float* y, const float* u, const float* v, uint32_t sin, int stype, void* r,
                          void* g, void* b, uint32_t sout, uint32_t w, uint32_t h, int32_t shift, int32_t mn,
                          int32_t mx);
void gk_launch_dc_inv_f(hipStream_t st, const float* in, uint32_t sin, int stype, void* out, uint32_t sout, uint32_t w,
                        uint32_t h, int32_t shift, int32_t mn, int32_t mx);
void gk_launch_dwt97_fwd(hipStream_t st, const float* src, uint32_t sstride, float* dst, uint32_t dstride, uint32_t w,
                         uint32_t h, GkTiles tb = GkTiles(), GkComps cs = GkComps());
void gk_launch_dwt97_inv(hipStream_t st, const float* src, uint32_t sstride, float* dst, uint32_t dstride, uint32_t w,
                         uint32_t h, GkTiles tb = GkTiles(), GkComps cs = GkComps());
// level 1 fused with the sample stage: nc = 3 (DC + ICT) or 1 (DC)
void gk_launch_dwt97_fwd_l1(hipStream_t st, int stype, int nc, GkPtr3 in, uint32_t sin, float* dst, uint64_t cstride,
                            uint32_t dstride, uint32_t w, uint32_t h, GkTiles tb, int32_t shift);
void gk_launch_dwt97_inv_l1(hipStream_t st, int stype, int nc, const float* src, uint64_t cstride, uint32_t sstride,
                            GkPtr3 out, uint32_t ostride, GkWin win, uint32_t w, uint32_t h, GkTiles tb, int32_t shift,
                            int32_t mn, int32_t mx);
// HTJ2K cleanup-pass block coder (gk_ht.hip); wide: some block is wider than 64 samples
void gk_launch_ht_enc(hipStream_t st, const int32_t* coef, const GkBlock* blocks, uint8_t* bytes, uint8_t* mel_scratch,
                      uint32_t mel_cap, uint32_t* info, uint32_t nblocks, int* err, bool wide = false, bool index = false,
                      const uint8_t* roi = nullptr, uint64_t roi_mod = 0);
void gk_launch_ht_dec(hipStream_t st, const uint8_t* bytes, const GkBlock* blocks, const uint32_t* ids, int32_t* coef,
                      uint32_t nblocks, int* err, bool wide = false, bool index = false);
// HT 9/7 quantisation control (gk_htq.hip).  k_htq_dist: for every work item (count blocks of one
// band class, order[first ..)) and each of the class's nsteps steps (steps[cls * nsteps + n]) the
// squared quantisation error of its float coefficients, GK_HTQ_RUNGS steps per launch; one float
// partial per item and step, added per class in item order into out[cls * nsteps + n] (double).
// cls_first[cls] .. cls_first[cls + 1]: the class's items.
#define GK_HTQ_RUNGS 32
#define GK_HTQ_ITEM_BLOCKS 8   // blocks per work item at most (the host's split)
struct GkHtqItem { uint32_t first, count, cls, pad; };
void gk_launch_htq_dist(hipStream_t st, const float* coef, const GkBlock* blocks, const uint32_t* order,
                        const GkHtqItem* items, uint32_t nitems, const float* steps, uint32_t nsteps,
                        const uint32_t* cls_first, uint32_t ncls, float* partial, double* out);
// k_htq_len: out[0] = the bytes of the nblocks code-blocks of an HT pass (info[4 i + 2]), out[1] = a
// lower bound of their packet-header bits; partial: 2 * gk_htq_len_partials(nblocks) words
#define GK_HTQ_LEN_PER 4
uint32_t gk_htq_len_partials(uint32_t nblocks);
void gk_launch_htq_len(hipStream_t st, const uint32_t* info, uint32_t nblocks, uint64_t* partial, uint64_t* out);
// JP2 palette expansion (gk_colour.hip).  One output channel: palette column `col` of the launch's
// index plane, or (direct) a copy of the component plane `src`.
struct GkPalChan {
    void* dst;             // output plane (the launch's destination sample type)
    const void* src;       // direct: the component's plane (the launch's source sample type)
    uint32_t dst_stride, src_stride;   // row strides in samples
    uint32_t col, direct;
};
struct GkPalArgs {
    const void* idx;       // index plane, row stride idx_stride samples (unused when npal = 0)
    uint32_t idx_stride;
    uint32_t w, h;
    const GkPalChan* chans;   // device memory: nchan channels, npal of them palette-mapped
    uint32_t nchan, npal;
    const uint32_t* table;    // device memory: ne entries of entry_words dwords (gk_pal_entry_words)
    uint32_t ne, entry_words, elem_bytes;
    uint32_t vec_store;       // every dst and its row stride are aligned to GK_PAL_PIX samples
    uint32_t rows;            // (set by the launcher)
};
#define GK_PAL_PIX 8
#define GK_PAL_LDS_BYTES 65536u   // tables up to this size are staged in LDS
// dwords per table entry: the columns padded to dwords, then to an odd count
uint32_t gk_pal_entry_words(uint32_t npc, uint32_t elem_bytes);
// stype / dtype: GK_U8, GK_U16 or GK_S32 planes in / out; idx, every src and their strides must be
// aligned to GK_PAL_PIX samples.  Returns the table path taken: 0 LDS (one dword per entry),
// 1 LDS, 2 global gather; < 0: nothing to do.
int gk_launch_jp2_palette(hipStream_t st, int stype, int dtype, const GkPalArgs& args);
// Display stage (gk_colour.hip): what Grok's CLI does after the decode (GrkDecompress::postProcess):
// sYCC / e-sYCC / CMYK to RGB and sample replication of subsampled components.  Source planes are
// the engine's own (bases and row strides aligned to GK_PAL_PIX samples); stype / dtype: GK_U8,
// GK_U16 or GK_S32 planes in / out.
enum GkYccMode { GK_YCC_444 = 0, GK_YCC_422 = 1, GK_YCC_420 = 2, GK_YCC_ESYCC = 3 };
struct GkYccArgs {
    const void* y; const void* cb; const void* cr;   // luma w x h; chroma on its own grid (mode)
    uint32_t ys, cs;           // row strides of luma / chroma in samples
    void* dst[3];              // R, G, B: w x h each
    uint32_t ds[3];            // their row strides in samples
    uint32_t w, h;
    uint32_t mode;             // GkYccMode
    uint32_t ofx, ofy;         // 4:2:2 / 4:2:0: the first column / row stands alone (odd image origin)
    int32_t offset, upb;       // 1 << (prec - 1), (1 << prec) - 1
    uint32_t flip_cb, flip_cr; // e-sYCC: the component is unsigned (loses `offset`)
    uint32_t vec_store;        // every dst and its row stride are aligned to GK_PAL_PIX samples
    uint32_t rows;             // (set by the launcher)
};
void gk_launch_ycc_rgb(hipStream_t st, int stype, int dtype, const GkYccArgs& args);
struct GkCmykArgs {
    const void* src[4];        // C, M, Y, K: w x h, row stride ss samples
    uint32_t ss;
    void* dst[3];
    uint32_t ds[3];
    uint32_t w, h;
    float scale[4];            // 1.0F / (float)((1 << prec) - 1) per source channel
    uint32_t vec_store;
    uint32_t rows;
};
void gk_launch_cmyk_rgb(hipStream_t st, int stype, int dtype, const GkCmykArgs& args);
// dst[y][x] = 0 when x < xoff or y < yoff, else src[(y - yoff) / dy][(x - xoff) / dx]
struct GkUpArgs {
    const void* src; uint32_t ss;
    void* dst; uint32_t ds;
    uint32_t w, h;             // of dst
    uint32_t dx, dy, xoff, yoff;
    uint32_t vec_store;
    uint32_t rows;
};
void gk_launch_upsample(hipStream_t st, int stype, int dtype, const GkUpArgs& args);
// Output stage (gk_pixels.hip): forced precision, grey to RGB and packed pixels in one pass.
// Sample k of pixel (x, y) is written at dst + y * row_bytes + (x * nch + k) * es; a planar
// plane is the nch = 1 case.  Source planes are the engine's own (bases and row strides aligned
// to GK_PAL_PIX samples); dst needs its element's alignment only.
enum GkPixOp { GK_PIX_NONE = 0, GK_PIX_CLAMP = 1, GK_PIX_SCALE = 2, GK_PIX_SHIFT = 3 };
#define GK_PIX_MAX_CH 16
struct GkPixChan {
    const void* src;           // the channel's plane, row stride ss samples
    uint32_t ss;
    uint32_t op;               // GkPixOp
    int32_t lo, hi;            // CLAMP
    float scale;               // SCALE: rint((float)v * scale), one float32 product
    uint32_t shift;            // SHIFT: v / 2^shift, truncating toward zero
    uint32_t same_prev;        // src is the plane of the channel before this one: loaded once
    uint32_t pad_;
};
struct GkPixArgs {
    GkPixChan ch[GK_PIX_MAX_CH];
    void* dst;
    uint64_t row_bytes;
    uint32_t w, h, nch;
    uint32_t rows;             // (set by the launcher)
};
// stype / dtype: GK_U8, GK_U16 or GK_S32 planes in / pixels out
void gk_launch_pixels(hipStream_t st, int stype, int dtype, const GkPixArgs& args);
// Last stage of a view (gk_view.hip): src holds rw x rh packed int32 pixels of nch channels, rows
// rw * nch samples apart (the engine's own buffer); they are area-averaged to ow x oh pixels
// (ow <= rw, oh <= rh), mirrored left-right, rotated clockwise by rot quarter turns and written as
// dtype samples: sample k of pixel (x, y) of the written image at dst + y * row_bytes +
// (x * nch + k) * es.  Returns 0, or -1 without a launch when the arguments break these rules.
#define GK_VIEW_MAX_TILES 0xffffffull   /* 16 x 16 output tiles on one grid axis: below 2^32 threads a launch */
struct GkViewArgs {
    const void* src;
    void* dst;
    uint64_t row_bytes;
    uint32_t rw, rh, ow, oh, nch;
    uint32_t mirror, rot;
    uint32_t swap, pix_w, pix_h, tiles_x;   // (set by the launcher)
};
// dtype: GK_U8, GK_U16 or GK_S32 pixels out
int gk_launch_view(hipStream_t st, int dtype, const GkViewArgs& args);
// The view's last stage under gk_set_decode_render (gk_render.hip, k_render): the geometry and the
// area average of k_view, then per channel the window (lo < hi; inv: the caller gave hi < lo)
//     t = floor((2 * 255 * (clamp(v, lo, hi) - lo) + (hi - lo)) / (2 (hi - lo))),  inv: 255 - t,
// the optional curve, and the mode: GK_RENDER_WINDOW writes nch bytes a pixel, GK_RENDER_MAP
// (nch == 1) the three bytes map[3 t + c], GK_RENDER_BLEND min(255, (2 sum_k t_k tint_k,c + 255) /
// 510).  tables: 1024 device bytes, 4-byte aligned: the curve (256), then the map (768); read only
// when has_curve / mode MAP say so.  The written image has out_ch (nch or 3) bytes a pixel.
#define GK_RENDER_TABLE_BYTES 1024u
enum GkRenderMode { GK_RMODE_WINDOW = 1, GK_RMODE_MAP = 2, GK_RMODE_BLEND = 3 };   // gk_render::mode (grok_amd.h)
struct GkRenderChan {
    int32_t lo, hi;            // lo < hi
    uint8_t tint[3];
    uint8_t inv;
};
struct GkRenderArgs {
    GkViewArgs v;              // (dst: uint8 pixels of out_ch channels; row_bytes in bytes)
    GkRenderChan ch[GK_PIX_MAX_CH];
    const uint8_t* tables;
    uint32_t mode, has_curve;
    uint32_t out_ch;           // (set by the launcher)
};
int gk_launch_render(hipStream_t st, const GkRenderArgs& args);
// Statistics of the pixels a view returns as int32 (gk_render.hip, k_levels): per channel k
// stats[k] = {min, max, sum} and, when bins > 0, hist[k * bins + clamp((v - origin_k) >> shift_k,
// 0, bins - 1)] += 1.  stats must hold {INT32_MAX, INT32_MIN, 0} per channel and hist zeros before
// the launch; both are only ever added to.  bins <= GK_LEVELS_BINS_MAX, shift <= 31.
#define GK_LEVELS_BINS_MAX 4096u
struct GkLevelsStat {
    int32_t min, max;
    unsigned long long sum;    // the int64 sum's bits (two's complement)
};
struct GkLevelsArgs {
    GkViewArgs v;              // (dst, row_bytes, mirror, rot unused)
    int32_t origin[GK_PIX_MAX_CH];
    uint32_t shift[GK_PIX_MAX_CH];
    GkLevelsStat* stats;
    unsigned long long* hist;
    uint32_t bins;
};
int gk_launch_levels(hipStream_t st, const GkLevelsArgs& args);
// The view's last stage as a float tensor (gk_tensor.hip, k_tensor): the geometry and the area
// average of k_view, then per channel k the int32 v the view would return becomes
//     z = (float)v * scale[k] + bias[k]     two float32 roundings to nearest even, never one fused
// and is written as float32, float16 or bfloat16 (z rounded to nearest even) at element
// k * stride_c + y * stride_y + x * stride_x of v.dst, (x, y) a pixel of the written image.  The
// strides are in elements and the caller's to vouch for: the launcher checks the geometry only.
enum GkTensorType { GK_TT_F32 = 1, GK_TT_F16 = 2, GK_TT_BF16 = 3 };   // gk_tensor::dtype (grok_amd.h)
struct GkTensorArgs {
    GkViewArgs v;              // (row_bytes unused)
    int64_t stride_c, stride_y, stride_x;
    float scale[GK_PIX_MAX_CH], bias[GK_PIX_MAX_CH];
};
int gk_launch_tensor(hipStream_t st, uint32_t dtype, const GkTensorArgs& args);
// Input stage of an encode from packed pixels (gk_unpixels.hip): sample k of pixel (x, y) is read
// at src + y * row_bytes + (x * nch + k) * es and written to plane k, dst + k * plane samples on,
// row stride ds samples, in the same sample type.  The planes are the engine's own: dst, ds and
// plane aligned to 32 bytes; src needs its element's alignment only, and no byte outside the w *
// nch * es bytes of a row is read.
#define GK_UNPIX_ALIGN 32u
struct GkUnpixArgs {
    const void* src;
    uint64_t row_bytes;
    void* dst;
    uint64_t plane;            // samples between the planes of consecutive channels
    uint32_t ds;
    uint32_t w, h, nch;
    uint32_t rows;             // (set by the launcher)
};
// es: bytes per sample (1, 2 or 4)
void gk_launch_unpixels(hipStream_t st, int es, const GkUnpixArgs& args);
// Input stage of an encode under gk_set_encode_convert (gk_rgbycc.hip): R, G, B to Y, Cb, Cr with
// the chroma planes on the grid of `mode` (GK_YCC_444 / 422 / 420), in the same sample type.
// packed: sample k of pixel (x, y) is read at src[0] + y * row_bytes + (x * 3 + k) * es, and no
// byte outside the w * 3 * es bytes of a row; otherwise plane k is src[k], row stride ss[k]
// samples, any alignment of its element.  y, cb, cr are the engine's own planes: bases and the
// row strides ys / cs aligned to 32 bytes; luma w x h, chroma cw x ch = ceil((w - ofx) / 2) [x
// ceil((h - ofy) / 2)] on a subsampled axis (ofx / ofy: the image origin's parity there).
struct GkRgbYccArgs {
    const void* src[3];
    uint64_t row_bytes;        // packed
    uint32_t ss[3];            // planar
    uint32_t packed;
    void* y; void* cb; void* cr;
    uint32_t ys, cs;
    uint32_t w, h, cw, ch;
    uint32_t mode;             // GkYccMode below GK_YCC_ESYCC
    uint32_t ofx, ofy;
    uint32_t prec;             // 1..16, unsigned
    uint32_t rows;             // (set by the launcher)
};
// es: bytes per sample (1, 2 or 4)
void gk_launch_rgb_ycc(hipStream_t st, int es, const GkRgbYccArgs& args);
// Colour management of the display stage (gk_icc.hip): a JP2 file's ICC profile (colr METH 2,
// matrix / tone-curve classes; gk_icc.h reads it) and the CIELab enumerated space (EnumCS 14)
// to sRGB, as color_apply_icc_profile / color_cielab_to_rgb (bin/common/color.cpp:423-964) on
// v / (2^prec - 1).  Source planes are the engine's own (aligned to GK_PAL_PIX samples).
enum GkIccKind { GK_ICC_IDENTITY = 0, GK_ICC_PARA = 1, GK_ICC_TABLE = 2, GK_ICC_LUT = 3 };
struct GkIccChan {
    uint32_t kind;             // GkIccKind
    uint32_t off, n;           // TABLE (n >= 2 16-bit entries over [0, 1], interpolated) / LUT (the value of sample v at v):
                               // n elements of the launch's table from element off on
    uint32_t pad_;
    double g, a, b, c, d, e, f;   // PARA: x >= d ? pow(a * x + b, g) + e : c * x + f
};
struct GkIccArgs {
    const void* src[3];        // R, G, B (nch = 3) or the grey channel (nch = 1): w x h
    uint32_t ss[3];
    void* dst[3];
    uint32_t ds[3];
    uint32_t w, h, nch, prec;
    GkIccChan ch[3];
    double m[3][3];            // curve output -> linear sRGB (unused when nch = 1)
    const void* table;         // device memory: table_elems floats (prec <= GK_ICC_FLOAT_PREC) or doubles
    uint32_t table_elems;
    uint32_t vec_store;
    uint32_t rows;             // (set by the launcher)
};
#define GK_ICC_FLOAT_PREC 12u      // samples of up to this many bits are evaluated in float32, wider ones in double
#define GK_ICC_LDS_BYTES 32768u    // curve tables up to this size are staged in LDS, larger ones read from global memory
// Returns 1 when the table was staged in LDS, 0 when it is read from global memory (or there is none).
int gk_launch_icc_rgb(hipStream_t st, int stype, int dtype, const GkIccArgs& args);
struct GkLabArgs {
    const void* src[3];        // L*, a*, b*: w x h, row stride ss samples
    uint32_t ss[3];
    void* dst[3];              // R, G, B at 16 bits
    uint32_t ds[3];
    uint32_t w, h;
    double lo[3], range[3];    // value = lo + v * range / vmax
    double vmax;               // 2^prec - 1
    double m[3][3];            // XYZ -> linear sRGB: the inverse of the sRGB colorants (gk_icc.h)
    uint32_t vec_store;
    uint32_t rows;
};
void gk_launch_lab_rgb(hipStream_t st, int stype, int dtype, const GkLabArgs& args);
// Coefficient masks of a shaped region of interest (gk_roi.hip).  Masks are bytes (0 / 1) in two
// planes of the work planes' geometry (row stride `stride`, a multiple of 64).
// level-0 mask of the w x h image: the union of nrects rectangles (device memory: x0, y0, x1, y1
// each, half-open, image samples) and the non-zero bytes of mask (device memory or NULL, row
// stride mask_stride)
void gk_launch_roi_fill(hipStream_t st, uint8_t* dst, uint32_t stride, uint32_t w, uint32_t h, const uint32_t* rects,
                        uint32_t nrects, const uint8_t* mask, uint32_t mask_stride);
// one decomposition level of every tile of tb: the w x h sample mask at each tile's corner of src
// (origin parities px, py) becomes the four band masks in Mallat placement at the same corner of dst
// *flag |= 1 when any of the n bytes at m is non-zero (flag cleared by the caller)
void gk_launch_roi_any(hipStream_t st, const uint8_t* m, size_t n, uint32_t* flag);
void gk_launch_roi_level(hipStream_t st, bool reversible, const uint8_t* src, uint8_t* dst, uint32_t stride, uint32_t w,
                         uint32_t h, uint32_t px, uint32_t py, GkTiles tb);
