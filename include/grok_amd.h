/*
 * grok_amd.h — C ABI of the MI355X JPEG 2000 tile-pipeline engine.
 *
 * Drop-in boundary for Grok 9.2.0's hot path.  Plain C types,
 * plain pointers and sizes; no torch/HIP types in any signature.  Every entry
 * point cites the reference interface it replaces (paths relative to
 * /root/reference/src/lib/jp2/).  INTEGRATION.md shows the reference-side
 * binding (ctypes / C call sites) a maintainer would add.
 *
 * Conventions mirror grok.h: functions return 0 / non-NULL on success and a
 * negative code on failure (grok.h returns bool false); messages are
 * retrievable with gk_last_error() (grok.h routes them to grk_set_error_handler
 * callbacks, grok.cpp:116-134).  Calls on one context are synchronous and
 * single-threaded, like calls on one grk_codec (grok.cpp:71-86).
 */
#ifndef GROK_AMD_H
#define GROK_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GK_MAXRLVLS 33
#define GK_MAX_LAYERS 100
#define GK_NUM_COMMENTS 256   /* GRK_NUM_COMMENTS_SUPPORTED */

/* One progression order change (grk_progression's resS, compS, layE, resE, compE, progression;
 * POC marker A.6.6): layers [0, layE), resolutions [resS, resE), components [compS, compE). */
typedef struct gk_poc {
    uint32_t resS, compS, layE, resE, compE;
    int32_t prog;                        /* GRK_PROG_ORDER */
} gk_poc;

/* Coding parameters: the subset of grk_cparameters (grok.h:466-590) the hot
 * path consumes, with the same field names and meaning. */
typedef struct gk_cparameters {
    uint16_t numlayers;                  /* grk_cparameters::numlayers */
    double layer_rate[GK_MAX_LAYERS];    /* grk_cparameters::layer_rate (compression ratio, 0 = lossless) */
    uint8_t numresolution;               /* grk_cparameters::numresolution (default 6) */
    uint32_t cblockw_init, cblockh_init; /* grk_cparameters::cblockw_init / cblockh_init (default 64) */
    uint8_t cblk_sty;                    /* grk_cparameters::cblk_sty: Part-1 mode switches (LAZY 1, RESET 2, TERMALL 4,
                                            VSC 8, PTERM 0x10, SEGSYM 0x20) or 0x40 alone (HTJ2K, GRK_CBLKSTY_HT) */
    uint8_t irreversible;                /* grk_cparameters::irreversible */
    uint8_t mct;                         /* grk_cparameters::mct (RCT/ICT for >= 3 components) */
    uint8_t numgbits;                    /* grk_cparameters::numgbits (default 2) */
    uint8_t csty;                        /* grk_cparameters::csty: bit0 user precincts, 2 SOP before every packet
                                            (grk_compress -S), 4 EPH after every packet header (-E) */
    uint32_t res_spec;                   /* grk_cparameters::res_spec */
    uint32_t prcw_init[GK_MAXRLVLS];     /* grk_cparameters::prcw_init */
    uint32_t prch_init[GK_MAXRLVLS];     /* grk_cparameters::prch_init */
    uint8_t write_comment;               /* write Grok's default COM marker (CodeStreamCompress.cpp:334) */
    uint8_t tile_size_on;                /* grk_cparameters::tile_size_on */
    uint32_t t_width, t_height;          /* grk_cparameters::t_width / t_height (tile origins on the 2^levels grid) */
    uint8_t writeTLM;                    /* grk_cparameters::writeTLM (grk_compress -X) */
    uint8_t writePLT;                    /* grk_cparameters::writePLT (grk_compress -L) */
    int32_t cod_format;                  /* grk_cparameters::cod_format: GRK_CODEC_J2K (0, raw codestream) or
                                            GRK_CODEC_JP2 (2, JP2 file boxes around it; FileFormatCompress.cpp) */
    int32_t prog_order;                  /* grk_cparameters::prog_order: GRK_LRCP 0, RLCP 1, RPCL 2, PCRL 3, CPRL 4 */
    uint8_t enableTilePartGeneration;    /* grk_cparameters::enableTilePartGeneration (grk_compress -u) */
    char newTilePartProgressionDivider;  /* grk_cparameters::newTilePartProgressionDivider: 'L', 'R' or 'C' */
    int32_t roi_compno;                  /* grk_cparameters::roi_compno (-1: none) */
    uint32_t roi_shift;                  /* grk_cparameters::roi_shift: RGN maxshift of that component (Part-1) */
    uint32_t numpocs;                    /* progression order changes, written as a POC marker in each tile's
                                            first tile-part header (CodeStreamCompress::writePoc) */
    gk_poc pocs[32];
    uint8_t allocationByQuality;         /* grk_cparameters::allocationByQuality (grk_compress -q): layers by PSNR */
    double layer_distortion[GK_MAX_LAYERS]; /* grk_cparameters::layer_distortion: PSNR per layer (0 = the rest) */
    uint32_t tx0, ty0;                   /* grk_cparameters::tx0 / ty0 (grk_compress -T): tile grid origin on the
                                            canvas, at or above-left of the image origin (B.3) */
    /* grk_cparameters::comment / comment_len / is_binary_comment / num_comments (grk_compress -C):
       COM markers written instead of Grok's default one (CodeStreamCompress.cpp:303-330 keeps the
       non-empty ones, write_com :1114-1145 writes Rcom 1 (text) or 0 (binary) and the bytes) */
    uint32_t num_comments;
    const char* comment[GK_NUM_COMMENTS];
    uint16_t comment_len[GK_NUM_COMMENTS];
    uint8_t is_binary_comment[GK_NUM_COMMENTS];
} gk_cparameters;

/* Image description: grk_image / grk_image_comp (grok.h:895-959) reduced to
 * what the tile pipeline reads.  Component planes are int32 (grk_image_comp::data),
 * row stride in samples (grk_image_comp::stride). */
typedef struct gk_image_info {
    uint32_t w, h;          /* grk_image::x1 - x0, y1 - y0: the image area (tiles per gk_cparameters) */
    uint32_t numcomps;      /* grk_image::numcomps */
    uint32_t prec;          /* grk_image_comp::prec (same for every component) */
    uint32_t sgnd;          /* grk_image_comp::sgnd */
    uint32_t sample_bytes;  /* the caller's planes: 0 or 4 = int32 (grk_image_comp::data); 1 / 2 = planar
                               8 / 16-bit samples, signed iff sgnd, as grk_compress_tile's buffer
                               (TileProcessor::ingestUncompressedData, TileProcessor.cpp:779-835);
                               must be 4 or (prec + 7) / 8.  Decode writes the same type. */
    uint32_t x0, y0;        /* grk_image::x0 / y0 (grk_compress -d): the image area's canvas origin (SIZ
                               XOsiz / YOsiz); planes hold the area only, windows are relative to it */
} gk_image_info;

/* Per-stage device times of the last call (HIP events on the engine stream). */
typedef struct gk_timings {
    float mct_ms, dwt_ms, t1_ms, t2_ms, assemble_ms, total_ms;
    float t1_cm_ms;         /* encode: context-modelling kernel (k_t1_cm) part of t1_ms */
    float t1_coder_ms;      /* the arithmetic-coder kernel alone: k_t1_mq (encode) / k_t1_dec (decode) */
    uint32_t dwt_launches, t1_blocks;
    uint64_t dwt_bytes;     /* algorithmic bytes moved by the DWT launches */
    uint64_t cs_bytes;      /* codestream bytes produced (encode) / consumed (decode) */
    uint64_t t1_bytes;      /* compressed code-block bytes coded by T1 */
    /* Part-1 decode with GK_T1_STATS set in the environment (0 otherwise): decision steps of
       the longest-running wave, all steps issued, symbols decoded (the T1 chain's work) */
    uint64_t t1_steps_max, t1_steps_total, t1_symbols;
    /* Part-1 decode: code-blocks given to solo waves (one wave per block on the SIMDs the
       lane-parallel waves leave); with GK_T1_STATS, their decisions and the largest per wave */
    uint64_t t1_solo_blocks, t1_solo_decisions, t1_solo_decisions_max;
    /* Part-1 decode: decoder classes of the last call whose solo / lane-parallel split was chosen
       by the rule for a device shared with another engine's call in progress (0 on encode) */
    uint64_t t1_shared;
    /* encode under gk_set_encode_roi: the region's mask kernels (k_roi_fill, k_roi_level), part of
       t1_ms (0 without a region and on decode) */
    float roi_ms;
} gk_timings;

typedef struct gk_ctx gk_ctx;

/* grk_initialize (grok.cpp:75-86): create an engine bound to one MI355X. */
gk_ctx* gk_create(int device_id);
/* grk_deinitialize / grk_object_unref(codec) */
void gk_destroy(gk_ctx* ctx);
/* grk_compress_set_default_params (grok.cpp:405-435) */
void gk_set_default_params(gk_cparameters* p);

/* grk_compress_init + grk_compress_start + grk_compress + grk_compress_end
 * (grok.cpp:382-469; TileProcessor::doCompress TileProcessor.cpp:202-260) for a
 * single- or multi-tile image (all tiles in one pass; one tile part per tile).  comps[c] points at component c's plane (device
 * memory if comps_on_device, host otherwise).  The codestream is written to
 * out (device memory if out_on_device); *out_len receives its size.
 * Returns 0, or < 0 on error (-2: capacity too small, *out_len = needed). */
int gk_encode(gk_ctx* ctx, const gk_image_info* info, const void* const* comps, const uint32_t* strides,
              int comps_on_device, const gk_cparameters* p, uint8_t* out, size_t cap, size_t* out_len,
              int out_on_device);

/* gk_encode from packed pixels, the mirror of gk_decode_pixels: what Grok's image readers hold
 * before they split it into planes (bin/image_format, e.g. PNGFormat / TIFFFormat's
 * interleaved-to-planar pass), read by the device.  Sample k of pixel (x, y) lies at
 * pixels + y * row_bytes + (x * C + k) * es; C = info->numcomps, es follows info->sample_bytes
 * (0 or 4: int32; 1 / 2: (prec + 7) / 8; signed samples are the same bits).  No byte outside the
 * w * C * es bytes of a row is read.  info->x0 / y0 and every coding parameter are honoured and the
 * codestream is the one gk_encode writes for the same samples in planes.  Refused, each by name,
 * before anything is allocated: an active gk_set_subsampling (packed pixels have one grid); a
 * sample_bytes that breaks the rule; row_bytes below w * C * es, or row_bytes / pixels no multiple
 * of es; more than 16 channels (use the planar call); whatever gk_encode refuses.  Returns as
 * gk_encode (-2: capacity too small, *out_len = needed). */
int gk_encode_pixels(gk_ctx* ctx, const gk_image_info* info, const void* pixels, size_t row_bytes,
                     int pixels_on_device, const gk_cparameters* p, uint8_t* out, size_t cap, size_t* out_len,
                     int out_on_device);

/* Tile sharding: encode only tiles [tile_begin, tile_end) of the
 * image described by info / p — grk_compress_tile (grok.h:1082-1657) per tile, without
 * the main header.  comps[c] addresses the image origin; only the sample rows of the
 * selected tiles are read.  out receives their tile parts (SOT [PLT] SOD packets,
 * CodeStreamCompress::writeTilePart :862-900) back to back; part_lens[i] = length
 * of tile tile_begin + i (the TLM Ptlm value).  Returns 0 / < 0 like gk_encode. */
int gk_encode_tiles(gk_ctx* ctx, const gk_image_info* info, const void* const* comps, const uint32_t* strides,
                    int comps_on_device, const gk_cparameters* p, uint32_t tile_begin, uint32_t tile_end,
                    uint8_t* out, size_t cap, size_t* out_len, uint32_t* part_lens, int out_on_device);

/* Main header alone (SOC SIZ [CAP] COD QCD [TLM] [COM]; CodeStreamCompress::
 * init_header_writing :822-860) for assembling sharded tile parts: codestream =
 * header + tile parts in tile order + EOC (0xFFD9).  With TLM, *tlm_offset is the
 * offset of the first 6-byte entry (Ttlm u16 = tile index, Ptlm u32 = tile-part
 * length, big-endian) for the caller to fill; *num_tiles = tiles in the grid. */
int gk_main_header(gk_ctx* ctx, const gk_image_info* info, const gk_cparameters* p, uint8_t* out, size_t cap,
                   size_t* out_len, size_t* tlm_offset, uint32_t* num_tiles);

/* JP2 boxes for a file wrapping a codestream of cs_len bytes (signature, ftyp, jp2h with
 * ihdr + colr, jp2c box header; FileFormatCompress::startCompress / write_jp2c,
 * FileFormatCompress.cpp:666-693, 59-102): JP2 file = these bytes + the codestream.  Used to
 * assemble sharded tile parts into a .jp2.  Returns 0, -2 if cap is too small (*out_len = needed). */
int gk_jp2_header(gk_ctx* ctx, const gk_image_info* info, uint64_t cs_len, uint8_t* out, size_t cap, size_t* out_len);

/* Colour description of later encodes: what FileFormatCompress::initCompress (FileFormatCompress.cpp
 * :694-909) reads from the grk_image, written into the jp2h box as write_jp2h does (:176-264), in
 * its order: ihdr, colr, cdef, pclr, cmap.
 * colr: METH 1 with EnumCS 16 (GRK_CLRSPC_SRGB), 17 (GRAY), 18 (SYCC), 24 (EYCC) or 12 (CMYK), or
 * METH 2 carrying the profile for GRK_CLRSPC_ICC (EnumCS 0); PREC = APPROX = 0.
 * cdef: written when any typ[] is not colour (0); numcomps entries, the first color_channels of
 * them forced to (i, 0, i + 1) (4 for CMYK, 3 for sRGB / sYCC / e-sYCC, 1 for grey, 0 for ICC), the
 * rest (i, typ[i], asoc[i]) (:811-865).
 * pclr + cmap: written when a palette is given; Bi = channel_prec - 1, every LUT value big-endian in
 * (prec + 7) / 8 bytes, one cmap entry per palette column.
 * One effect reaches the codestream, raw or wrapped: sYCC and e-sYCC clear the MCT
 * (CodeStreamCompress.cpp:494-500).
 * Refused, each by name: GRK_CLRSPC_UNKNOWN and values Grok errors on; GRK_CLRSPC_DEFAULT_CIE (EnumCS
 * 14: CIELab is read, not written); GRK_CLRSPC_ICC without a profile; a profile with another colour
 * space (Grok drops it silently); typ / asoc for another component count; a cdef whose
 * color_channels exceed the component count; and every box the engine's own reader refuses
 * (gk_probe_colour's messages: NE outside 1..1024, NPC 0, a column above 16 bits, a LUT value
 * outside its column, MTYP above 1, a column mapped twice or out of range, a direct mapping with a
 * column, a component index out of range, a signed mapped component, a mapped component of more bits
 * than the palette has entries, an incomplete or contradictory cdef). */
typedef struct gk_cmap_entry {
    uint16_t component;        /* grk_component_mapping_comp::component_index (CMP) */
    uint8_t mapping_type;      /* MTYP: 0 direct, 1 palette */
    uint8_t palette_column;    /* PCOL */
} gk_cmap_entry;
typedef struct gk_encode_colour {
    uint32_t colour_space;     /* GRK_COLOR_SPACE, as gk_colour_info::colour_space */
    const uint8_t* icc;        /* grk_color::icc_profile_buf / icc_profile_len */
    uint32_t icc_len;
    uint32_t num_channels;     /* entries of typ / asoc: 0 (every component is colour) or the component count */
    const uint16_t* typ;       /* grk_image_comp::type */
    const uint16_t* asoc;      /* grk_image_comp::association */
    uint32_t palette_entries;  /* grk_palette_data::num_entries (NE); 0 with palette_columns 0: no palette */
    uint32_t palette_columns;  /* num_channels (NPC) */
    const uint8_t* channel_prec;   /* NPC column precisions */
    const int32_t* lut;        /* NE rows of NPC values */
    const gk_cmap_entry* cmap; /* NPC entries */
} gk_encode_colour;
/* Sticky: later gk_encode / gk_encode_pixels calls with cod_format 2, and gk_jp2_header, write the
 * boxes above instead of ihdr + a default colr; everything is copied.  spec = NULL clears it (the
 * state of a new engine: every byte as before).  What depends on the image (component count,
 * precision, sign) is checked by the call that writes the boxes, before anything is allocated.  A
 * refused spec leaves the engine with none. */
int gk_set_encode_colour(gk_ctx* ctx, const gk_encode_colour* spec);
/* gk_jp2_header without an engine (no device needed): the JP2 boxes in front of a codestream of
 * cs_len bytes for the image `info` under `spec` (NULL: ihdr + the default colr).  Returns 0, -2 if
 * cap is too small (*out_len = needed), -1 with the refusal in msg. */
int gk_jp2_boxes(const gk_image_info* info, const gk_encode_colour* spec, uint64_t cs_len, uint8_t* out, size_t cap,
                 size_t* out_len, char* msg, size_t msg_cap);

/* R, G, B in, sYCC out: the mirror of GK_DISPLAY_RGB's sYCC / e-sYCC conversions, done by the
 * device in front of the encode (k_rgb_ycc).  Grok has no forward conversion to restate (grk_compress
 * takes subsampled raw YUV, -F); the arithmetic is the engine's own, in integers, p = precision,
 * offset = 2^(p-1), upb = 2^p - 1:
 *   Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16                                    per pixel
 *   Cb = floor((-11059 SR - 21709 SG + 32768 SB + 2^(s-1)) / 2^s) + offset, clamped to [0, upb]
 *   Cr = floor(( 32768 SR - 27439 SG -  5329 SB + 2^(s-1)) / 2^s) + offset, clamped to [0, upb]
 * SR, SG, SB: the sums over the chroma sample's box of n = 1, 2 or 4 pixels, s = 16 + log2(n).
 * Chroma sample (i, j) takes image columns chroma_dx * j + ofx .. + chroma_dx - 1 and rows likewise,
 * cut at the image's edge; ofx = x0 & 1 when chroma_dx = 2 (ofy likewise): column 0 under an odd x0
 * and row 0 under an odd y0 belong to no box and give luma only, the pixels sycc422_to_rgb /
 * sycc420_to_rgb convert without a chroma sample.  e-sYCC: the same formulas (unsigned chroma).
 * While a conversion is set, gk_encode_pixels with 3 channels and gk_encode with three planes of the
 * image's size (host or device; u8 / u16 / int32 by gk_image_info::sample_bytes) convert into the
 * engine's planes and encode them exactly as gk_encode does under gk_set_subsampling(3, {1, dx, dx},
 * {1, dy, dy}) with colour space `space`: the MCT is cleared, a JP2 file gets colr EnumCS 18 / 24, an
 * encode colour of the same space is honoured (its cdef), every coding parameter, origin and tile
 * grid too; the stream is byte for byte the planar encode of the planes defined above.
 * Refused, each by name, before anything is allocated or launched: a space other than
 * GRK_CLRSPC_SYCC (4) / GRK_CLRSPC_EYCC (5); (chroma_dx, chroma_dy) other than (1, 1), (2, 1), (2, 2);
 * e-sYCC with subsampled chroma; a channel count other than 3; signed samples; a precision above 16;
 * an active gk_set_subsampling (the only way to hand over planes of different sizes); an encode
 * colour of another colour space or with a palette; gk_encode_tiles / gk_encode_blocks /
 * gk_main_header while a conversion is set; whatever the subsampled planar encode refuses (a tile
 * size the factors do not divide). */
typedef struct gk_encode_convert {
    uint32_t space;                  /* 0 none, GRK_CLRSPC_SYCC (4), GRK_CLRSPC_EYCC (5) */
    uint32_t chroma_dx, chroma_dy;
} gk_encode_convert;
/* Sticky; spec = NULL (or space 0) clears it: every call is then byte for byte as without.  A
 * refused spec leaves none set.  No encode changes it. */
int gk_set_encode_convert(gk_ctx* ctx, const gk_encode_convert* spec);
/* What an encode of `info` under `spec` codes, no device needed: the components' dx / dy and plane
 * sizes cw x ch (any may be NULL); 0, or -1 with the refusal in msg. */
int gk_probe_encode_convert(const gk_image_info* info, const gk_encode_convert* spec, uint32_t dx[3], uint32_t dy[3],
                            uint32_t cw[3], uint32_t ch[3], char* msg, size_t msg_cap);

/* A shaped region of interest (ISO 15444-1 Annex H, maxshift): the samples of a region, given as
 * rectangles and / or a mask, are coded ahead of the background.  Grok's -ROI (roi_compno /
 * roi_shift above) makes a whole component the region; it has no counterpart to this, so the
 * region's arithmetic is the standard's (H.3): per tile-component and decomposition level, in that
 * level's interleaved canvas coordinates k (even low-pass, odd high-pass), a region sample at k
 * needs the coefficients at k + d, |d| <= 1 (k even) or 2 (k odd) for 5/3, 3 or 4 for 9/7, indices
 * outside the tile-component reflected whole-sample symmetrically (an interval of one sample needs
 * itself); two dimensions are the product; the low/low positions are the next level's samples.  The
 * T1 encoders scale exactly those coefficients of the listed components up by 2^shift; the band
 * bit-plane counts rise by the shift for the whole component and one RGN marker (Srgn 0) is
 * written per listed component, so the stream is a plain Part-1 / Part-15 maxshift stream and any
 * decoder separates region from background by magnitude.  The masks are computed on the device
 * inside the encode (k_roi_fill, k_roi_level).
 * shift = 0 takes, per component, the smallest legal shift: the largest band bit-plane count of
 * the component without ROI (a background magnitude then stays below 2^shift).
 * Refused, each by name, by the encode (before anything is allocated or launched) and by
 * gk_probe_encode_roi alike: a region together with roi_compno / roi_shift; an empty rectangle or
 * one that leaves the image; a mask whose size is not the image's; a component index past the
 * last; an empty region (no rectangle and no non-zero mask byte); subsampled components
 * (gk_set_subsampling, gk_set_encode_convert with subsampled chroma); an explicit shift below the
 * smallest legal one; "ROI shift too large for this precision" (a band of more than 25 bit-planes,
 * shift included); gk_encode_tiles and gk_main_header while a region is set (sharded encodes are
 * out of scope).  TERMALL: the code-block slots of a component with an ROI shift are enlarged by
 * the terminations its extra passes can cost. */
typedef struct gk_rect {
    uint32_t x0, y0, x1, y1;   /* half-open, in samples from the image's top-left sample (not canvas coordinates) */
} gk_rect;
typedef struct gk_encode_roi {
    uint32_t shift;            /* RGN SPrgn of the listed components; 0: the smallest legal shift of each */
    uint32_t num_comps;        /* entries of comps; 0: every component carries the region */
    const uint32_t* comps;
    uint32_t num_rects;
    const gk_rect* rects;
    const uint8_t* mask;       /* NULL, or mask_h rows of mask_w bytes, mask_row_bytes apart: non-zero = region */
    uint32_t mask_w, mask_h;   /* must be the image's w / h */
    size_t mask_row_bytes;
    int mask_on_device;
} gk_encode_roi;
/* Sticky, like gk_set_encode_colour: later gk_encode / gk_encode_pixels calls (host or device
 * input and output, .j2k and .jp2) code the region, the union of the rectangles and the mask.
 * Everything is copied (the mask to the device).  roi = NULL clears it: every byte as before.  What
 * depends on the image is checked by the encode.  A refused description leaves the engine with
 * none. */
int gk_set_encode_roi(gk_ctx* ctx, const gk_encode_roi* roi);
/* What an encode of `info` under `params` and `roi` would answer, no engine or device needed: 0
 * and, in shift_out[c] (NULL, or info->numcomps entries), the shift each component gets (0: the
 * component does not carry the region); -1 with the refusal in msg.  A mask in device memory is
 * judged by its size alone (its bytes cannot be read without a device). */
int gk_probe_encode_roi(const gk_image_info* info, const gk_cparameters* params, const gk_encode_roi* roi,
                        uint32_t* shift_out, char* msg, size_t msg_cap);
/* The coefficient mask of one band under the engine's current region, computed by the kernels the
 * encode runs: band `band` (resolution 0: 0 = LL; above: 0 HL, 1 LH, 2 HH) of resolution
 * `resolution` of tile `tile` (raster index) of component `comp`, as *w x *h bytes (1 = region),
 * rows *w apart, in out (device memory if out_on_device).  Returns 0, -2 when cap is below
 * *w * *h (both still set), -1 on error (no region set; an index out of range; whatever the encode
 * refuses).  A diagnostic: what a region costs in coefficients. */
int gk_roi_band_mask(gk_ctx* ctx, const gk_image_info* info, const gk_cparameters* params, uint32_t comp, uint32_t tile,
                     uint32_t resolution, uint32_t band, uint8_t* out, size_t cap, uint32_t* w, uint32_t* h,
                     int out_on_device);

/* The quantisation step of HTJ2K 9/7 encodes: to a chosen step, size or PSNR.  An HT block has one
 * pass, so its step is the only rate knob (layer_rate cannot cut a block); Grok's encoder has one
 * operating point, base step 2^-(prec + sgnd) (HTParams.cpp:211-212), and no option to move it
 * (OpenJPH has -qstep, Kakadu Qstep and -rate).  Band b is quantised with base_step / (gl gh), its
 * 9/7 synthesis gain, exactly as Grok derives its own steps; the QCD is scalar expounded and holds
 * the (exponent, mantissa) pair of every band, and the encoder quantises with the step that pair
 * represents, so any decoder reconstructs on the encoder's grid.
 * The ladder: notch n has base_step = 2^-(prec + sgnd) * 2^(n / 8), n = 0 .. 8 (prec - 1); at its top
 * every band still has an exponent >= 1, i.e. a bit-plane.
 * GK_QUANT_STEP: a plain encode with that base step, anywhere in [step(0), step(top)] (at step(0)
 * the stream is byte for byte the one without a setting).
 * GK_QUANT_BYTES: the finest notch whose stream (the .jp2 file when one is written) is at most
 * value bytes: MCT and DWT run once, the HT pass alone repeats, bisecting the ladder with the
 * pass's length summed on the device (k_htq_len).  Passes: ceil(log2(notches + 1)) probes, one
 * more when the last probe was not the chosen notch, and one per exact-length correction (the
 * probes count a lower bound of the packet headers; the final length is checked exactly and a
 * notch that is over moves one coarser).  That is 2 + ceil(log2(notches)) with at most one
 * correction, what the tests hold it to; 6 to 8 were measured, gk_quant_result says how many.
 * GK_QUANT_PSNR: one pass over the float coefficients (k_htq_dist) gives the squared quantisation
 * error of every band at every notch; weighted by the bands' energy gains (and the inverse ICT's
 * column norms), plus 1/12 for the decoder's rounding, it estimates the image-domain MSE; the
 * coarsest notch whose estimate reaches value dB against the source samples is encoded, once.
 * Refused, each by name, by the encode (before anything is allocated or launched) and by
 * gk_probe_encode_quant alike: a mode other than the three, a value that is not finite and
 * positive; a Part-1 or a reversible encode while a setting is held; numlayers > 1, layer_rate or
 * allocationByQuality with it; a step outside the ladder's range (finer than the default is out of
 * scope: DESIGN.md §7); GK_QUANT_BYTES / GK_QUANT_PSNR with gk_encode_tiles or gk_main_header (a
 * shard cannot know the other shards' bytes; GK_QUANT_STEP works there); gk_encode_blocks; a byte
 * target that the coarsest notch still exceeds (the probe knows the headers' share alone).
 * Composes with tiles, TLM / PLT, JP2 and its colour boxes, gk_encode_pixels,
 * gk_set_encode_convert and gk_set_encode_roi.  gk_transcode keeps a QCD as it is. */
#define GK_QUANT_STEP  1u  /* value = base step, nominal-range units (the default is 2^-(prec+sgnd)) */
#define GK_QUANT_BYTES 2u  /* value = largest output length in bytes (codestream, or the whole .jp2 file) */
#define GK_QUANT_PSNR  3u  /* value = PSNR in dB against the source samples */
/* gk_probe_encode_quant only, or-ed into mode: answer for gk_encode_tiles / gk_encode_blocks */
#define GK_QUANT_FOR_TILES  0x100u
#define GK_QUANT_FOR_BLOCKS 0x200u
typedef struct gk_encode_quant { uint32_t mode; double value; } gk_encode_quant;
/* Sticky; quant = NULL clears it: every call is then byte for byte as without.  A refused setting
 * leaves none.  No encode changes it, and no result depends on what the engine encoded before. */
int gk_set_encode_quant(gk_ctx* ctx, const gk_encode_quant* quant);
/* What an encode of `info` under `params` and `quant` would answer, no engine or device needed:
 * 0 and the ladder's ends *step_min = step(0), *step_max = step(top) and its length *notches (any
 * may be NULL; quant may be NULL to ask for the ladder alone); -1 with the refusal in msg. */
int gk_probe_encode_quant(const gk_image_info* info, const gk_cparameters* params, const gk_encode_quant* quant,
                          double* step_min, double* step_max, uint32_t* notches, char* msg, size_t msg_cap);
typedef struct gk_quant_result {
    uint32_t mode, notch;    /* the setting's mode (0: none was set); the notch used (STEP: the last one not coarser) */
    uint32_t t1_passes;      /* HT encode passes the call ran (1 in STEP mode) */
    uint32_t stats_passes;   /* k_htq_dist passes over the coefficients (ladder launches counted once); with the
                                search's passes they are part of gk_timings::t1_ms */
    double base_step;        /* the step used */
    double est_mse;          /* estimate for the chosen step */
    double est_psnr;         /* estimate for the chosen step */
    double est_psnr_next;    /* estimate for the next coarser notch (0 at the top of the ladder) */
    uint64_t bytes;          /* output length */
} gk_quant_result;
/* Of the last gk_encode / gk_encode_pixels / gk_encode_tiles (zeros after one without a setting). */
int gk_get_encode_quant(gk_ctx* ctx, gk_quant_result* result);

/* grk_decompress_read_header (grok.cpp:287-297, CodeStreamDecompress::readHeader) of a raw
 * codestream or a JP2 file (its jp2c box; FileFormatDecompress::read_box_hdr :632-672). */
int gk_decode_header(gk_ctx* ctx, const uint8_t* cs, size_t len, int cs_on_device, gk_image_info* info);

/* The same header parse on host bytes without an engine (no device needed): image info of a
 * codestream / JP2 file and, when coding != NULL, its coding style in gk_cparameters terms
 * (CodeStreamDecompress main-header markers; what grk_decompress_read_header reports in
 * grk_header_info), or < 0 with the reason in msg. */
int gk_probe_header(const uint8_t* cs, size_t len, gk_image_info* info, gk_cparameters* coding, char* msg,
                    size_t msg_cap);

/* grk_decompress (grok.cpp:287-297; TileProcessor::decompressT2T1 TileProcessor.cpp:384-408):
 * decode into comps[c] (device memory if out_on_device): int32 planes (sample_bytes 0 / 4) or planar
 * (prec + 7) / 8-byte samples (sample_bytes 1 / 2, signed iff the image is; gk_image_info).  Every tile
 * part present in cs is decoded; a stream holding the main header and only some
 * tile parts (tile sharding, window decode) writes only those tiles' samples. */
int gk_decode(gk_ctx* ctx, const uint8_t* cs, size_t len, int cs_on_device, void* const* comps,
              const uint32_t* strides, uint32_t sample_bytes, int out_on_device);

/* grk_dparameters::cp_layer (CodeStreamDecompress.cpp:2570-2579): later gk_decode /
 * gk_decode_window calls decode only the first max_layers quality layers (0 = all); packets of
 * later layers are skipped through PLT or parsed without their data (T2Decompress.cpp:55-116). */
int gk_set_decode_layers(gk_ctx* ctx, uint32_t max_layers);

/* grk_dparameters::cp_reduce (CodeStreamDecompress / TileComponent resolutions_to_decompress):
 * later gk_decode calls discard the `reduce` highest resolutions: packets of those resolutions
 * are skipped, the inverse DWT stops `reduce` levels early and the output planes are
 * ceil(w / 2^reduce) x ceil(h / 2^reduce) (0 = full resolution); gk_decode_window then returns
 * the window on the reduced canvas (every edge of its canvas rectangle ceil(x / 2^reduce),
 * CodeStreamDecompress.cpp:471-481). */
int gk_set_decode_reduce(gk_ctx* ctx, uint32_t reduce);

/* grk_image_comp::dx / dy of the components of later gk_encode / gk_encode_tiles / gk_main_header calls (SIZ XRsiz /
 * YRsiz, 1..255; numcomps = 0 clears it).  Component c's plane then holds the image area sampled
 * every (dx[c], dy[c]) canvas positions: ceil((x0 + w) / dx) - ceil(x0 / dx) columns and the same
 * in y (grk_image_comp w / h), row stride strides[c].  Its tile-components are the tiles divided
 * by (dx, dy), rounded up (TileProcessor.cpp:116-131); the MCT is cleared unless the first three
 * components share a grid (CodeStreamCompress.cpp:501-512); rate control takes component 0's
 * factors (updateRates :961).  Tiled images need each factor to divide the tile size.  With
 * gk_encode_tiles, comps[c] addresses component c's plane at its row 0 and only the rows of the
 * selected tiles (on that component's grid) are read. */
int gk_set_subsampling(gk_ctx* ctx, uint32_t numcomps, const uint32_t* dx, const uint32_t* dy);

/* A stream's components from its header, no device needed (SIZ XRsiz / YRsiz / Ssiz): fills dx[c],
 * dy[c], prec[c], sgnd[c] (any may be NULL) for the first cap components and returns the component
 * count (< 0 on error).  gk_decode writes component c into a plane of its own size: the image area
 * divided by (dx, dy) as in gk_set_subsampling, then reduced by cp_reduce (ceil of both edges /
 * 2^reduce); windows take the window's rectangle on each component's grid.  Components of
 * different precisions are DC-shifted and clamped each by its own (gk_image_info::prec reports the
 * largest; 8 / 16-bit output needs one sign). */
int gk_probe_components(const uint8_t* cs, size_t len, uint32_t* dx, uint32_t* dy, uint32_t* prec, uint32_t* sgnd,
                        uint32_t cap);

/* The same for the stream the last gk_decode_header read (host or device bytes); returns the
 * component count. */
int gk_header_components(gk_ctx* ctx, uint32_t* dx, uint32_t* dy, uint32_t* prec, uint32_t* sgnd, uint32_t cap);

/* JP2 colour boxes (jp2h: colr, pclr, cmap, cdef; FileFormatDecompress::readHeader :198-280 and
 * applyColour :378-401).  A decode applies them as Grok's library does: a palette (pclr + cmap)
 * expands the mapped components into its columns (apply_palette_clr :1299-1436, indices clamped
 * to the palette) and a cdef reorders the channels (apply_channel_definition :876-930), so
 * gk_decode_header / gk_probe_header report the OUTPUT channel count and the widest channel
 * precision, gk_header_components / gk_probe_components each channel's precision and sign, and
 * gk_decode / gk_decode_window write one plane per output channel (8 / 16-bit planes sized by the
 * widest channel).  Files without pclr + cmap / cdef, and raw codestreams, decode as before. */
#define GK_MAX_CHANNELS 256   /* channels described in gk_colour_info (more are counted, not described) */
typedef struct gk_colour_info {
    uint32_t colour_space;     /* GRK_COLOR_SPACE: 0 unknown, 2 sRGB, 3 grey, 4 sYCC, 5 e-YCC, 6 CMYK, 7 default CIELab,
                                  8 custom CIELab (colr EnumCS 14; gk_header_cielab), 9 ICC */
    uint32_t enumcs;           /* colr EnumCS as read (METH 1), else 0 */
    uint32_t meth;             /* colr METH of the accepted box (1 / 2), 0: none accepted */
    uint32_t icc_len;          /* bytes of the METH 2 profile (gk_header_icc) */
    uint32_t has_palette;      /* pclr + cmap present and applied */
    uint32_t palette_entries, palette_columns;   /* pclr NE / NPC (also of a pclr dropped for want of a cmap) */
    uint32_t has_cdef;         /* cdef present and applied */
    uint32_t num_comps;        /* components of the codestream */
    uint32_t num_channels;     /* output channels */
    uint16_t typ[GK_MAX_CHANNELS];    /* per output channel: cdef Typ (0 colour, 1 opacity, 2 premultiplied opacity, */
    uint16_t asoc[GK_MAX_CHANNELS];   /* 65535 unspecified) and Asoc (0 whole image, 1..3 colour, 65535 none);
                                         without a cdef Grok's defaults: colour 1..3, then unspecified */
    uint32_t display_applied;  /* gk_set_decode_display: GK_DISPLAY_RGB set when a conversion to RGB runs,
                                  GK_DISPLAY_UPSAMPLE when components are upsampled, GK_DISPLAY_FORCE_RGB when
                                  a grey channel is replicated, GK_DISPLAY_ICC when an ICC profile or CIELab is
                                  converted to sRGB (0 without flags) */
} gk_colour_info;
/* Colour description of host codestream / JP2 bytes, no device needed (like gk_probe_header);
 * < 0 with the reason, naming the box, in msg. */
int gk_probe_colour(const uint8_t* cs, size_t len, gk_colour_info* info, char* msg, size_t msg_cap);
/* The ICC profile of host JP2 bytes, no device needed: as gk_header_icc. */
int gk_probe_icc(const uint8_t* cs, size_t len, uint8_t* buf, size_t cap, size_t* icc_len);
/* gk_probe_components for the codestream's own components, the colour boxes not applied (what a
 * header read shows before Grok's applyColour has run). */
int gk_probe_stream_components(const uint8_t* cs, size_t len, uint32_t* dx, uint32_t* dy, uint32_t* prec,
                               uint32_t* sgnd, uint32_t cap);
/* gk_probe_colour for the stream the last gk_decode_header read. */
int gk_header_colour(gk_ctx* ctx, gk_colour_info* info);
/* Its ICC profile (colr METH 2; grk_image_meta's color.icc_profile_buf): *len receives the size,
 * the bytes are copied when cap holds them (-2 otherwise). */
int gk_header_icc(gk_ctx* ctx, uint8_t* buf, size_t cap, size_t* len);
/* The CIELab parameters of that stream (colr EnumCS 14) as Grok keeps them in icc_profile_buf
 * (FileFormatDecompress::read_colr :1076-1123): 14, GRK_DEFAULT_CIELAB_SPACE (0x44454600) or
 * GRK_CUSTOM_CIELAB_SPACE (0), then rl, ol, ra, oa, rb, ob, il.  *n receives the word count: 2 for
 * the 7-byte box (and any other size but 35: the default space), 9 for the 35-byte one, 0 for a
 * stream that is not CIELab. */
int gk_header_cielab(gk_ctx* ctx, uint32_t words[9], uint32_t* n);
/* The same for host JP2 bytes, no device needed. */
int gk_probe_cielab(const uint8_t* cs, size_t len, uint32_t words[9], uint32_t* n);
/* apply = 1 (default): later gk_decode_header / gk_decode / gk_decode_window calls apply the
 * palette and channel definition.  apply = 0: they return the codestream's components untouched
 * (the colour description is still read). */
int gk_set_decode_colour(gk_ctx* ctx, int apply);

/* What Grok's CLI does to the decoded image before it writes it (GrkDecompress::postProcess,
 * bin/jp2/grk_decompress.cpp:1300-1506), done on the device by later gk_decode / gk_decode_window
 * calls.  flags = 0 (default): the components as decoded.
 * GK_DISPLAY_RGB: sYCC (4:4:4, 4:2:2, 4:2:0), e-sYCC and CMYK images are converted to RGB
 * (color_sycc_to_rgb, color_esycc_to_rgb, color_cmyk_to_rgb, bin/common/color.cpp) by
 * postProcess's rule: a 3-component image whose component 0 has dx == dy and component 1 dx != 1
 * is taken as sYCC whatever its colr box says, otherwise one of <= 2 components as grey; an sYCC
 * image with another subsampling pattern, or an e-sYCC / CMYK image that fails
 * all_components_sanity_check (precision 1..16, one precision, one sign), stays unconverted.
 * GK_DISPLAY_UPSAMPLE: components with dx > 1 or dy > 1 are then replicated to the image grid
 * (upsample_image_components, bin/common/convert.cpp:209-360; grk_decompress -u), the window's with
 * a window; refused together with gk_set_decode_reduce > 0.
 * While flags are set the header calls (gk_decode_header, gk_header_components, gk_header_colour
 * and gk_probe_display) describe the OUTPUT: channel count, each channel's dx / dy / precision /
 * sign, the colour space (sRGB after a conversion that ran) and gk_colour_info::display_applied.
 * Refused, each by name: a channel count other than 3 (sYCC, e-sYCC) or 4 (CMYK); signed
 * components into the sYCC or CMYK conversion; a window or reduction that leaves the chroma planes
 * of 4:2:2 / 4:2:0 other than ceil((w - ox) / 2) [x ceil((h - oy) / 2)] for a w x h luma plane
 * (ox, oy: the origin's parities, cleared by a window edge that is not the image's); e-sYCC / CMYK
 * components of different sizes; a palette or channel definition on a file that would be
 * converted; a stream that holds only some of its tiles; 8 / 16-bit planes that are not
 * (output precision + 7) / 8 bytes. */
#define GK_DISPLAY_RGB 1u
#define GK_DISPLAY_UPSAMPLE 2u
/* GK_DISPLAY_FORCE_RGB (grk_decompress -f; postProcess :1444-1468, convert_gray_to_rgb,
 * bin/common/convert.cpp:148-207), evaluated after the GK_DISPLAY_RGB conversion.  The colour-space
 * rule of :1335-1341 (a 3-component image with subsampled chroma counts as sYCC, one of <= 2
 * components as grey) is applied when GK_DISPLAY_RGB or GK_DISPLAY_FORCE_RGB is set.  An sRGB image
 * is left alone.  A grey image's channel 0 becomes three channels with its dx / dy / precision /
 * sign / typ, the remaining channels follow with their own (grey + alpha: R, G, B, A), the colour
 * space becomes sRGB and display_applied gains this bit; the grey plane is read once by the
 * output stage, not copied.  Every other colour space is refused by name (Grok: "don't know how to
 * convert image to RGB colorspace"): unknown (a raw codestream of >= 3 components), sYCC or CMYK
 * left unconverted (add GK_DISPLAY_RGB), e-sYCC, ICC, CIELab. */
#define GK_DISPLAY_FORCE_RGB 4u
/* GK_DISPLAY_ICC: colour management, where postProcess does it (:1390-1443): after the
 * GK_DISPLAY_RGB conversions, before GK_DISPLAY_FORCE_RGB, the upsampling, the precision list and
 * the pixel pack.  A tensor cannot embed a profile, so this is the CLI's behaviour for an output
 * format that cannot either.
 * A file whose colr box carries an ICC profile (METH 2; color_apply_icc_profile,
 * bin/common/color.cpp:423-776) of the two classes Part 1 allows there: channels 0..2 (data colour
 * space 'RGB ', rXYZ / gXYZ / bXYZ + rTRC / gTRC / bTRC) or channel 0 ('GRAY', kTRC) become sRGB at
 * the same precision p: v / (2^p - 1) -> tone curve -> colorants -> inverse of lcms2's sRGB
 * colorants -> clip to [0, 1] -> sRGB encoding -> * (2^p - 1), rounded half up, p = 1..16.  Curves:
 * 'curv' (identity, gamma, table with linear interpolation) and 'para' types 0..4; the header's
 * rendering intent changes nothing for these classes.  Further channels (opacity through a cdef)
 * pass through.  A grey profile takes 1 or 2 channels and leaves the colour space grey (with
 * GK_DISPLAY_FORCE_RGB the result is replicated: R, G, B, then the other channel, sRGB).
 * A CIELab file (colr EnumCS 14; color_cielab_to_rgb :779-964): L*, a*, b* through their ranges and
 * offsets (the default ones, or the 35-byte box's), to XYZ under D50 (the illuminant word has no
 * effect on lcms2's result), to sRGB; channels 0..2 become 16-bit unsigned.
 * Above 8 bits Grok's own arithmetic is defective; the engine computes on
 * v / (2^p - 1) and agrees with lcms2 run unoptimised.
 * The header calls describe the output (colour space sRGB, or grey for a grey profile; precisions;
 * display_applied gains this bit when a conversion runs).  A file with neither a METH 2 profile nor
 * EnumCS 14 is untouched and the bit stays clear; so is an RGB-profile image whose first
 * min(channels, 4) channels differ in dx / dy / precision / sign, or any image whose channels are
 * not of one precision and sign (Grok's silent return).
 * Refused, each by name: bytes that are not a profile (no 'acsp', a size field past the box, a tag
 * table or a tag outside the profile, a curve count that overruns its tag); a profile with A2B0 /
 * A2B1 / A2B2 (lcms2 would use the table); a data colour space other than 'RGB ' / 'GRAY'; a
 * connection space other than 'XYZ '; a missing colorant or curve tag; an unknown curve type; signed
 * channels; a precision above 16; an RGB profile or CIELab on fewer than 3 channels, a grey profile
 * on more than 2; subsampled components; a palette; a stream that holds only some of its tiles;
 * 8 / 16-bit planes that are not (output precision + 7) / 8 bytes (CIELab output is 16-bit). */
#define GK_DISPLAY_ICC 8u
int gk_set_decode_display(gk_ctx* ctx, uint32_t flags);
/* What a decode of host codestream / JP2 bytes under `flags` and `reduce` returns, no device
 * needed: the image info and colour description of the output (either may be NULL), dx / dy /
 * prec / sgnd of the first cap channels (any may be NULL); returns the channel count, or < 0 with
 * the refusal in msg.  flags = 0, reduce = 0: what gk_probe_header / gk_probe_colour /
 * gk_probe_components report. */
int gk_probe_display(const uint8_t* cs, size_t len, uint32_t flags, uint32_t reduce, gk_image_info* info,
                     gk_colour_info* colour, uint32_t* dx, uint32_t* dy, uint32_t* prec, uint32_t* sgnd, uint32_t cap,
                     char* msg, size_t msg_cap);

/* Forced output precision (grk_decompress -p; postProcess :1469-1494, grk_precision /
 * grk_precision_mode).  Sticky; n = 0 clears the list.  Output channel k (counted after the colour
 * boxes, the conversion and grey to RGB) takes entry min(k, n - 1); prec = 0 keeps the channel's
 * precision; the channel's reported precision becomes the forced one.
 * GK_PREC_SCALE is scale_component (bin/common/convert.cpp:96-146): equal precisions untouched;
 * up: lrintf((float)v * scale), scale = (float)newMax / (float)oldMax a float32 quotient taken on
 * the host, max = 2^p - 1 unsigned, 2^(p - 1) signed; down: C division by 2^(old - new), truncating
 * toward zero.
 * GK_PREC_CLIP clamps to the forced precision's range with the channel's sign, [0, 2^p - 1] or
 * [-2^(p - 1), 2^(p - 1) - 1] (Grok's clip<T>, :1476-1486, clamps to the limits of the 32-bit type
 * and so changes no sample: DESIGN.md R-BUG-11).
 * Entries are 0..16 and a channel that gets a forced precision must itself be <= 16 bits (the
 * CLI's limit :1249-1258); otherwise the header and decode calls refuse, naming the channel,
 * before anything is allocated or launched.  The list applies to gk_decode / gk_decode_window
 * (planar) and to the pixel calls; the header calls describe the output, and the plane-size rule
 * (8 / 16-bit planes of (widest output precision + 7) / 8 bytes) follows the forced precision. */
#define GK_PREC_CLIP 0u    /* GRK_PREC_MODE_CLIP */
#define GK_PREC_SCALE 1u   /* GRK_PREC_MODE_SCALE */
typedef struct gk_precision {
    uint8_t prec;
    uint8_t mode;
} gk_precision;
int gk_set_decode_precision(gk_ctx* ctx, const gk_precision* list, uint32_t n);

/* gk_probe_display with a precision list: what a decode under `flags`, `reduce` and the list
 * returns, no device needed.  n = 0: what gk_probe_display reports. */
int gk_probe_output(const uint8_t* cs, size_t len, uint32_t flags, uint32_t reduce, const gk_precision* list,
                    uint32_t n, gk_image_info* info, gk_colour_info* colour, uint32_t* dx, uint32_t* dy, uint32_t* prec,
                    uint32_t* sgnd, uint32_t cap, char* msg, size_t msg_cap);

/* Decode to packed pixels: the image Grok's image writers are handed after postProcess
 * (interleaving as in bin/image_format, e.g. PNGFormat / TIFFFormat's planar-to-interleaved
 * pass), written by the device.  Sample k of pixel (x, y) lies at
 * pixels + y * row_bytes + (x * C + k) * es; C is the output channel count the header calls report,
 * es = sample_bytes (0 or 4: int32; 1 / 2: (widest output precision + 7) / 8, one sign).  Row bytes
 * past w * C * es are never written.  Every sticky setting is honoured (layers, reduce, colour
 * boxes, display flags, precision list, window rule).  Refused, each by name: output channels of
 * different sizes (subsampled components without GK_DISPLAY_UPSAMPLE); a sample_bytes that breaks
 * the rule or mixes signs in 8 / 16 bits; row_bytes below w * C * es or no multiple of es; more
 * than 16 output channels (use the planar calls); a stream that holds only some of its tiles. */
int gk_decode_pixels(gk_ctx* ctx, const uint8_t* cs, size_t len, int cs_on_device, void* pixels, size_t row_bytes,
                     uint32_t sample_bytes, int out_on_device);
/* The same for the window [x0, x1) x [y0, y1) (gk_decode_window): pixels addresses sample (x0, y0). */
int gk_decode_window_pixels(gk_ctx* ctx, const uint8_t* cs, size_t len, int cs_on_device, uint32_t x0, uint32_t y0,
                            uint32_t x1, uint32_t y1, void* pixels, size_t row_bytes, uint32_t sample_bytes,
                            int out_on_device);

/* Decode a view: a region of the image at exactly out_w x out_h pixels, mirrored and rotated, as
 * packed pixels in one call (the IIIF Image API's region / size / rotation; Grok's CLI has the
 * region, -d, and the power-of-two reduction, -r, only).  The rules are the engine's own:
 * The size.  W x H: the region at full resolution.  Both sizes given and fit = 0: as given (the
 * aspect may change).  out_h = 0: out_h = max(1, (2 out_w H + W) / (2 W)); out_w = 0 likewise.
 * fit = 1 with both given: if out_w H <= out_h W the width is kept and the height derived as above,
 * otherwise the height is kept and the width derived.
 * The reduce level.  The largest r that gk_set_decode_reduce accepts for the stream (below its
 * smallest resolution count; 0 under GK_DISPLAY_UPSAMPLE) at which the reduced region, every edge
 * of its canvas rectangle ceil(x / 2^r), is still at least out_w wide and out_h high.
 * The decode.  The window path at r, under every sticky setting (layers, window rule, colour boxes,
 * display flags, precision list), leaves the reduced region, rw x rh, as packed int32 pixels in an
 * engine-owned device buffer: the samples gk_decode_window_pixels returns with sample_bytes 0 under
 * gk_set_decode_reduce(r) (a region given as all 0: gk_decode_pixels').  k_view (gk_view.hip) then
 * writes the caller's pixels.
 * The resampling.  An exact area average on the reduced region.  In units of 1 / out_w, output
 * column i covers [i rw, (i + 1) rw) and source column s covers [s out_w, (s + 1) out_w); the
 * weight wx(i, s) is the length of their overlap, an integer, and a column's weights sum to rw;
 * rows alike.  Per channel, in signed 64-bit integers,
 *   out = floor((2 sum(wy wx v) + rw rh) / (2 rw rh))            (floor division; halves round up)
 * so equal sizes copy the samples, an integer ratio gives the rounded block mean and a constant
 * image stays constant.
 * The orientation.  mirror: column i becomes out_w - 1 - i; the result is then rotated clockwise by
 * `rotate` degrees (numpy: rot90(fliplr(a), k = -rotate / 90)); 90 and 270 swap the written
 * image's width and height.
 * pixels, row_bytes, sample_bytes, out_on_device: as gk_decode_pixels, for the written image of
 * pix_w x pix_h pixels; row bytes past pix_w * C * es are never written.
 * Refused, each by name, before anything is allocated or launched, and leaving the engine's state
 * as it was: a non-zero gk_set_decode_reduce (the view chooses the level); a rotate other than 0,
 * 90, 180, 270; mirror or fit above 1; a region that is empty or leaves the image; upscaling
 * (out_w > W or out_h > H); both sizes 0; whatever gk_decode_window_pixels refuses from the
 * header (subsampled channels without GK_DISPLAY_UPSAMPLE, more than 16 channels, the row_bytes /
 * sample_bytes rules); a source with (rw rh) << prec >= 2^62 (the accumulator); an output of
 * 2^24 tiles of 16 x 16 pixels or more.  One refusal comes later, where gk_decode_pixels makes it:
 * a stream that holds only some of its tiles is found once its tile parts are located, after the
 * engine's buffers have grown and before any kernel runs; it too changes no setting.  gk_get_timings afterwards: the decode's, with the view pass added to mct_ms and
 * total_ms as the output pass is. */
typedef struct gk_view {
    uint32_t x0, y0, x1, y1;   /* region: gk_decode_window's rectangle convention; all 0 = whole image */
    uint32_t out_w, out_h;     /* size before rotation; one of them may be 0 (kept aspect) */
    uint32_t fit;              /* 1: the largest size of the region's aspect inside out_w x out_h (IIIF "!w,h") */
    uint32_t rotate;           /* 0, 90, 180, 270, clockwise */
    uint32_t mirror;           /* 1: mirror left-right before rotating (IIIF "!n") */
} gk_view;
typedef struct gk_view_result {
    uint32_t reduce;                 /* resolutions discarded */
    uint32_t rx0, ry0, rx1, ry1;     /* the region on the reduced canvas (every edge ceil(x / 2^reduce)) */
    uint32_t out_w, out_h;           /* resolved size before rotation */
    uint32_t pix_w, pix_h;           /* size of the written image (swapped for 90 / 270) */
    uint32_t channels, prec, sgnd;   /* as the header calls report under the sticky settings */
} gk_view_result;
/* What gk_decode_view_pixels would answer for host bytes under these display flags and this
 * precision list (n = 0: none), no device needed: 0 and *res, or -1 with the refusal in msg.  (The
 * sticky reduce and the caller's buffer are the decode's to judge.) */
int gk_probe_view(const uint8_t* cs, size_t len, uint32_t display_flags, const gk_precision* list, uint32_t n,
                  const gk_view* v, gk_view_result* res, char* msg, size_t msg_cap);
int gk_decode_view_pixels(gk_ctx* ctx, const uint8_t* cs, size_t len, int cs_on_device, const gk_view* v,
                          void* pixels, size_t row_bytes, uint32_t sample_bytes, int out_on_device,
                          gk_view_result* res /* may be NULL */);

/* Render for display: the int32 pixels of the pixel calls (gk_decode_pixels,
 * gk_decode_window_pixels, gk_decode_view_pixels) become unsigned 8-bit display pixels on the
 * device, by the engine's own integer rule (Grok's CLI stops at -p).  Sticky and
 * copied in; NULL or mode 0 clears it; a refused description leaves the previous one.
 * Input: the int32 sample v of output channel k exactly as the same call delivers it with
 * sample_bytes 0 and no render (after colour boxes, display flags and the precision list; for a
 * view after the area average).  Channel k takes entry min(k, n - 1) of ch.
 * Window (lo, hi), lo < hi, any int32 pair, in signed 64-bit integers:
 *   u = min(max(v, lo), hi),  t = floor((2 * 255 * (u - lo) + (hi - lo)) / (2 * (hi - lo)))
 * (0, 4095): 2048 -> 128, 8 -> 0, 9 -> 1, 4095 -> 255.  lo > hi inverts: t = 255 - level(v; hi, lo)
 * (MONOCHROME1).  lo == hi is refused.  For a centre c and width w use lo = c - w / 2,
 * hi = c + w / 2 with your own rounding: the engine takes the two ends as they are.
 * curve: NULL or 256 bytes, t = curve[t] (gamma, sigmoid: tables the caller builds).
 * GK_RENDER_WINDOW: C channels in, C out, out_k = t_k.
 * GK_RENDER_MAP: exactly one channel in, three out, out_c = map[3 t + c] (map: 768 bytes).
 * GK_RENDER_BLEND: 1..16 channels in, three out, out_c = min(255, floor((2 sum_k t_k tint_k,c +
 * 255) / 510)); a channel whose tint is (0, 0, 0) is left out.
 * While it is set sample_bytes must be 1, the header calls (gk_decode_header,
 * gk_header_components, gk_header_colour) and gk_view_result describe the output (C or 3
 * channels, precision 8, unsigned; sRGB under MAP / BLEND), and the planar calls gk_decode /
 * gk_decode_window refuse by name.  Refused here, each by name: a mode above 3; n of 0 or above
 * 16; no ch; lo == hi (the entry is named); MAP without a map; BLEND with every tint zero.  Refused
 * by the header, probe and decode calls, before anything is allocated or launched: MAP on a
 * channel count other than 1; BLEND whose channels' tints are all zero; more than 16 channels; a
 * sample_bytes other than 1. */
#define GK_RENDER_WINDOW 1u
#define GK_RENDER_MAP 2u
#define GK_RENDER_BLEND 3u
#define GK_RENDER_MAX_CHANNELS 16u
typedef struct gk_render_channel {
    int32_t lo, hi;
    uint8_t tint[3];           /* BLEND: r, g, b in 0..255 */
} gk_render_channel;
typedef struct gk_render {
    uint32_t mode;             /* 0: none */
    uint32_t n;                /* entries of ch, 1..16 */
    const gk_render_channel* ch;
    const uint8_t* curve;      /* NULL or 256 bytes */
    const uint8_t* map;        /* MAP: 256 x 3 bytes */
} gk_render;
int gk_set_decode_render(gk_ctx* ctx, const gk_render* r);
typedef struct gk_render_result {
    uint32_t channels, prec, sgnd;   /* of the rendered output: C or 3, 8, 0 */
    uint32_t colour_space;           /* GRK_COLOR_SPACE: sRGB (2) under MAP / BLEND, else the unrendered output's */
} gk_render_result;
/* What the pixel calls return for host bytes under these display flags, this precision list
 * (n = 0: none) and this render description (NULL or mode 0: none), no device needed: 0 and *res,
 * or -1 with the refusal in msg. */
int gk_probe_render(const uint8_t* cs, size_t len, uint32_t display_flags, const gk_precision* list, uint32_t n,
                    const gk_render* r, gk_render_result* res, char* msg, size_t msg_cap);

/* Where a view's values lie: the view is resolved and decoded exactly as gk_decode_view_pixels does
 * (same reduce level, same sticky settings; a sticky render is ignored here, so it can stay set
 * while the window is re-measured), no pixels are written, and per output channel k stats[k]
 * receives min, max, sum and count (= pix_w * pix_h) of exactly the int32 pixels the same view
 * returns.  bins > 0: hist[k * bins + b] counts the pixels with
 *   b = clamp(floor((v - origin_k) / 2^shift_k), 0, bins - 1),
 * channel k taking entry min(k, nq - 1) of q (nq = 0: origin 0, shift 0); values outside the binned
 * range fall into the end bins.  A 16-bit histogram at full resolution is two calls: min / max
 * first, then origin = min and the smallest shift that fits.  stats holds res->channels entries
 * (at most 16).  Refused by name, before anything is allocated or launched: bins above
 * GK_LEVELS_MAX_BINS; a shift above 31; bins > 0 without hist, or hist_cap below channels * bins;
 * everything gk_decode_view_pixels refuses. */
#define GK_LEVELS_MAX_BINS 4096u
typedef struct gk_levels_bins {
    int32_t origin;
    uint32_t shift;
} gk_levels_bins;
typedef struct gk_channel_levels {
    int32_t min, max;
    int64_t sum;
    uint64_t count;
} gk_channel_levels;
int gk_decode_levels(gk_ctx* ctx, const uint8_t* cs, size_t len, int cs_on_device, const gk_view* v,
                     const gk_levels_bins* q, uint32_t nq, uint32_t bins, gk_channel_levels* stats, uint64_t* hist,
                     size_t hist_cap, gk_view_result* res /* may be NULL */);

/* Decode a view to a float tensor: the view is resolved and decoded exactly as
 * gk_decode_view_pixels does, and its last pass (k_tensor, gk_tensor.hip) writes normalised
 * float32, float16 or bfloat16 elements in the caller's strides, planar (C, H, W), packed
 * (H, W, C), with padded rows, or as one image of a batch the caller owns.
 * The rule.  The input is the int32 sample v of channel k of written pixel (x, y), exactly as
 * gk_decode_view_pixels delivers it for the same gk_view with sample_bytes 0 and no render: after
 * layers, colour boxes, display flags, the precision list, the reduce level the view chooses, the
 * area average, mirror and rotation.  The output element is
 *   f = float32(v)          int32 -> float32, round to nearest even (exact for |v| <= 2^24)
 *   g = f * scale_k         one float32 multiplication, round to nearest even
 *   z = g + bias_k          one float32 addition, round to nearest even; never fused with the multiplication
 *   out = z                                     GK_TENSOR_F32
 *         float16(z), round to nearest even     GK_TENSOR_F16
 *         bfloat16(z), round to nearest even    GK_TENSOR_BF16
 * Channel k takes entry min(k, n - 1) of scale and bias; n = 0 means scale 1 and bias 0.  Overflow
 * gives an infinity, as IEEE says.  A result that is subnormal in the output type (or a subnormal
 * g or z on the way) follows the device's default float mode: nothing is promised about it.
 * The element is written at data + (k * stride_c + y * stride_y + x * stride_x) * es, es = 4, 2 or
 * 2 bytes, and no other byte is touched.
 * The layout.  The three dimensions are (channels, stride_c), (pix_h, stride_y) and (pix_w,
 * stride_x), strides in elements.  A dimension of size 1 is left out and its stride ignored.  The
 * rest are sorted by stride: the smallest must be >= 1 and each next one >= the previous stride
 * times the previous size, so no two elements share an address.  extent = 1 + sum((size_d - 1) *
 * stride_d) is the span in elements from data on.  A host tensor (on_device = 0) must also be
 * dense, extent == channels * pix_w * pix_h: it is written on the device in the same strides and
 * brought back by one copy of extent * es bytes.
 * Refused, each by name, before anything is allocated or launched, and changing no setting: no t or
 * no data; a dtype outside 1..3; n above 16; n > 0 without scale or without bias; a scale or bias
 * entry that is NaN or infinite (the entry is named); a render that is set (a rendered tensor is
 * out of scope: clear it); a zero or negative stride on a dimension of size above 1; overlapping
 * strides; a host tensor that is not dense; a device pointer not aligned to es; everything
 * gk_decode_view_pixels refuses of the view (and its one late refusal, a stream that holds only
 * some of its tiles, stays where that call makes it).  gk_get_timings afterwards: the decode's,
 * with the tensor pass added to mct_ms and total_ms as the view pass is.  *res: the view's. */
#define GK_TENSOR_F32 1u
#define GK_TENSOR_F16 2u
#define GK_TENSOR_BF16 3u
typedef struct gk_tensor {
    void* data;
    int32_t on_device;
    uint32_t dtype;
    int64_t stride_c, stride_y, stride_x;   /* in elements, of the written image (after rotation) */
    uint32_t n;                             /* entries of scale and bias, 0..16 */
    const float* scale;
    const float* bias;
} gk_tensor;
int gk_decode_view_tensor(gk_ctx* ctx, const uint8_t* cs, size_t len, int cs_on_device, const gk_view* v,
                          const gk_tensor* t, gk_view_result* res /* may be NULL */);
/* What gk_decode_view_tensor would say of this description for a resolved view (gk_probe_view's
 * result), no device needed and data never read (it may be NULL here; when it is not, a device
 * pointer's alignment is judged too): 0 and *extent in elements, or -1 with the refusal in msg.
 * The decode call runs the same check through the same function.  (The sticky render and reduce
 * are the decode's to judge.) */
int gk_probe_tensor(const gk_view_result* view, const gk_tensor* t, uint64_t* extent, char* msg, size_t msg_cap);

/* Inverse 5/3 rule of later gk_decode_window calls.  whole_tile = 0 (default): Grok's partial-tile
 * inverse, which a window set through setDecompressWindow selects for every tile
 * (CodeStreamDecompress.cpp:389; a one-sample-wide resolution on an odd coordinate shifts its
 * sample, WaveletReverse.cpp:1551-1554).  whole_tile = 1: the whole-tile rule (that sample halved,
 * WaveletReverse.cpp:583), which CodeStreamDecompress::decompressTile keeps when no window is set
 * (grk_decompress_tile with the CLI's set_window(0,0,0,0), :309-316, 416-493). */
int gk_set_window_rule(gk_ctx* ctx, int whole_tile);

/* grk_decompress_set_window + grk_decompress (grok.h:1082-1657; CodeStreamDecompress
 * window decode): decode the window [x0, x1) x [y0, y1) of the image.
 * Only the tile parts of tiles intersecting the window are read (located through TLM
 * when present, their packet headers through PLT), decoded and inverse-transformed;
 * comps[c][0] receives sample (x0, y0) of component c, row stride strides[c] (with
 * gk_set_decode_reduce: the reduced window's first sample, see there). */
int gk_decode_window(gk_ctx* ctx, const uint8_t* cs, size_t len, int cs_on_device, uint32_t x0, uint32_t y0,
                     uint32_t x1, uint32_t y1, void* const* comps, const uint32_t* strides, uint32_t sample_bytes,
                     int out_on_device);

/* Code-block results of a single-tile encode, for Grok's T1 plugin interface (SURVEY.md
 * §8(b) B2: grk_plugin_tile -> ... -> grk_plugin_code_block, grok.h:995-1077): what the host
 * takes from the plugin in compress_synch_with_plugin (plugin/plugin_bridge.cpp:146-270).
 * Order is canonical: component, resolution, band, precinct, code-block
 * (T1CompressScheduler.cpp:31-94). */
typedef struct gk_band_result {
    uint32_t comp, res, band;   /* position in the tile tree */
    uint32_t orient;            /* 0 LL, 1 HL, 2 LH, 3 HH (grk_plugin_band::orientation) */
    uint32_t num_precincts;     /* grk_plugin_band::numPrecincts (precinct grid of the resolution) */
    float stepsize;             /* the band's quantisation step (Subband::stepsize) */
} gk_band_result;
typedef struct gk_block_result {
    uint32_t comp, res, band, precinct, cblk;   /* position; cblk = raster index in the precinct */
    uint32_t x0, y0, x1, y1;                    /* code-block rectangle in band coordinates */
    uint32_t numbps;                            /* Codeblock::numbps */
    uint32_t npasses;                           /* CompressCodeblock::numPassesTotal */
    uint32_t len;                               /* compressed bytes */
    uint32_t pass_off;                          /* first pass record in the pass array */
    uint64_t data_off;                          /* first byte in the byte array */
} gk_block_result;
typedef struct gk_pass_result {
    uint32_t rate;     /* cumulative bytes after the pass (CodePass::rate, T1.cpp:856-930 rules) */
    uint32_t len;      /* rate - previous rate (CodePass::len) */
    double dist;       /* cumulative distortion decrease (CodePass::distortiondec); 0 unless the
                          parameters ask for rate control (TileProcessor::needsRateControl) */
} gk_pass_result;

/* TileProcessor::doCompress up to and including T1 (TileProcessor.cpp:202-232: DC shift, MCT,
 * DWT, t1_encode) of a single-tile image; the results stay in the context and *nbands,
 * *nblocks, *nbytes, *npasses receive their counts.  Returns 0 / < 0 (error). */
int gk_encode_blocks(gk_ctx* ctx, const gk_image_info* info, const void* const* comps, const uint32_t* strides,
                     int comps_on_device, const gk_cparameters* p, uint32_t* nbands, uint32_t* nblocks,
                     uint64_t* nbytes, uint32_t* npasses);
/* Copies the results of the last gk_encode_blocks into caller arrays of the reported sizes
 * (any pointer may be NULL to skip that array). */
int gk_encode_blocks_get(gk_ctx* ctx, gk_band_result* bands, gk_block_result* blocks, uint8_t* data,
                         gk_pass_result* passes);

/* Transcode between the two block coders, Part-1 (EBCOT / MQ) and HTJ2K, without touching a
 * coefficient: the source coder's T1 decoders leave signed quantisation indices in the work
 * planes and the target coder's T1 encoders read them there.  No DWT, MCT or sample stage runs,
 * so a 9/7 stream takes no second lossy generation.  (Grok 9.2.0 has no counterpart: its
 * CodeStreamTranscode / FileFormatTranscode classes are empty.)
 * cs: a raw codestream or a JP2 file (device memory if cs_on_device).  Of a JP2 file every box
 * outside jp2c is copied byte for byte and jp2c gets the new codestream and its length (the XL
 * form stays).  The new codestream keeps SIZ, the COD's levels, code-block size, precincts,
 * progression order, MCT flag and transform, QCD / QCC verbatim, RGN and (com) the COM markers.
 * It changes the code-block style (0x40 for HT, 0 for Part-1), Rsiz bit 14 and the CAP marker
 * (MAGBp from the largest band bit-plane count, ROI shift included; for a 9/7 stream the count
 * the engine's HT encoder writes for those bands); it has one layer, one tile
 * part per tile, no SOP / EPH, packet headers in the packets (PPM / PPT unpacked) and TLM / PLT as
 * the params say.  Blocks the Part-1 coder finds all zero are written as not included; the HT
 * coder writes every block, as on encode.
 * Refused, each by name and before any kernel runs (gk_probe_transcode gives the same answer on
 * the host): a truncated code-block of a Part-1 source (an included block with fewer than
 * 3 * numbps - 2 passes: streams cut by rate control or quality layers); an HT block with
 * SigProp / MagRef passes; a band of more bit-planes than the target coder holds (HT 30, Part-1
 * 26, Part-1 with a code-block side above 64: 25); POC; a COC, or a tile-part COD / COC / QCD /
 * QCC / RGN, that changes a component's or tile's coding; Part-2 markers; a source already in the
 * target coder; a non-zero gk_set_decode_layers or gk_set_decode_reduce (display, precision and
 * colour settings are output settings and are ignored).
 * gk_transcode returns 0, -2 with *out_len = the size needed, or -1 (gk_last_error).  Afterwards
 * gk_get_timings has t1_cm_ms = the source coder's decode kernels, t1_coder_ms = the target
 * coder's encode kernels, t1_ms their sum, t2_ms the packet parse and write, and 0 in the DWT and
 * MCT fields. */
#define GK_TRANSCODE_HT 1u
#define GK_TRANSCODE_PART1 2u
typedef struct gk_transcode_params {
    uint32_t target;          /* GK_TRANSCODE_HT | GK_TRANSCODE_PART1 */
    uint32_t tlm, plt, com;   /* write TLM / PLT markers (as gk_cparameters), keep the source's COM markers */
} gk_transcode_params;
/* target HT, no TLM / PLT (Grok's defaults), COM kept */
void gk_set_default_transcode(gk_transcode_params* p);
int gk_transcode(gk_ctx* ctx, const uint8_t* cs, size_t len, int cs_on_device, const gk_transcode_params* p,
                 uint8_t* out, size_t cap, int out_on_device, size_t* out_len);
/* 0 if the host bytes would transcode, -1 with the refusal in msg.  Needs no device: it parses
 * the headers and every packet header on the host. */
int gk_probe_transcode(const uint8_t* cs, size_t len, const gk_transcode_params* p, char* msg, size_t msg_cap);

/* Stage timings of the last gk_encode / gk_decode / gk_transcode. */
int gk_get_timings(gk_ctx* ctx, gk_timings* t);
/* Last error message for this context (grk_set_error_handler equivalent). */
const char* gk_last_error(gk_ctx* ctx);
/* Engine version string (grk_version, grok.cpp). */
const char* gk_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GROK_AMD_H */
