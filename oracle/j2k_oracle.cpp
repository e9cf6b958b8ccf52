// =============================================================================
// j2k_oracle.cpp — CPU restatement of Grok 9.2.0's JPEG 2000 tile pipeline.
//
// TEST INFRASTRUCTURE ONLY.  This file is the parity oracle for the MI355X
// hot path in grok_amd/.  Only tests/, __graft_entry__.smoke() and bench.py's
// cpu_baseline leg may load it, and only as the checker (or the timed CPU
// baseline) — never as the product.  The product library (grok_amd/csrc) does
// not include, link or call anything in this directory.
//
// Parity pin: the outputs of this restatement are checked byte-for-byte
// against codestreams produced by reference Grok 9.2.0 (the binaries the survey
// stage built with cmake; fixtures made by
// tests/golden/make_fixtures.py and make_fullsize.py).  The JP2
// box wrapper (FileFormatCompress.cpp) is restated but not pinned by a Grok
// output: Grok needs cmake-generated headers, so it is not rebuilt here.
//
// Restated from the reference sources with no Grok-produced fixture, so PARITY UNPINNED
// for them (the engine is tested byte-/sample-exact against these restatements): code-block
// mode switches (T1.cpp, mqc_enc.cpp, T2 segments), progression orders other than LRCP and
// POC (PacketIter.cpp), HT with 9/7 (the standard-correct fix of R-BUG-2), layer-limited and
// reduced-resolution decode, tiles in several tile parts and tile-part generation.
//
// Threads (orc_set_threads): code-blocks of a tile, and tiles of a multi-tile
// image, are coded on worker threads; the result does not depend on the count.
//
// Every stage cites the reference function it restates (paths relative to
// /root/reference/src/lib/jp2/).  The code is written from the JPEG 2000
// Part-1 standard (ISO 15444-1 Annexes B, C, D, E, F, G) plus the Grok-specific
// conventions the survey identified (pass termination, rate rules, FF back-off,
// marker layout), not translated from the reference sources.
// =============================================================================
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <memory>
#include <algorithm>
#include <atomic>
#include <functional>
#include <map>
#include <tuple>
#include <thread>

namespace orc {

// ----------------------------------------------------------------------------
// Worker threads: par_for(n, f) runs f(0..n-1) on up to g_threads threads
// (nested calls run serially on the calling thread).
// ----------------------------------------------------------------------------
static unsigned g_threads = 1;
static uint32_t g_dec_layers = 0;   // decode: quality layers to use (0 = all; grk_dparameters::cp_layer)
static uint32_t g_dec_reduce = 0;   // decode: resolutions discarded (grk_dparameters::cp_reduce)
static thread_local bool t_in_par = false;
template <class F> static void par_for(size_t n, F f) {
    const unsigned T = (unsigned)std::min<size_t>(g_threads, n);
    if (T <= 1 || t_in_par) { for (size_t i = 0; i < n; ++i) f(i); return; }
    std::atomic<size_t> next{0};
    auto work = [&] {
        t_in_par = true;
        for (;;) { const size_t i = next++; if (i >= n) break; f(i); }
        t_in_par = false;
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < T; ++t) th.emplace_back(work);
    work();
    for (auto& x : th) x.join();
}

static inline uint32_t ceildivpow2(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a + (1ull << b) - 1) >> b); }
static inline uint32_t floordivpow2(uint32_t a, uint32_t b) { return a >> b; }
static inline uint32_t ceildiv(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a + b - 1) / b); }
static inline int floorlog2(uint32_t a) { int l = 0; while (a > 1) { a >>= 1; ++l; } return l; }

// ----------------------------------------------------------------------------
// Coding parameters (subset of grk_cparameters, grok.h:466-590)
// ----------------------------------------------------------------------------
struct PocE { uint32_t rs, cs, lye, re, ce, prog; };   // progression order change (POC marker, A.6.6)

struct Params {
    uint32_t numres = 6;        // grok.cpp:405-435 default: 6 resolutions
    uint32_t cbw_exp = 6, cbh_exp = 6;  // 64x64
    uint32_t irreversible = 0;  // qmfbid: 1 = 5/3, 0 = 9/7
    uint32_t mct = 1;
    uint32_t numgbits = 2;
    uint32_t prcw_exp[33], prch_exp[33];  // per resolution
    uint32_t nlayers = 1;
    double rates[100] = {0};    // grk_cparameters::layer_rate (compression ratios; 0 = all remaining passes)
    int write_com = 1;
    uint32_t cblk_sty = 0;      // mode switches (grok.h:98-103) or 0x40 = HTJ2K block coder (GRK_CBLKSTY_HT, grok.h:104)
    uint32_t prog = 0;          // progression order (GRK_PROG_ORDER): LRCP 0, RLCP 1, RPCL 2, PCRL 3, CPRL 4
    char tp_div = 0;            // tile-part divider 'L' / 'R' / 'C' (grk_compress -u), 0 = one part per tile
    std::vector<PocE> pocs;     // progression order changes (encode: every tile; decode: main header)
    std::vector<uint32_t> roishift;   // per component ROI maxshift (RGN); empty = none
    uint32_t roi(uint32_t c) const { return c < roishift.size() ? roishift[c] : 0u; }
    uint32_t tw = 0, th = 0;    // nominal tile size (0 = one tile covering the image), grk_cparameters::t_width/t_height
    // canvas offsets (B.2, B.3): the image area starts at (x0, y0) (grk_image::x0 / y0, CLI -d), the
    // tile grid at (gx0, gy0) <= (x0, y0) (grk_cparameters::tx0 / ty0, CLI -T); w x h is the image area
    uint32_t x0 = 0, y0 = 0, gx0 = 0, gy0 = 0;
    int tlm = 0, plt = 0;       // write TLM (-X) / PLT (-L) markers
    uint32_t sop_eph = 0;       // Scod bits: 2 = SOP before every packet, 4 = EPH after every packet header (-S / -E)
    bool quality = false;       // fixed-quality layers (-q, grk_cparameters::allocationByQuality)
    double dist[100] = {0};     // per-layer PSNR targets (layer_distortion; 0 = every remaining pass)
    bool ht() const { return (cblk_sty & 0x40) != 0; }
    // per-component quantisation of third-party encoders (written as QCC markers, A.6.5; Grok's own
    // encoder pushes one QCD to every component, CodeStreamCompress.cpp:382-384): guard bits per
    // component (empty: numgbits), irreversible exponents lowered by qshift[c] (a step 2^qshift
    // times coarser), and scalar-derived quantisation (Sqcd style 1: only the LL step is written,
    // the others follow E-5 as Quantizer.cpp:319-331 expands them)
    std::vector<uint32_t> comp_gb;
    std::vector<int32_t> comp_qshift;
    bool qderived = false;
    uint32_t gb(uint32_t c) const { return c < comp_gb.size() ? comp_gb[c] : numgbits; }
    // component subsampling (SIZ XRsiz / YRsiz, grk_image_comp::dx / dy; empty = 1): component c
    // samples the canvas at multiples of (sx(c), sy(c)), its tile-components are the tiles'
    // rectangles divided by them, rounded up (TileProcessor.cpp:116-131)
    std::vector<uint32_t> cdx, cdy;
    // packed packet headers (A.7.4 / A.7.5): 1 = PPT (each tile's headers in its tile-part
    // header), 2 = PPM (every tile's in the main header); the packets then carry their bodies only.
    // Grok's encoder writes neither; they are third-party streams its decoder reads
    // (CodeStreamDecompress read_ppm / read_ppt, T2Decompress.cpp:255-270)
    uint32_t ppx = 0;
    // caller COM markers (grk_compress -C; CodeStreamCompress.cpp:303-330, write_com :1114-1145):
    // (Rcom, bytes), written instead of the default comment
    std::vector<std::pair<uint32_t, std::string>> comments;
    uint32_t sx(uint32_t c) const { return c < cdx.size() ? cdx[c] : 1u; }
    uint32_t sy(uint32_t c) const { return c < cdy.size() ? cdy[c] : 1u; }
    bool subsampled() const {
        for (uint32_t v : cdx) if (v != 1) return true;
        for (uint32_t v : cdy) if (v != 1) return true;
        return false;
    }
    int32_t qshift(uint32_t c) const { return c < comp_qshift.size() ? comp_qshift[c] : 0; }
    Params() { for (int i = 0; i < 33; ++i) { prcw_exp[i] = 15; prch_exp[i] = 15; } }
};

// A component's quantisation as decoded from QCD / QCC (A.6.4-A.6.5): guard bits and the (expn,
// mant) of every band, LL first then (HL, LH, HH) per resolution, scalar-derived steps expanded
struct Quant { uint32_t gb = 2; std::vector<std::pair<uint32_t, uint32_t>> steps; };

// ----------------------------------------------------------------------------
// Tile geometry (Annex B; Grok: Resolution.h:37-72, Precinct.h:59-68,
// TileComponentWindowBuffer.h:180-222 for the Mallat placement)
// ----------------------------------------------------------------------------
struct PassInfo { uint32_t rate; uint32_t len; int term; double dist; };

struct Cblk {
    uint32_t x0, y0, x1, y1;      // band coordinates
    uint32_t numbps = 0;          // encoder: bit planes; decoder: from zero-bitplane tag tree
    uint32_t npasses = 0;         // total passes (encoder) / decoded passes (decoder)
    std::vector<uint8_t> data;
    std::vector<PassInfo> passes;
    // T2 state
    uint32_t numlenbits = 0;
    uint32_t passes_in_prev = 0;  // passes included in previous layers (encoder)
    std::vector<uint32_t> layer_np; // encoder: passes contributed to each layer (rate allocation)
    bool included_before = false;
    std::vector<uint32_t> seglens; // decoder: per segment lengths (one segment in default mode)
    std::vector<uint32_t> segpasses;
};

struct Precinct {
    uint32_t x0, y0, x1, y1;     // band coords
    uint32_t cw = 0, ch = 0;     // code-block grid dims
    std::vector<Cblk> cblks;
};

struct Band {
    uint32_t orient;             // 0 LL, 1 HL, 2 LH, 3 HH
    uint32_t x0, y0, x1, y1;     // band coords
    uint32_t offx, offy;         // Mallat placement in the component buffer
    uint32_t numbps;             // Quantizer.cpp:45-49 : expn + guard - 1
    uint32_t expn, mant;
    float stepsize;              // Quantizer.cpp:40-42 (compress semantics)
    std::vector<Precinct> prcs;  // same count for every band of a resolution
    bool empty() const { return x1 <= x0 || y1 <= y0; }
};

struct Res {
    uint32_t x0, y0, x1, y1;
    uint32_t pw = 0, ph = 0;     // precinct grid
    uint32_t prcw_exp, prch_exp, cbw_exp, cbh_exp;
    std::vector<Band> bands;
};

struct Comp {
    uint32_t w, h;               // tile-component size (origin 0)
    std::vector<Res> res;
};

// Tile-component (tx0,ty0)-(tx1,ty1) in reference-grid coordinates (B.5).  The
// sample buffer is tile-local (c.w x c.h); the band, precinct and code-block
// grids are absolute, as in Grok's Resolution/Precinct setup.
static void build_geometry(Comp& c, uint32_t tx0, uint32_t ty0, uint32_t tx1, uint32_t ty1, const Params& p) {
    c.w = tx1 - tx0; c.h = ty1 - ty0;
    c.res.assign(p.numres, Res());
    for (uint32_t r = 0; r < p.numres; ++r) {
        Res& R = c.res[r];
        uint32_t nb = p.numres - 1 - r;
        R.x0 = ceildivpow2(tx0, nb); R.y0 = ceildivpow2(ty0, nb);
        R.x1 = ceildivpow2(tx1, nb); R.y1 = ceildivpow2(ty1, nb);
        R.prcw_exp = p.prcw_exp[r]; R.prch_exp = p.prch_exp[r];
        uint32_t px0 = floordivpow2(R.x0, R.prcw_exp) << R.prcw_exp;
        uint32_t py0 = floordivpow2(R.y0, R.prch_exp) << R.prch_exp;
        uint32_t px1 = ceildivpow2(R.x1, R.prcw_exp) << R.prcw_exp;
        uint32_t py1 = ceildivpow2(R.y1, R.prch_exp) << R.prch_exp;
        R.pw = (R.x1 > R.x0) ? ((px1 - px0) >> R.prcw_exp) : 0;
        R.ph = (R.y1 > R.y0) ? ((py1 - py0) >> R.prch_exp) : 0;
        uint32_t bprcw, bprch;
        if (r == 0) { bprcw = R.prcw_exp; bprch = R.prch_exp; }
        else { bprcw = R.prcw_exp - 1; bprch = R.prch_exp - 1; }
        R.cbw_exp = std::min(p.cbw_exp, bprcw);
        R.cbh_exp = std::min(p.cbh_exp, bprch);
        uint32_t nbands = (r == 0) ? 1 : 3;
        R.bands.assign(nbands, Band());
        for (uint32_t bi = 0; bi < nbands; ++bi) {
            Band& B = R.bands[bi];
            B.orient = (r == 0) ? 0 : bi + 1;
            if (r == 0) {
                B.x0 = R.x0; B.y0 = R.y0; B.x1 = R.x1; B.y1 = R.y1;
                B.offx = 0; B.offy = 0;
            } else {
                uint32_t nbb = p.numres - r;  // decomposition level of this band
                uint32_t xo = (B.orient & 1), yo = (B.orient >> 1);
                // tbx0 = ceil((tcx0 - 2^(nbb-1) xo) / 2^nbb) with tcx0 = 0
                uint64_t half = 1ull << (nbb - 1);
                auto cb = [&](uint64_t t, uint32_t o) -> uint32_t {
                    if (o == 0) return ceildivpow2((uint32_t)t, nbb);
                    if (t <= half) return 0;
                    return ceildivpow2((uint32_t)(t - half), nbb);
                };
                B.x0 = cb(tx0, xo); B.y0 = cb(ty0, yo);
                B.x1 = cb(tx1, xo); B.y1 = cb(ty1, yo);
                const Res& L = c.res[r - 1];
                B.offx = xo ? (L.x1 - L.x0) : 0;
                B.offy = yo ? (L.y1 - L.y0) : 0;
            }
            // precincts of this band (B.6)
            uint32_t nprc = R.pw * R.ph;
            B.prcs.assign(nprc, Precinct());
            uint32_t tlx = (r == 0) ? px0 : (px0 >> 1);
            uint32_t tly = (r == 0) ? py0 : (py0 >> 1);
            for (uint32_t pi = 0; pi < nprc; ++pi) {
                Precinct& P = B.prcs[pi];
                uint32_t i = pi % R.pw, j = pi / R.pw;
                uint32_t cx0 = tlx + (i << bprcw), cy0 = tly + (j << bprch);
                uint32_t cx1 = cx0 + (1u << bprcw), cy1 = cy0 + (1u << bprch);
                P.x0 = std::max(cx0, B.x0); P.y0 = std::max(cy0, B.y0);
                P.x1 = std::min(cx1, B.x1); P.y1 = std::min(cy1, B.y1);
                if (B.empty() || P.x1 <= P.x0 || P.y1 <= P.y0) { P.cw = P.ch = 0; continue; }
                uint32_t gx0 = floordivpow2(P.x0, R.cbw_exp) << R.cbw_exp;
                uint32_t gy0 = floordivpow2(P.y0, R.cbh_exp) << R.cbh_exp;
                uint32_t gx1 = ceildivpow2(P.x1, R.cbw_exp) << R.cbw_exp;
                uint32_t gy1 = ceildivpow2(P.y1, R.cbh_exp) << R.cbh_exp;
                P.cw = (gx1 - gx0) >> R.cbw_exp; P.ch = (gy1 - gy0) >> R.cbh_exp;
                P.cblks.assign(P.cw * P.ch, Cblk());
                for (uint32_t k = 0; k < P.cw * P.ch; ++k) {
                    Cblk& K = P.cblks[k];
                    uint32_t a = k % P.cw, b = k / P.cw;
                    uint32_t kx0 = gx0 + (a << R.cbw_exp), ky0 = gy0 + (b << R.cbh_exp);
                    K.x0 = std::max(kx0, P.x0); K.y0 = std::max(ky0, P.y0);
                    K.x1 = std::min(kx0 + (1u << R.cbw_exp), P.x1);
                    K.y1 = std::min(ky0 + (1u << R.cbh_exp), P.y1);
                }
            }
        }
    }
}

// ----------------------------------------------------------------------------
// Step sizes (HTParams.cpp:194-252 param_qcd::generate, Part-1 branch;
// Quantizer.cpp:26-66 setBandStepSizeAndBps)
// ----------------------------------------------------------------------------
static const double dwt_norms_53[4][10] = {
    {1.000, 1.500, 2.750, 5.375, 10.68, 21.34, 42.67, 85.33, 170.7, 341.3},
    {1.038, 1.592, 2.919, 5.703, 11.33, 22.64, 45.25, 90.48, 180.9},
    {1.038, 1.592, 2.919, 5.703, 11.33, 22.64, 45.25, 90.48, 180.9},
    {.7186, .9218, 1.586, 3.043, 6.019, 12.01, 24.00, 47.97, 95.93}};
static const double dwt_norms_97[4][10] = {
    {1.000, 1.965, 4.177, 8.403, 16.90, 33.84, 67.69, 135.3, 270.6, 540.9},
    {2.022, 3.989, 8.355, 17.04, 34.27, 68.63, 137.3, 274.6, 549.0},
    {2.022, 3.989, 8.355, 17.04, 34.27, 68.63, 137.3, 274.6, 549.0},
    {2.080, 3.865, 8.307, 17.18, 34.71, 69.59, 139.3, 278.6, 557.2}};
static double getnorm(uint32_t level, uint32_t orient, bool rev) {  // T1.cpp:264-277
    if (orient == 0 && level > 9) level = 9;
    else if (orient > 0 && level > 8) level = 8;
    return rev ? dwt_norms_53[orient][level] : dwt_norms_97[orient][level];
}

// BIBO gains of the 5/3 synthesis (HTParams.cpp:134-145), used by the HT
// reversible QCD.
static const float bibo53_l[16] = {1.0000f, 1.5000f, 1.6250f, 1.6875f, 1.6963f, 1.7067f, 1.7116f, 1.7129f,
                                   1.7141f, 1.7145f, 1.7151f, 1.7152f, 1.7155f, 1.7155f, 1.7156f, 1.7156f};
static const float bibo53_h[16] = {2.0000f, 2.5000f, 2.7500f, 2.8047f, 2.8198f, 2.8410f, 2.8558f, 2.8601f,
                                   2.8628f, 2.8656f, 2.8662f, 2.8667f, 2.8669f, 2.8670f, 2.8671f, 2.8671f};
static uint32_t ht_rev_expn(uint32_t B, uint32_t ndecomp, uint32_t r, uint32_t orient) {
    auto L = [](uint32_t i) { return bibo53_l[std::min(i, 15u)]; };
    auto H = [](uint32_t i) { return bibo53_h[std::min(i, 15u)]; };
    auto X = [](float g) { return (int)ceil(log(g * 1.1f) / 0.69314718055994530942); };
    if (r == 0) return (uint32_t)((int)B + X(L(ndecomp) * L(ndecomp)));
    uint32_t d = ndecomp - r;   // OpenJPH level index of this resolution's bands
    if (orient == 3) return (uint32_t)((int)B + X(H(d) * H(d)));
    return (uint32_t)((int)B + X(H(d) * L(d + 1)));
}

// HT irreversible QCD: param_qcd::set_irrev_quant (HTParams.cpp:273-317) with base_delta =
// 2^-(bit depth + signed) (:211-212) and the 9/7 synthesis energy gains (sqrt_energy_gains,
// HTParams.cpp:75-86; constant data of the 9/7 filter bank).
static const float HT_G97_L[34] = {
    1.0000e+00f, 1.4021e+00f, 2.0304e+00f, 2.9012e+00f, 4.1153e+00f, 5.8245e+00f, 8.2388e+00f, 1.1652e+01f, 1.6479e+01f,
    2.3304e+01f, 3.2957e+01f, 4.6609e+01f, 6.5915e+01f, 9.3217e+01f, 1.3183e+02f, 1.8643e+02f, 2.6366e+02f, 3.7287e+02f,
    5.2732e+02f, 7.4574e+02f, 1.0546e+03f, 1.4915e+03f, 2.1093e+03f, 2.9830e+03f, 4.2185e+03f, 5.9659e+03f, 8.4371e+03f,
    1.1932e+04f, 1.6874e+04f, 2.3864e+04f, 3.3748e+04f, 4.7727e+04f, 6.7496e+04f, 9.5454e+04f};
static const float HT_G97_H[34] = {
    1.4425e+00f, 1.9669e+00f, 2.8839e+00f, 4.1475e+00f, 5.8946e+00f, 8.3472e+00f, 1.1809e+01f, 1.6701e+01f, 2.3620e+01f,
    3.3403e+01f, 4.7240e+01f, 6.6807e+01f, 9.4479e+01f, 1.3361e+02f, 1.8896e+02f, 2.6723e+02f, 3.7792e+02f, 5.3446e+02f,
    7.5583e+02f, 1.0689e+03f, 1.5117e+03f, 2.1378e+03f, 3.0233e+03f, 4.2756e+03f, 6.0467e+03f, 8.5513e+03f, 1.2093e+04f,
    1.7103e+04f, 2.4187e+04f, 3.4205e+04f, 4.8373e+04f, 6.8410e+04f, 9.6747e+04f, 1.3682e+05f};
static void ht_irrev_quant(uint32_t prec, int sgnd, uint32_t nd, uint32_t r, uint32_t orient, uint32_t& expn, uint32_t& mant) {
    const float base_delta = 1.0f / (float)(1u << (prec + (sgnd ? 1 : 0)));
    float gl, gh;
    if (r == 0) { gl = HT_G97_L[nd]; gh = gl; }
    else {
        const uint32_t d = nd - r;
        gl = orient == 3 ? HT_G97_H[d] : HT_G97_L[d + 1];
        gh = HT_G97_H[d];
    }
    float delta_b = base_delta / (gl * gh);
    uint32_t e = 0;
    while (delta_b < 1.0f) { e++; delta_b *= 2.0f; }
    uint32_t m = (uint32_t)round(delta_b * (float)(1 << 11)) - (1 << 11);
    mant = m < (1u << 11) ? m : 0x7ff;
    expn = e;
}

// Expand a QCD / QCC body's steps (Sqcd, then SPqcd) into a Quant for numres resolutions:
// scalar derived (style 1) as Grok's read_SQcd_SQcc (Quantizer.cpp:319-331), band b > 0 taking
// expn_0 - floor((b - 1) / 3) (E-5: epsilon_0 - N_L + n_b) and mant_0.  false: malformed.
static bool parse_quant(const uint8_t* s, size_t n, uint32_t numres, Quant& q) {
    if (n < 1) return false;
    const uint32_t sq = s[0], qt = sq & 0x1f, nb = 3 * numres - 2;
    q.gb = sq >> 5;
    q.steps.clear();
    if (qt == 0) for (size_t k = 1; k < n; ++k) q.steps.push_back({(uint32_t)s[k] >> 3, 0u});
    else if (qt == 1 || qt == 2) for (size_t k = 1; k + 1 < n; k += 2) { uint32_t v = ((uint32_t)s[k] << 8) | s[k + 1]; q.steps.push_back({v >> 11, v & 0x7ff}); }
    else return false;
    if (q.steps.empty()) return false;
    if (qt == 1) {
        const auto s0 = q.steps[0];
        q.steps.assign(nb, s0);
        for (uint32_t b = 1; b < nb; ++b) q.steps[b] = {s0.first > (b - 1) / 3 ? s0.first - (b - 1) / 3 : 0u, s0.second};
    }
    return true;
}

static void assign_steps(Comp& c, const Params& p, uint32_t prec, bool compress, const Quant* qd, int sgnd = 0,
                         uint32_t roishift = 0, uint32_t comp = 0) {
    // qd (decoding): the component's guard bits and band steps, band order LL, (HL,LH,HH) per
    // resolution; encoding: p's guard bits, exponent shift and derived style of component comp
    uint32_t bandno = 0;
    const uint32_t gbits = qd ? qd->gb : p.gb(comp);
    uint32_t e0 = 0, m0 = 0;   // the LL step (scalar derived)
    for (uint32_t r = 0; r < p.numres; ++r) {
        for (auto& B : c.res[r].bands) {
            uint32_t expn, mant;
            if (qd) {
                expn = qd->steps[std::min<size_t>(bandno, qd->steps.size() - 1)].first;
                mant = qd->steps[std::min<size_t>(bandno, qd->steps.size() - 1)].second;
            } else if (p.ht() && p.irreversible) {
                ht_irrev_quant(prec, sgnd, p.numres - 1, r, B.orient, expn, mant);
            } else if (p.ht() && !p.irreversible) {
                // param_qcd::set_rev_quant (HTParams.cpp:253-272): B + ceil(log2(bibo^2 * 1.1)).
                // Grok passes tcp->mct before it is assigned (CodeStreamCompress.cpp:382 vs the
                // later mct setup), so the RCT bit is never added: B = precision.
                expn = ht_rev_expn(prec, p.numres - 1, r, B.orient);
                mant = 0;
            } else {
                uint32_t level = p.numres - 1 - r;
                uint32_t gain = p.irreversible ? 0 : (B.orient == 0 ? 0 : (B.orient == 3 ? 2 : 1));
                double stepsize = p.irreversible ? (double)(1u << gain) / getnorm(level, B.orient, false) : 1.0;
                uint32_t step = (uint32_t)floor(stepsize * 8192.0);
                int pp = floorlog2(step) - 13;
                int n = 11 - floorlog2(step);
                mant = (n < 0 ? step >> -n : step << n) & 0x7ff;
                expn = (uint32_t)std::max(0, (int)(prec + gain) - pp - (p.irreversible ? p.qshift(comp) : 0));
                if (p.irreversible && p.qderived) {   // E-5 from the LL step
                    if (bandno == 0) { e0 = expn; m0 = mant; }
                    else { expn = e0 > (bandno - 1) / 3 ? e0 - (bandno - 1) / 3 : 0u; mant = m0; }
                }
            }
            B.expn = expn; B.mant = mant;
            uint32_t log2_gain = (!compress && p.irreversible) ? 0 : (B.orient == 0 ? 0 : (B.orient == 3 ? 2 : 1));
            uint32_t nbps = prec + log2_gain;
            B.stepsize = (float)((1.0 + mant / 2048.0) * pow(2.0, (int)nbps - (int)expn));
            int v = (int)expn + (int)gbits - 1;
            B.numbps = roishift + (uint32_t)std::max(0, v);   // Quantizer.cpp:47: roishift + expn + guard - 1
            ++bandno;
        }
    }
}

// ----------------------------------------------------------------------------
// DC level shift + RCT  (TileProcessor.cpp:506-535, mct.cpp:99-146 / 221-283)
// ----------------------------------------------------------------------------
static void dc_rct_fwd(std::vector<std::vector<int32_t>>& planes, uint32_t prec, bool sgnd, bool mct) {
    int32_t shift = sgnd ? 0 : (1 << (prec - 1));
    for (auto& pl : planes) for (auto& v : pl) v -= shift;
    if (mct && planes.size() >= 3) {
        size_t n = planes[0].size();
        for (size_t i = 0; i < n; ++i) {
            int32_t r = planes[0][i], g = planes[1][i], b = planes[2][i];
            planes[0][i] = (r + 2 * g + b) >> 2;
            planes[1][i] = b - g;
            planes[2][i] = r - g;
        }
    }
}

// ICT (mct.cpp:147-219 CompressIrrev): y = a_r r + a_g g + a_b b, u = cb (b - y),
// v = cr (r - y) in float, evaluated left to right without contraction.
static void dc_ict_fwd(std::vector<std::vector<float>>& f, const std::vector<std::vector<int32_t>>& planes,
                       uint32_t prec, bool sgnd, bool mct) {
    int32_t shift = sgnd ? 0 : (1 << (prec - 1));
    f.assign(planes.size(), {});
    for (size_t c = 0; c < planes.size(); ++c) {
        f[c].resize(planes[c].size());
        for (size_t i = 0; i < planes[c].size(); ++i) f[c][i] = (float)(planes[c][i] - shift);
    }
    if (mct && planes.size() >= 3) {
        const float a_r = 0.299f, a_g = 0.587f, a_b = 0.114f;
        const float cb = 0.5f / (1.0f - a_b), cr = 0.5f / (1.0f - a_r);
        size_t n = f[0].size();
        for (size_t i = 0; i < n; ++i) {
            float r = f[0][i], g = f[1][i], b = f[2][i];
            float t0 = a_r * r, t1 = a_g * g, t2 = a_b * b;
            float y = (t0 + t1) + t2;
            float u = cb * (b - y);
            float v = cr * (r - y);
            f[0][i] = y; f[1][i] = u; f[2][i] = v;
        }
    }
}

// ----------------------------------------------------------------------------
// 5/3 reversible DWT (Annex F.3/F.4; Grok WaveletFwd.cpp:635-960 vertical
// first then horizontal, in-place Mallat deinterleave).  Parity 0 only
// (tile origin even at every level, which holds for single-tile images).
// ----------------------------------------------------------------------------
// A resolution whose first sample sits on an odd coordinate (tile origins off the 2^L grid,
// e.g. -t 200,160) starts with a high-pass sample: WaveletFwd.cpp's parity_row / parity_col
// (:486-489) select the odd ("cas1") lifting, and WaveletReverse.cpp:559-663 its inverse.
// Written once for both parities: sample i is high-pass when (i + parity) is odd, with
// whole-sample symmetric extension at both ends of the line; lows then highs on output.
static inline int64_t mirror(int64_t i, uint32_t n) {
    if (i < 0) i = -i;
    if (i >= (int64_t)n) i = 2 * (int64_t)n - 2 - i;
    return i;
}
static void fwd53_1d(int32_t* x, uint32_t n, std::vector<int32_t>& tmp, uint32_t par, bool) {
    if (n == 1) { if (par) x[0] *= 2; return; }   // odd single sample: 2x (WaveletFwd.cpp:932-935)
    if (n < 2) return;
    const uint32_t sn = (n + 1 - par) >> 1;       // low-pass count
    // predict on the high positions, then update the low positions
    for (uint32_t i = 1 - par; i < n; i += 2) x[i] -= (x[mirror((int64_t)i - 1, n)] + x[mirror((int64_t)i + 1, n)]) >> 1;
    for (uint32_t i = par; i < n; i += 2) x[i] += (x[mirror((int64_t)i - 1, n)] + x[mirror((int64_t)i + 1, n)] + 2) >> 2;
    tmp.resize(n);
    uint32_t k = 0;
    for (uint32_t i = par; i < n; i += 2) tmp[k++] = x[i];
    for (uint32_t i = 1 - par; i < n; i += 2) tmp[k++] = x[i];
    (void)sn;
    memcpy(x, tmp.data(), n * sizeof(int32_t));
}
// A decode with a window (grk_decompress_set_window) runs Grok's partial-tile inverse for every
// tile (CodeStreamDecompress.cpp:389, WaveletReverse.cpp:2237-2246); its single odd sample
// across is shifted, S(buf, 0) >>= 1 (:1551-1554), where the whole-tile path divides (:583).
static bool g_partial_inverse = false;
static void inv53_1d(int32_t* x, uint32_t n, std::vector<int32_t>& tmp, uint32_t par, bool vertical) {
    if (n == 1) {
        // odd single sample: horizontal bandH[0] / 2, vertical bandL[0] >> 1 (WaveletReverse.cpp:583, :636)
        if (par) x[0] = (vertical || g_partial_inverse) ? (x[0] >> 1) : (x[0] / 2);
        return;
    }
    if (n < 2) return;
    const uint32_t sn = (n + 1 - par) >> 1;
    tmp.resize(n);
    uint32_t k = 0;
    for (uint32_t i = par; i < n; i += 2) tmp[i] = x[k++];
    for (uint32_t i = 1 - par; i < n; i += 2) tmp[i] = x[k++];
    (void)sn;
    for (uint32_t i = par; i < n; i += 2) tmp[i] -= (tmp[mirror((int64_t)i - 1, n)] + tmp[mirror((int64_t)i + 1, n)] + 2) >> 2;
    for (uint32_t i = 1 - par; i < n; i += 2) tmp[i] += (tmp[mirror((int64_t)i - 1, n)] + tmp[mirror((int64_t)i + 1, n)]) >> 1;
    memcpy(x, tmp.data(), n * sizeof(int32_t));
}

// ----------------------------------------------------------------------------
// 9/7 irreversible DWT (Annex F.4.8.2; WaveletFwd.cpp:39-44, 964-1025 and
// WaveletReverse.cpp:882-1024, 1272-1351).  Float lifting; a single sample is left as it is
// for either parity (WaveletFwd.cpp:973-976, 1018-1021; WaveletReverse.cpp:1012-1014).
// ----------------------------------------------------------------------------
static const float A97 = -1.586134342f, B97 = -0.052980118f, G97 = 0.882911075f, D97 = 0.443506852f;
static const float K97 = 1.230174105f, INVK97 = (float)(1.0 / 1.230174105), TWO_INVK97 = 1.625732422f;

static void fwd97_1d(float* x, uint32_t n, std::vector<float>& tmp, uint32_t par, bool) {
    if (n < 2) return;
    tmp.resize(n);
    auto X = [&](int64_t i) -> float& { return x[mirror(i, n)]; };
    auto lift = [&](uint32_t start, float c) {   // (left + right) * c added (encode_step2, :135-163)
        for (int64_t i = start; i < (int64_t)n; i += 2) { float t = (X(i - 1) + X(i + 1)) * c; x[i] = x[i] + t; }
    };
    lift(1 - par, A97); lift(par, B97); lift(1 - par, G97); lift(par, D97);
    uint32_t k = 0;
    for (uint32_t i = par; i < n; i += 2) tmp[k++] = x[i] * INVK97;
    for (uint32_t i = 1 - par; i < n; i += 2) tmp[k++] = x[i] * K97;
    memcpy(x, tmp.data(), n * sizeof(float));
}
static void inv97_1d(float* x, uint32_t n, std::vector<float>& tmp, uint32_t par, bool) {
    if (n < 2) return;
    tmp.resize(n);
    uint32_t k = 0;
    for (uint32_t i = par; i < n; i += 2) tmp[i] = x[k++] * K97;
    // high band scaled by 2/K: Grok's decoder step sizes omit the band gain
    // (Quantizer.cpp:31-36, "BUG_WEIRD_TWO_INVK"), WaveletReverse.cpp:365-371
    for (uint32_t i = 1 - par; i < n; i += 2) tmp[i] = x[k++] * TWO_INVK97;
    auto X = [&](int64_t i) -> float& { return tmp[mirror(i, n)]; };
    for (int64_t i = par; i < (int64_t)n; i += 2) tmp[i] -= D97 * (X(i - 1) + X(i + 1));
    for (int64_t i = 1 - par; i < (int64_t)n; i += 2) tmp[i] -= G97 * (X(i - 1) + X(i + 1));
    for (int64_t i = par; i < (int64_t)n; i += 2) tmp[i] -= B97 * (X(i - 1) + X(i + 1));
    for (int64_t i = 1 - par; i < (int64_t)n; i += 2) tmp[i] -= A97 * (X(i - 1) + X(i + 1));
    memcpy(x, tmp.data(), n * sizeof(float));
}

template <typename T, typename F>
static void dwt2d(T* buf, uint32_t stride, const Comp& c, uint32_t numres, bool forward, F f1d) {
    std::vector<T> col, tmp;
    auto level = [&](uint32_t r) {  // transform resolution r (rw x rh) <-> r-1 + 3 bands
        const Res& R = c.res[r];
        uint32_t rw = R.x1 - R.x0, rh = R.y1 - R.y0;
        const uint32_t px = R.x0 & 1, py = R.y0 & 1;   // parity_row / parity_col
        auto vpass = [&]() {
            col.resize(rh);
            for (uint32_t x = 0; x < rw; ++x) {
                for (uint32_t y = 0; y < rh; ++y) col[y] = buf[(size_t)y * stride + x];
                f1d(col.data(), rh, tmp, py, true);
                for (uint32_t y = 0; y < rh; ++y) buf[(size_t)y * stride + x] = col[y];
            }
        };
        if (forward) {
            vpass();                                   // vertical first
            for (uint32_t y = 0; y < rh; ++y) f1d(buf + (size_t)y * stride, rw, tmp, px, false);
        } else {
            for (uint32_t y = 0; y < rh; ++y) f1d(buf + (size_t)y * stride, rw, tmp, px, false);  // horizontal first
            vpass();
        }
    };
    if (forward) for (uint32_t r = numres - 1; r >= 1; --r) level(r);
    else for (uint32_t r = 1; r < numres; ++r) level(r);
}

// ----------------------------------------------------------------------------
// MQ arithmetic coder (Annex C; mqc_enc.cpp:34-330, mqc_dec.cpp, mqc_*_inl.h)
// ----------------------------------------------------------------------------
struct QeEntry { uint16_t qe; uint8_t nmps, nlps, sw; };
static const QeEntry QE[47] = {
    {0x5601, 1, 1, 1}, {0x3401, 2, 6, 0}, {0x1801, 3, 9, 0}, {0x0AC1, 4, 12, 0}, {0x0521, 5, 29, 0},
    {0x0221, 38, 33, 0}, {0x5601, 7, 6, 1}, {0x5401, 8, 14, 0}, {0x4801, 9, 14, 0}, {0x3801, 10, 14, 0},
    {0x3001, 11, 17, 0}, {0x2401, 12, 18, 0}, {0x1C01, 13, 20, 0}, {0x1601, 29, 21, 0}, {0x5601, 15, 14, 1},
    {0x5401, 16, 14, 0}, {0x5101, 17, 15, 0}, {0x4801, 18, 16, 0}, {0x3801, 19, 17, 0}, {0x3401, 20, 18, 0},
    {0x3001, 21, 19, 0}, {0x2801, 22, 19, 0}, {0x2401, 23, 20, 0}, {0x2201, 24, 21, 0}, {0x1C01, 25, 22, 0},
    {0x1801, 26, 23, 0}, {0x1601, 27, 24, 0}, {0x1401, 28, 25, 0}, {0x1201, 29, 26, 0}, {0x1101, 30, 27, 0},
    {0x0AC1, 31, 28, 0}, {0x09C1, 32, 29, 0}, {0x08A1, 33, 30, 0}, {0x0521, 34, 31, 0}, {0x0441, 35, 32, 0},
    {0x02A1, 36, 33, 0}, {0x0221, 37, 34, 0}, {0x0141, 38, 35, 0}, {0x0111, 39, 36, 0}, {0x0085, 40, 37, 0},
    {0x0049, 41, 38, 0}, {0x0025, 42, 39, 0}, {0x0015, 43, 40, 0}, {0x0009, 44, 41, 0}, {0x0005, 45, 42, 0},
    {0x0001, 45, 43, 0}, {0x5601, 46, 46, 0}};

enum { CTX_ZC = 0, CTX_SC = 9, CTX_MAG = 14, CTX_AGG = 17, CTX_UNI = 18, NUM_CTX = 19 };

struct MqEnc {
    uint32_t a, c, ct;
    uint8_t* buf;    // buf[-1] must exist (left pad), buf[-1] == 0
    int64_t bp;      // index into buf, may be -1
    uint8_t st[NUM_CTX], mps[NUM_CTX];
    void reset_states() {                   // mqc_dec.cpp:121-130
        for (int i = 0; i < NUM_CTX; ++i) { st[i] = 0; mps[i] = 0; }
        st[CTX_UNI] = 46; st[CTX_AGG] = 3; st[CTX_ZC] = 4;
    }
    void init(uint8_t* b) { a = 0x8000; c = 0; ct = 12; buf = b; bp = -1; }
    uint8_t& B(int64_t i) { return buf[i]; }
    void byteout() {
        if (B(bp) == 0xff) { ++bp; B(bp) = (uint8_t)(c >> 20); c &= 0xfffff; ct = 7; }
        else if ((c & 0x8000000) == 0) { ++bp; B(bp) = (uint8_t)(c >> 19); c &= 0x7ffff; ct = 8; }
        else {
            B(bp)++;
            if (B(bp) == 0xff) { c &= 0x7ffffff; ++bp; B(bp) = (uint8_t)(c >> 20); c &= 0xfffff; ct = 7; }
            else { ++bp; B(bp) = (uint8_t)(c >> 19); c &= 0x7ffff; ct = 8; }
        }
    }
    void renorm() { do { a <<= 1; c <<= 1; if (--ct == 0) byteout(); } while ((a & 0x8000) == 0); }
    void encode(int cx, uint32_t d) {
        const QeEntry& q = QE[st[cx]];
        if (mps[cx] == d) {
            a -= q.qe;
            if ((a & 0x8000) == 0) {
                if (a < q.qe) a = q.qe; else c += q.qe;
                st[cx] = q.nmps; renorm();
            } else c += q.qe;
        } else {
            a -= q.qe;
            if (a < q.qe) c += q.qe; else a = q.qe;
            if (q.sw) mps[cx] ^= 1;
            st[cx] = q.nlps; renorm();
        }
    }
    void flush() {                          // mqc_enc.cpp:213-227
        uint32_t tempc = c + a;
        c |= 0xffff;
        if (c >= tempc) c -= 0x8000;
        c <<= ct; byteout();
        c <<= ct; byteout();
        if (B(bp) != 0xff) ++bp;
    }
    uint32_t numbytes() const { return (uint32_t)bp; }  // wraps for bp == -1 as in the reference
    // ---- mode switches (mqc_enc.cpp:229-330).  In raw (bypass) mode bp indexes the next byte
    // to write; BYPASS_CT_INIT marks "no raw bit written yet" (mqc_inl.h:24).
    static constexpr uint32_t CT_INIT = 0xDEADBEEFu;
    void bypass_init() { c = 0; ct = CT_INIT; }                                 // :229-246
    void bypass_encode(uint32_t d) {                                           // mqc_enc_inl.h:104-124
        if (ct == CT_INIT) ct = 8;
        --ct;
        c += d << ct;
        if (ct == 0) {
            B(bp) = (uint8_t)c;
            ct = (B(bp) == 0xff) ? 7 : 8;
            ++bp; c = 0;
        }
    }
    uint32_t bypass_extra_bytes(bool erterm) {                                 // :247-250
        return (ct < 7 || (ct == 7 && (erterm || B(bp - 1) != 0xff))) ? 2 : 1;
    }
    void bypass_flush(bool erterm) {                                           // :251-292
        if (ct < 7 || (ct == 7 && (erterm || B(bp - 1) != 0xff))) {
            uint32_t bit = 0;
            while (ct > 0) { --ct; c += bit << ct; bit = 1 - bit; }
            B(bp) = (uint8_t)c;
            ++bp;
        } else if (ct == 7 && B(bp - 1) == 0xff) {
            --bp;
        } else if (ct == 8 && !erterm && B(bp - 1) == 0x7f && B(bp - 2) == 0xff) {
            bp -= 2;
        }
    }
    void restart_init() {                                                      // :294-310
        a = 0x8000; c = 0; ct = 12;
        --bp;
        if (B(bp) == 0xff) ct = 13;
    }
    void erterm() {                                                            // :312-325
        int32_t k = (int32_t)(11 - ct + 1);
        while (k > 0) { c <<= ct; ct = 0; byteout(); k -= (int32_t)ct; }
        if (B(bp) != 0xff) byteout();
    }
    void segmark() { for (uint32_t i = 1; i < 5; ++i) encode(CTX_UNI, i % 2); }   // :327-330
};

struct MqDec {
    const uint8_t* buf; uint32_t len; uint32_t bp;
    uint32_t a, c, ct;
    uint8_t st[NUM_CTX], mps[NUM_CTX];
    std::vector<uint8_t> store;
    uint64_t ndec = 0;           // decisions decoded (instrumentation for tools/t1_simt_stats.py)
    void reset_states() {
        for (int i = 0; i < NUM_CTX; ++i) { st[i] = 0; mps[i] = 0; }
        st[CTX_UNI] = 46; st[CTX_AGG] = 3; st[CTX_ZC] = 4;
    }
    uint8_t at(uint32_t i) const { return i < len ? buf[i] : 0xff; }  // artificial FFFF end marker
    void bytein() {
        uint32_t l_c = at(bp + 1);
        if (at(bp) == 0xff) {
            if (l_c > 0x8f) { c += 0xff00; ct = 8; }
            else { ++bp; c += l_c << 9; ct = 7; }
        } else { ++bp; c += l_c << 8; ct = 8; }
    }
    void init(const uint8_t* b, uint32_t n) {   // mqc_dec.cpp:98-112 (INITDEC)
        buf = b; len = n; bp = 0;
        c = (uint32_t)(((n == 0) ? 0xff : at(0)) << 16);
        bytein();
        c <<= 7; ct -= 7; a = 0x8000;
    }
    void raw_init(const uint8_t* b, uint32_t n) { buf = b; len = n; bp = 0; c = 0; ct = 0; }   // mqc_dec.cpp:108-113
    uint32_t raw_decode() {                                                    // mqc_dec_inl.h:61-91
        if (ct == 0) {
            if (c == 0xff) {
                if (at(bp) > 0x8f) { c = 0xff; ct = 8; }
                else { c = at(bp); ++bp; ct = 7; }
            } else { c = at(bp); ++bp; ct = 8; }
        }
        --ct;
        return (c >> ct) & 1u;
    }
    void renorm() { do { if (ct == 0) bytein(); a <<= 1; c <<= 1; --ct; } while (a < 0x8000); }
    uint32_t decode(int cx) {
        ++ndec;
        const QeEntry& q = QE[st[cx]];
        uint32_t d;
        a -= q.qe;
        if (c < ((uint32_t)q.qe << 16)) {
            if (a < q.qe) { a = q.qe; d = mps[cx]; st[cx] = q.nmps; }
            else { a = q.qe; d = mps[cx] ^ 1; if (q.sw) mps[cx] ^= 1; st[cx] = q.nlps; }
            renorm();
        } else {
            c -= (uint32_t)q.qe << 16;
            if (a < 0x8000) {
                if (a < q.qe) { d = mps[cx] ^ 1; if (q.sw) mps[cx] ^= 1; st[cx] = q.nlps; }
                else { d = mps[cx]; st[cx] = q.nmps; }
                renorm();
            } else d = mps[cx];
        }
        return d;
    }
};

// ----------------------------------------------------------------------------
// EBCOT context tables (Annex D, Tables D.1-D.3; Grok t1_generate_luts.cpp)
// ----------------------------------------------------------------------------
// zero coding: orient, h (0..2), v (0..2), d (0..4)
static int zc_ctx(uint32_t orient, int h, int v, int d) {
    if (orient == 1) std::swap(h, v);      // HL: horizontal and vertical roles swap
    if (orient == 3) {
        int hv = h + v;
        if (d == 0) return hv == 0 ? 0 : (hv == 1 ? 1 : 2);
        if (d == 1) return hv == 0 ? 3 : (hv == 1 ? 4 : 5);
        if (d == 2) return hv == 0 ? 6 : 7;
        return 8;
    }
    if (h == 0) {
        if (v == 0) return d == 0 ? 0 : (d == 1 ? 1 : 2);
        return v == 1 ? 3 : 4;
    }
    if (h == 1) {
        if (v == 0) return d == 0 ? 5 : 6;
        return 7;
    }
    return 8;
}
// sign coding: H, V contributions in {-1,0,1}; returns ctx offset (0..4) and xor bit
static void sc_ctx(int H, int V, int& ctx, int& xorbit) {
    int hc = H, vc = V;
    if (hc == 0 && vc == 0) { ctx = 0; xorbit = 0; return; }
    xorbit = (hc < 0 || (hc == 0 && vc < 0)) ? 1 : 0;
    if (hc < 0) { hc = -hc; vc = -vc; }
    if (hc == 0) ctx = 1;                  // vc = +-1
    else ctx = (vc == -1) ? 2 : (vc == 0 ? 3 : 4);
}

// Per-sample state with a one-sample border (Grok packs the same information
// into 32-bit flag words per 4-row column, T1.cpp:45-130).
enum { S_SIG = 1, S_NEG = 2, S_PI = 4, S_MU = 8 };

// VSC (GRK_CBLKSTY_VSC): a stripe's first row does not update the flags of the row above it
// (update_flags, T1.cpp:209-232, `ci == 0 && !vsc`), i.e. the last row of a stripe sees the
// next stripe's samples as insignificant.
struct T1State {
    uint32_t w, h, sw;  // sw = w + 2
    bool vsc = false;
    std::vector<uint8_t> s;
    void init(uint32_t W, uint32_t H, bool VSC = false) { w = W; h = H; sw = W + 2; vsc = VSC; s.assign((size_t)(W + 2) * (H + 2), 0); }
    uint8_t& at(int x, int y) { return s[(size_t)(y + 1) * sw + (x + 1)]; }
    uint8_t get(int x, int y) const { return s[(size_t)(y + 1) * sw + (x + 1)]; }
    // neighbour (xx, yy) of sample row y
    uint8_t nbr(int xx, int yy, int y) const { return (vsc && yy == y + 1 && (y & 3) == 3) ? 0 : get(xx, yy); }
    void counts(int x, int y, int& hh, int& vv, int& dd) const {
        auto sg = [&](int xx, int yy) { return (nbr(xx, yy, y) & S_SIG) ? 1 : 0; };
        hh = sg(x - 1, y) + sg(x + 1, y);
        vv = sg(x, y - 1) + sg(x, y + 1);
        dd = sg(x - 1, y - 1) + sg(x + 1, y - 1) + sg(x - 1, y + 1) + sg(x + 1, y + 1);
    }
    bool any_sig_nbr(int x, int y) const { int a, b, c; counts(x, y, a, b, c); return (a + b + c) != 0; }
    int contrib(int x, int y, int yc) const {
        uint8_t v = nbr(x, y, yc);
        if (!(v & S_SIG)) return 0;
        return (v & S_NEG) ? -1 : 1;
    }
    void sign_ctx(int x, int y, int& ctx, int& xorbit) const {
        int H = contrib(x - 1, y, y) + contrib(x + 1, y, y);
        int V = contrib(x, y - 1, y) + contrib(x, y + 1, y);
        H = std::max(-1, std::min(1, H)); V = std::max(-1, std::min(1, V));
        sc_ctx(H, V, ctx, xorbit);
    }
};

// ----------------------------------------------------------------------------
// T1 encoder (T1.cpp:498-932 enc_sigpass / enc_refpass / enc_clnpass /
// compress_cblk; T1Part1.cpp:36-127 preCompress), with the code-block style mode
// switches (BYPASS/LAZY, RESET, TERMALL, VSC, PTERM, SEGSYM; mqc_enc.cpp:229-330).
// coef: SMR magnitudes already shifted by T1_NMSEDEC_FRACBITS (6).
// ----------------------------------------------------------------------------
static const int FRACBITS = 6;

struct NmseLuts {
    int16_t sig[1 << 7], sig0[1 << 7], ref[1 << 7], ref0[1 << 7];
    NmseLuts() {  // t1_generate_luts.cpp:338-362
        for (int i = 0; i < (1 << 7); ++i) {
            double t = i / pow(2.0, FRACBITS), u = t, v = t - 1.5;
            sig[i] = (int16_t)std::max(0, (int)(floor((u * u - v * v) * pow(2.0, FRACBITS) + 0.5) / pow(2.0, FRACBITS) * 8192.0));
            sig0[i] = (int16_t)std::max(0, (int)(floor((u * u) * pow(2.0, FRACBITS) + 0.5) / pow(2.0, FRACBITS) * 8192.0));
            u = t - 1.0;
            v = (i & (1 << 6)) ? t - 1.5 : t - 0.5;
            ref[i] = (int16_t)std::max(0, (int)(floor((u * u - v * v) * pow(2.0, FRACBITS) + 0.5) / pow(2.0, FRACBITS) * 8192.0));
            ref0[i] = (int16_t)std::max(0, (int)(floor((u * u) * pow(2.0, FRACBITS) + 0.5) / pow(2.0, FRACBITS) * 8192.0));
        }
    }
};
static const NmseLuts NMSE;
static int nmse_sig(uint32_t x, int bpno) { return bpno > 0 ? NMSE.sig[(x >> bpno) & 127] : NMSE.sig0[x & 127]; }
static int nmse_ref(uint32_t x, int bpno) { return bpno > 0 ? NMSE.ref[(x >> bpno) & 127] : NMSE.ref0[x & 127]; }

struct BlockEncResult {
    uint32_t numbps = 0, npasses = 0;
    std::vector<uint8_t> data;
    std::vector<PassInfo> passes;
};

// weight for distortion (T1.cpp:418-436)
struct DistCtx { uint32_t compno, level, orient, qmfbid; double stepsize; const double* mct_norms; uint32_t mct_nc; };
static double getwmsedec(int nmsedec, const DistCtx& dc, int bpno) {
    double w1 = 1, w2;
    if (dc.mct_norms && dc.compno < dc.mct_nc) w1 = dc.mct_norms[dc.compno];
    w2 = getnorm(dc.level, dc.orient, dc.qmfbid == 1);
    double wm = w1 * w2 * dc.stepsize * (1 << bpno);
    wm *= wm * nmsedec / 8192.0;
    return wm;
}

// Code-block style bits (grok.h:98-104)
enum { STY_LAZY = 0x01, STY_RESET = 0x02, STY_TERMALL = 0x04, STY_VSC = 0x08, STY_PTERM = 0x10, STY_SEGSYM = 0x20 };

// T1::enc_is_term_pass (T1.cpp:437-458)
static bool enc_is_term_pass(uint32_t sty, int numbps, int bpno, int passtype) {
    if (passtype == 2 && bpno == 0) return true;
    if (sty & STY_TERMALL) return true;
    if (sty & STY_LAZY) {
        if (bpno == numbps - 4 && passtype == 2) return true;   // the 4th cleanup pass
        if (bpno < numbps - 4 && passtype > 0) return true;     // later MR (raw) and CL (MQ) passes
    }
    return false;
}

static void t1_encode_block(const uint32_t* mag, const uint8_t* neg, uint32_t w, uint32_t h, uint32_t orient,
                            BlockEncResult& out, const DistCtx* dctx, uint32_t sty = 0) {
    uint32_t mx = 0;
    for (uint32_t i = 0; i < w * h; ++i) mx = std::max(mx, mag[i]);
    out.numbps = 0; out.npasses = 0; out.passes.clear(); out.data.clear();
    if (mx) {
        uint32_t t = (uint32_t)floorlog2(mx) + 1;
        out.numbps = (t <= (uint32_t)FRACBITS) ? 0 : t - FRACBITS;
    }
    if (out.numbps == 0) return;
    T1State S; S.init(w, h, (sty & STY_VSC) != 0);
    // generous buffer: 2-byte left pad (Codeblock.h:156-170)
    std::vector<uint8_t> buf(64 + (size_t)w * h * 4 + (size_t)out.numbps * 3 * 64, 0);
    MqEnc mq; mq.reset_states(); mq.init(buf.data() + 2);
    uint32_t maxpasses = 3 * out.numbps - 2;
    out.passes.resize(maxpasses);
    int bpno = (int)out.numbps - 1;
    int passtype = 2;
    double cum = 0;
    const int nbp = (int)out.numbps;
    for (uint32_t passno = 0; bpno >= 0; ++passno) {
        uint32_t one = 1u << (bpno + FRACBITS);
        int nmsedec = 0;
        // BYPASS: SP and MR passes below the 4th bit-plane are raw (T1.cpp:820-824)
        const bool raw = (sty & STY_LAZY) && bpno < nbp - 4 && passtype < 2;
        if (passno > 0 && out.passes[passno - 1].term) {   // T1.cpp:826-833
            if (raw) mq.bypass_init(); else mq.restart_init();
        }
        auto code = [&](int cx, uint32_t d) { if (raw) mq.bypass_encode(d); else mq.encode(cx, d); };
        auto bit = [&](uint32_t x, uint32_t y) { return (mag[y * w + x] & one) ? 1u : 0u; };
        if (passtype == 0) {            // significance propagation
            for (uint32_t k = 0; k < h; k += 4)
                for (uint32_t x = 0; x < w; ++x)
                    for (uint32_t y = k; y < std::min(k + 4, h); ++y) {
                        uint8_t& st = S.at(x, y);
                        if (st & (S_SIG | S_PI)) continue;
                        int hh, vv, dd; S.counts(x, y, hh, vv, dd);
                        if (hh + vv + dd == 0) continue;
                        uint32_t v = bit(x, y);
                        code(CTX_ZC + zc_ctx(orient, hh, vv, dd), v);
                        if (v) {
                            int cx, xb; S.sign_ctx(x, y, cx, xb);
                            uint32_t sg = neg[y * w + x];
                            if (dctx) nmsedec += nmse_sig(mag[y * w + x], bpno);
                            code(CTX_SC + cx, raw ? sg : (sg ^ (uint32_t)xb));   // raw signs are not predicted
                            st |= S_SIG | (sg ? S_NEG : 0);
                        }
                        st |= S_PI;
                    }
        } else if (passtype == 1) {     // magnitude refinement
            for (uint32_t k = 0; k < h; k += 4)
                for (uint32_t x = 0; x < w; ++x)
                    for (uint32_t y = k; y < std::min(k + 4, h); ++y) {
                        uint8_t& st = S.at(x, y);
                        if ((st & (S_SIG | S_PI)) != S_SIG) continue;
                        int cx = (st & S_MU) ? 2 : (S.any_sig_nbr(x, y) ? 1 : 0);
                        if (dctx) nmsedec += nmse_ref(mag[y * w + x], bpno);
                        code(CTX_MAG + cx, bit(x, y));
                        st |= S_MU;
                    }
        } else {                        // cleanup (always MQ)
            for (uint32_t k = 0; k < h; k += 4)
                for (uint32_t x = 0; x < w; ++x) {
                    uint32_t ylim = std::min(k + 4, h);
                    uint32_t y = k;
                    if (ylim - k == 4) {
                        bool agg = true;
                        for (uint32_t yy = k; yy < ylim && agg; ++yy) {
                            uint8_t st = S.get(x, yy);
                            if (st & (S_SIG | S_PI | S_MU)) agg = false;
                            else if (S.any_sig_nbr(x, yy)) agg = false;
                        }
                        if (agg) {
                            uint32_t runlen = 0;
                            for (; runlen < 4; ++runlen) if (bit(x, k + runlen)) break;
                            mq.encode(CTX_AGG, runlen != 4);
                            if (runlen == 4) continue;
                            mq.encode(CTX_UNI, runlen >> 1);
                            mq.encode(CTX_UNI, runlen & 1);
                            y = k + runlen;
                            // the sample at y is significant: code its sign
                            int cx, xb; S.sign_ctx(x, y, cx, xb);
                            uint32_t sg = neg[y * w + x];
                            if (dctx) nmsedec += nmse_sig(mag[y * w + x], bpno);
                            mq.encode(CTX_SC + cx, sg ^ (uint32_t)xb);
                            S.at(x, y) |= S_SIG | (sg ? S_NEG : 0);
                            ++y;
                        }
                    }
                    for (; y < ylim; ++y) {
                        uint8_t& st = S.at(x, y);
                        if (st & (S_SIG | S_PI)) continue;
                        int hh, vv, dd; S.counts(x, y, hh, vv, dd);
                        uint32_t v = bit(x, y);
                        mq.encode(CTX_ZC + zc_ctx(orient, hh, vv, dd), v);
                        if (v) {
                            int cx, xb; S.sign_ctx(x, y, cx, xb);
                            uint32_t sg = neg[y * w + x];
                            if (dctx) nmsedec += nmse_sig(mag[y * w + x], bpno);
                            mq.encode(CTX_SC + cx, sg ^ (uint32_t)xb);
                            st |= S_SIG | (sg ? S_NEG : 0);
                        }
                    }
                    for (uint32_t yy = k; yy < ylim; ++yy) S.at(x, yy) &= (uint8_t)~S_PI;
                }
            if (sty & STY_SEGSYM) mq.segmark();
        }
        PassInfo& P = out.passes[passno];
        if (dctx) { cum += getwmsedec(nmsedec, *dctx, bpno); P.dist = cum; } else P.dist = 0;
        if (enc_is_term_pass(sty, nbp, bpno, passtype)) {   // T1.cpp:856-869
            if (raw) mq.bypass_flush((sty & STY_PTERM) != 0);
            else if (sty & STY_PTERM) mq.erterm();
            else mq.flush();
            P.term = 1; P.rate = mq.numbytes();
        } else {
            uint32_t extra;                           // T1.cpp:870-897
            if (raw) extra = mq.bypass_extra_bytes((sty & STY_PTERM) != 0);
            else { extra = 4 + 1; if (mq.ct < 5) extra++; }
            P.term = 0; P.rate = mq.numbytes() + extra;
        }
        if (++passtype == 3) { passtype = 0; --bpno; }
        if (sty & STY_RESET) mq.reset_states();
        out.npasses = passno + 1;
    }
    out.passes.resize(out.npasses);
    uint32_t last = mq.numbytes();
    for (uint32_t i = out.npasses; i > 0;) {         // monotone rates, T1.cpp:907-919
        PassInfo& P = out.passes[--i];
        if (P.rate > last) P.rate = last; else last = P.rate;
    }
    const uint8_t* d = buf.data() + 2;
    for (uint32_t i = 0; i < out.npasses; ++i) {     // FF back-off, T1.cpp:920-930
        PassInfo& P = out.passes[i];
        if (d[P.rate - 1] == 0xff) P.rate--;
        P.len = P.rate - (i == 0 ? 0 : out.passes[i - 1].rate);
    }
    out.data.assign(d, d + out.passes[out.npasses - 1].rate);
}

// ----------------------------------------------------------------------------
// T1 decoder (T1.cpp:934-1446).  Output: magnitudes scaled by 2 with the
// half-bit reconstruction (oneplushalf), sign applied, like Grok's
// uncompressedData before PostDecompressFilters.
// ----------------------------------------------------------------------------
// stripe_counts (optional, instrumentation): decisions per (pass, stripe), pass-major.
// Passes of codeword segment `seg` (T2Decompress::initSegment, T2Decompress.cpp:28-54):
// TERMALL one pass each; BYPASS 10, then alternately 2 (raw SP + MR) and 1 (MQ CL);
// otherwise one segment of every pass.
static uint32_t seg_maxpasses(uint32_t sty, uint32_t seg) {
    if (sty & STY_TERMALL) return 1;
    if (sty & STY_LAZY) return seg == 0 ? 10 : ((seg & 1) ? 2 : 1);
    return 0xffffffffu;
}

// seglens: byte length of each codeword segment (concatenated in `data`); empty = one
// segment of `len` bytes.
static void t1_decode_block(const uint8_t* data, uint32_t len, uint32_t npasses, uint32_t numbps,
                            uint32_t orient, uint32_t w, uint32_t h, int32_t* out, uint32_t* stripe_counts = nullptr,
                            uint32_t sty = 0, const std::vector<uint32_t>* seglens = nullptr) {
    std::fill(out, out + (size_t)w * h, 0);
    if (!npasses || !numbps) return;
    T1State S; S.init(w, h, (sty & STY_VSC) != 0);
    MqDec mq; mq.reset_states();
    const uint32_t ns = (h + 3) / 4;
    auto tick = [&](uint32_t p, uint32_t k) {
        if (stripe_counts) stripe_counts[p * ns + k / 4] = (uint32_t)mq.ndec;
        return true;
    };
    int bpno1 = (int)numbps;   // bpno_plus_one
    int passtype = 2;
    uint32_t p = 0, segno = 0, off = 0, seg_left = 0;
    bool raw = false;
    for (; p < npasses && bpno1 >= 1; ++p) {
        if (seg_left == 0) {   // next codeword segment (T1::decompress_cblk, T1.cpp:1380-1400)
            const uint32_t sl = seglens ? (segno < seglens->size() ? (*seglens)[segno] : 0) : len;
            const uint32_t sb = std::min(sl, len - std::min(off, len));
            raw = (sty & STY_LAZY) && bpno1 <= (int)numbps - 4 && passtype < 2;
            if (raw) mq.raw_init(data + off, sb); else mq.init(data + off, sb);
            off += sb;
            seg_left = seg_maxpasses(sty, segno++);
        }
        --seg_left;
        int32_t one = 1 << bpno1, half = one >> 1, oph = one | half;
        auto dec = [&](int cx) { return raw ? mq.raw_decode() : mq.decode(cx); };
        if (passtype == 0) {
            for (uint32_t k = 0; k < h && tick(p, k); k += 4)
                for (uint32_t x = 0; x < w; ++x)
                    for (uint32_t y = k; y < std::min(k + 4, h); ++y) {
                        uint8_t& st = S.at(x, y);
                        if (st & (S_SIG | S_PI)) continue;
                        int hh, vv, dd; S.counts(x, y, hh, vv, dd);
                        if (hh + vv + dd == 0) continue;
                        if (dec(CTX_ZC + zc_ctx(orient, hh, vv, dd))) {
                            int cx, xb; S.sign_ctx(x, y, cx, xb);
                            uint32_t sg = raw ? mq.raw_decode() : (mq.decode(CTX_SC + cx) ^ (uint32_t)xb);
                            out[y * w + x] = sg ? -oph : oph;
                            st |= S_SIG | (sg ? S_NEG : 0);
                        }
                        st |= S_PI;
                    }
        } else if (passtype == 1) {
            int32_t poshalf = half;
            for (uint32_t k = 0; k < h && tick(p, k); k += 4)
                for (uint32_t x = 0; x < w; ++x)
                    for (uint32_t y = k; y < std::min(k + 4, h); ++y) {
                        uint8_t& st = S.at(x, y);
                        if ((st & (S_SIG | S_PI)) != S_SIG) continue;
                        int cx = (st & S_MU) ? 2 : (S.any_sig_nbr(x, y) ? 1 : 0);
                        uint32_t v = dec(CTX_MAG + cx);
                        int32_t& o = out[y * w + x];
                        o += (v ^ (o < 0 ? 1u : 0u)) ? poshalf : -poshalf;
                        st |= S_MU;
                    }
        } else {
            for (uint32_t k = 0; k < h && tick(p, k); k += 4)
                for (uint32_t x = 0; x < w; ++x) {
                    uint32_t ylim = std::min(k + 4, h);
                    uint32_t y = k;
                    bool partial = false;
                    if (ylim - k == 4) {
                        bool agg = true;
                        for (uint32_t yy = k; yy < ylim && agg; ++yy) {
                            uint8_t st = S.get(x, yy);
                            if (st & (S_SIG | S_PI | S_MU)) agg = false;
                            else if (S.any_sig_nbr(x, yy)) agg = false;
                        }
                        if (agg) {
                            if (!mq.decode(CTX_AGG)) { continue; }
                            uint32_t r = mq.decode(CTX_UNI);
                            r = (r << 1) | mq.decode(CTX_UNI);
                            y = k + r;
                            partial = true;
                        }
                    }
                    for (; y < ylim; ++y) {
                        uint8_t& st = S.at(x, y);
                        if (!partial) {
                            if (st & (S_SIG | S_PI)) continue;
                            int hh, vv, dd; S.counts(x, y, hh, vv, dd);
                            if (!mq.decode(CTX_ZC + zc_ctx(orient, hh, vv, dd))) continue;
                        }
                        partial = false;
                        int cx, xb; S.sign_ctx(x, y, cx, xb);
                        uint32_t sg = mq.decode(CTX_SC + cx) ^ (uint32_t)xb;
                        out[y * w + x] = sg ? -oph : oph;
                        st |= S_SIG | (sg ? S_NEG : 0);
                    }
                    for (uint32_t yy = k; yy < ylim; ++yy) S.at(x, yy) &= (uint8_t)~S_PI;
                }
            if (sty & STY_SEGSYM)   // dec_clnpass_check_segsym: four UNIFORM decisions
                for (int i = 0; i < 4; ++i) mq.decode(CTX_UNI);
        }
        if ((sty & STY_RESET) && !raw) mq.reset_states();   // T1.cpp:1420-1421
        if (++passtype == 3) { passtype = 0; --bpno1; }
    }
    if (stripe_counts) stripe_counts[(size_t)npasses * ns] = (uint32_t)mq.ndec;
}

// ----------------------------------------------------------------------------
// Bit I/O for packet headers (t2/BitIO.cpp) and tag trees (t2/TagTree.h)
// ----------------------------------------------------------------------------
struct BitWriter {
    std::vector<uint8_t>* out; uint8_t buf = 0; int ct = 8;
    // ops (optional): every write() call as (value, bits, whether the caller checks its result),
    // for replaying the header through Grok's bounded BitIO (GrkSimBitIO below)
    std::vector<uint64_t>* ops = nullptr;
    void wbyte() { out->push_back(buf); ct = (buf == 0xff) ? 7 : 8; buf = 0; }
    void putbit(uint32_t b) { if (ct == 0) wbyte(); --ct; buf |= (uint8_t)(b << ct); }
    void write(uint32_t v, int n, bool checked = true) {
        if (ops) ops->push_back((uint64_t)v | ((uint64_t)n << 32) | ((uint64_t)checked << 40));
        for (int i = n - 1; i >= 0; --i) putbit((v >> i) & 1);
    }
    void flush() { wbyte(); if (ct == 7) wbyte(); }
    // BitIO::putcommacode / putnumpasses (BitIO.cpp:144-178) return nothing: the callers never
    // see a failed write inside them
    void commacode(uint32_t n) { for (uint32_t i = 0; i < n; ++i) write(1, 1, false); write(0, 1, false); }
    void numpasses(uint32_t n) {
        if (n == 1) write(0, 1, false);
        else if (n == 2) write(2, 2, false);
        else if (n <= 5) write(0xc | (n - 3), 4, false);
        else if (n <= 36) write(0x1e0 | (n - 6), 9, false);
        else if (n <= 164) write(0xff80 | (n - 37), 16, false);
    }
};

// Grok's bounded BitIO as compressPacketSimulate uses it (BitIO(nullptr, max_bytes, true),
// BitIO.cpp:24-52, 80-122): writeByte counts a byte and fails when the count reaches buf_len
// (never when buf_len is 0: the count starts above it), leaving the pending byte and ct as they
// were; putbit fails when that writeByte fails, and write() returns at the first failed bit,
// dropping the rest of its value.  A failure inside putcommacode / putnumpasses is ignored, so
// the header goes on: the next writeByte counts the same byte again (count buf_len + 1 != buf_len
// succeeds) and nothing fails after it.  Replays a header's write() calls; returns false when a
// checked write or the flush fails, else the byte count (BitIO::numBytes) in *nbytes.
struct GrkSimBitIO {
    uint64_t offset = 0, buf_len; uint8_t buf = 0; int ct = 8;
    explicit GrkSimBitIO(uint64_t len) : buf_len(len) {}
    bool write_byte() { ++offset; if (offset == buf_len) return false; ct = buf == 0xff ? 7 : 8; buf = 0; return true; }
    bool putbit(uint32_t b) { if (ct == 0 && !write_byte()) return false; --ct; buf = (uint8_t)(buf | (b << ct)); return true; }
    bool write(uint32_t v, int n) { for (int i = n - 1; i >= 0; --i) if (!putbit((v >> i) & 1)) return false; return true; }
    bool flush() { if (!write_byte()) return false; return ct == 7 ? write_byte() : true; }
};
static bool grk_sim_header(const std::vector<uint64_t>& ops, uint64_t buf_len, uint64_t* nbytes) {
    GrkSimBitIO b(buf_len);
    for (uint64_t op : ops)
        if (!b.write((uint32_t)op, (int)((op >> 32) & 0xff)) && (op >> 40)) return false;
    if (!b.flush()) return false;
    *nbytes = b.offset;
    return true;
}
struct BitReader {
    const uint8_t* p; size_t len; size_t off = 0; uint8_t buf = 0; int ct = 0;
    void bytein() {
        int prev_ff = (buf == 0xff);
        ct = prev_ff ? 7 : 8;
        buf = off < len ? p[off] : 0;
        ++off;
    }
    uint32_t getbit() { if (ct == 0) bytein(); --ct; return (buf >> ct) & 1; }
    uint32_t read(int n) { uint32_t v = 0; for (int i = n - 1; i >= 0; --i) v |= getbit() << i; return v; }
    void align() { if (buf == 0xff) bytein(); ct = 0; }
    uint32_t numpasses() {
        if (!read(1)) return 1;
        if (!read(1)) return 2;
        uint32_t n = read(2);
        if (n != 3) return n + 3;
        n = read(5);
        if (n != 31) return n + 6;
        return read(7) + 37;
    }
    uint32_t commacode() { uint32_t n = 0; while (read(1)) ++n; return n; }
};

struct TagTree {
    struct Node { int parent; uint32_t value, low; bool known; };
    std::vector<Node> nodes; uint32_t nleaves = 0;
    static const uint32_t UNINIT = 0xffffffffu;
    void build(uint32_t nw, uint32_t nh) {
        // level sizes
        std::vector<uint32_t> lw, lh; lw.push_back(nw); lh.push_back(nh);
        size_t total = 0;
        while (true) { total += (size_t)lw.back() * lh.back(); if ((size_t)lw.back() * lh.back() <= 1) break; lw.push_back((lw.back() + 1) / 2); lh.push_back((lh.back() + 1) / 2); }
        nodes.assign(total, Node{-1, UNINIT, 0, false});
        nleaves = nw * nh;
        size_t base = 0;
        for (size_t l = 0; l + 1 < lw.size(); ++l) {
            size_t nbase = base + (size_t)lw[l] * lh[l];
            for (uint32_t y = 0; y < lh[l]; ++y)
                for (uint32_t x = 0; x < lw[l]; ++x)
                    nodes[base + (size_t)y * lw[l] + x].parent = (int)(nbase + (size_t)(y / 2) * lw[l + 1] + x / 2);
            base = nbase;
        }
        reset();
    }
    void reset() { for (auto& n : nodes) { n.value = UNINIT; n.low = 0; n.known = false; } }
    void setvalue(uint32_t leaf, uint32_t v) {
        int n = (int)leaf;
        while (n >= 0 && nodes[n].value > v) { nodes[n].value = v; n = nodes[n].parent; }
    }
    void encode(BitWriter& bw, uint32_t leaf, uint32_t threshold) {
        int stk[40]; int sp = 0; int n = (int)leaf;
        while (nodes[n].parent >= 0) { stk[sp++] = n; n = nodes[n].parent; }
        uint32_t low = 0;
        while (true) {
            Node& N = nodes[n];
            if (N.low < low) N.low = low; else low = N.low;
            while (low < threshold) {
                if (low >= N.value) { if (!N.known) { bw.write(1, 1); N.known = true; } break; }
                bw.write(0, 1); ++low;
            }
            N.low = low;
            if (sp == 0) break;
            n = stk[--sp];
        }
    }
    uint32_t decode(BitReader& br, uint32_t leaf, uint32_t threshold) {
        int stk[40]; int sp = 0; int n = (int)leaf;
        while (nodes[n].parent >= 0) { stk[sp++] = n; n = nodes[n].parent; }
        uint32_t low = 0;
        while (true) {
            Node& N = nodes[n];
            if (N.low < low) N.low = low; else low = N.low;
            while (low < threshold && low < N.value) {
                if (br.read(1)) { N.value = low; break; }
                ++low;
            }
            N.low = low;
            if (sp == 0) break;
            n = stk[--sp];
        }
        return nodes[n].value;
    }
};

// ----------------------------------------------------------------------------
// Codestream writer / reader (CodeStreamCompress.cpp: SIZ/COD/QCD/COM/SOT,
// T2Compress.cpp:113-240 packet headers; T2Decompress.cpp:216-570)
// ----------------------------------------------------------------------------
static void put16(std::vector<uint8_t>& o, uint32_t v) { o.push_back((uint8_t)(v >> 8)); o.push_back((uint8_t)v); }
static void put32(std::vector<uint8_t>& o, uint32_t v) { put16(o, v >> 16); put16(o, v & 0xffff); }
static uint32_t get16(const uint8_t* p) { return ((uint32_t)p[0] << 8) | p[1]; }
static uint32_t get32(const uint8_t* p) { return (get16(p) << 16) | get16(p + 2); }

struct Image {
    uint32_t w, h, nc, prec; bool sgnd;
    // decode: per-component precision and signedness (SIZ Ssiz; empty = prec / sgnd for all)
    std::vector<uint32_t> cprec;
    std::vector<uint8_t> csgnd;
    uint32_t pr(uint32_t c) const { return c < cprec.size() ? cprec[c] : prec; }
    bool sg(uint32_t c) const { return c < csgnd.size() ? csgnd[c] != 0 : sgnd; }
};

// Tile grid (B.3, CodeStreamCompress.cpp:352-363): nominal tile size (tw, th) anchored at the grid
// origin (gx0, gy0); without tiling one tile from the grid origin to the image's far corner.  Tile
// rectangles are canvas coordinates clipped to the image area [x0, x0 + W) x [y0, y0 + H).
static uint32_t tile_count(const Params& p, uint32_t W, uint32_t H) {
    const uint32_t X1 = p.x0 + W, Y1 = p.y0 + H;
    uint32_t tw = p.tw ? p.tw : X1 - p.gx0, th = p.th ? p.th : Y1 - p.gy0;
    return ((X1 - p.gx0 + tw - 1) / tw) * ((Y1 - p.gy0 + th - 1) / th);
}
static void tile_rect(const Params& p, uint32_t W, uint32_t H, uint32_t t, uint32_t& x0, uint32_t& y0, uint32_t& x1,
                      uint32_t& y1) {
    const uint32_t X1 = p.x0 + W, Y1 = p.y0 + H;
    uint32_t tw = p.tw ? p.tw : X1 - p.gx0, th = p.th ? p.th : Y1 - p.gy0;
    uint32_t ntx = (X1 - p.gx0 + tw - 1) / tw;
    x0 = std::max(p.gx0 + (t % ntx) * tw, p.x0); y0 = std::max(p.gy0 + (t / ntx) * th, p.y0);
    x1 = std::min(p.gx0 + (t % ntx + 1) * tw, X1); y1 = std::min(p.gy0 + (t / ntx + 1) * th, Y1);
}

// Component c's plane: the image area divided by its subsampling, each edge rounded up
// (grk_image_comp w / h; the caller's planes are these sizes, back to back)
static void comp_size(const Params& p, uint32_t W, uint32_t H, uint32_t c, uint32_t& cw, uint32_t& ch) {
    cw = ceildiv(p.x0 + W, p.sx(c)) - ceildiv(p.x0, p.sx(c));
    ch = ceildiv(p.y0 + H, p.sy(c)) - ceildiv(p.y0, p.sy(c));
}
static std::vector<size_t> plane_offsets(const Params& p, uint32_t W, uint32_t H, uint32_t nc) {
    std::vector<size_t> o(nc + 1, 0);
    for (uint32_t c = 0; c < nc; ++c) {
        uint32_t cw, ch;
        comp_size(p, W, H, c, cw, ch);
        o[c + 1] = o[c] + (size_t)cw * ch;
    }
    return o;
}
// The MCT needs the first three components on one sampling grid: Grok disables it otherwise
// (CodeStreamCompress.cpp:501-512), and below three components
static void settle_mct(Params& p, uint32_t nc) {
    if (nc < 3 || p.sx(0) != p.sx(1) || p.sx(0) != p.sx(2) || p.sy(0) != p.sy(1) || p.sy(0) != p.sy(2)) p.mct = 0;
}

// Main header: SOC SIZ [CAP] COD QCD [TLM] [COM] (CodeStreamCompress::init_header_writing
// :822-860).  *tlm_pos receives the offset of the first TLM entry (6 bytes per tile
// part: Ttlm u16, Ptlm u32; Stlm = 0x60, LengthCache.cpp:437-482), patched later.
static int tile_parts(const Params& p, uint32_t nc);   // tile parts per tile from the divider (below)
static int num_parts(const Params& p, uint32_t nc);    // tile parts per tile (divider or POC entries)

// POC marker (A.6.6): RSpoc, CSpoc, LYEpoc (16 bit), REpoc, CEpoc, Ppoc per entry; CSpoc /
// CEpoc take two bytes when there are more than 256 components, CEpoc 0 means 256.  The
// entries are appended to `out` (CodeStreamDecompress::read_poc :1148-1231 appends to the
// tcp's list at :1171-1172: a tile-part POC extends the main header's list the tile's tcp
// was copied from, and a later tile part's POC extends it again).
static bool read_poc(const uint8_t* s, uint32_t L, uint32_t nc, std::vector<PocE>& out) {
    const uint32_t cw = nc <= 256 ? 1 : 2, esz = 5 + 2 * cw;
    if (L < 2 + esz || (L - 2) % esz) return false;
    for (uint32_t q = 0; q + esz <= L - 2; q += esz) {
        const uint8_t* e = s + q;
        PocE v;
        v.rs = e[0]; v.cs = cw == 1 ? e[1] : get16(e + 1); v.lye = get16(e + 1 + cw); v.re = e[3 + cw];
        v.ce = cw == 1 ? e[4 + cw] : get16(e + 4 + cw);
        if (cw == 1 && v.ce == 0) v.ce = 256;
        v.prog = e[4 + 2 * cw];
        if (v.prog > 4) return false;
        out.push_back(v);
    }
    return true;
}
static void write_poc(std::vector<uint8_t>& o, const std::vector<PocE>& pocs, uint32_t nc) {   // CodeStreamCompress::writePoc
    const uint32_t cw = nc <= 256 ? 1 : 2;
    put16(o, 0xff5f); put16(o, 2 + (uint32_t)pocs.size() * (5 + 2 * cw));
    for (const PocE& e : pocs) {
        o.push_back((uint8_t)e.rs);
        if (cw == 1) o.push_back((uint8_t)e.cs); else put16(o, e.cs);
        put16(o, e.lye);
        o.push_back((uint8_t)e.re);
        if (cw == 1) o.push_back((uint8_t)e.ce); else put16(o, e.ce);
        o.push_back((uint8_t)e.prog);
    }
}
static void write_main_header(std::vector<uint8_t>& o, const Image& im, const Params& p, const Comp& c0,
                              size_t* tlm_pos = nullptr) {
    put16(o, 0xff4f);                               // SOC
    put16(o, 0xff51); put16(o, 38 + 3 * im.nc);     // SIZ
    put16(o, p.ht() ? 0x4000 : 0);                  // Rsiz (GRK_JPH_RSIZ_FLAG for HT, CodeStreamCompress.cpp:216-219)
    put32(o, p.x0 + im.w); put32(o, p.y0 + im.h); put32(o, p.x0); put32(o, p.y0);   // Xsiz Ysiz XOsiz YOsiz
    put32(o, p.tw ? p.tw : p.x0 + im.w - p.gx0); put32(o, p.th ? p.th : p.y0 + im.h - p.gy0);
    put32(o, p.gx0); put32(o, p.gy0);                                                 // XTOsiz YTOsiz
    put16(o, im.nc);
    for (uint32_t i = 0; i < im.nc; ++i) {          // Ssiz, XRsiz, YRsiz
        o.push_back((uint8_t)((im.prec - 1) | (im.sgnd ? 0x80 : 0)));
        o.push_back((uint8_t)p.sx(i)); o.push_back((uint8_t)p.sy(i));
    }
    if (p.ht()) {                                   // CAP (CodeStreamCompress::write_cap :1064-1111)
        uint32_t B = 0;
        // param_qcd::get_MAGBp (HTParams.cpp:318-336): reversible expn + guard - 1; scalar
        // expounded expn + guard - nb, nb = the band's decomposition level (LL: num_decomps),
        // in unsigned arithmetic as there
        for (uint32_t r = 0; r < p.numres; ++r)
            for (auto& Bd : c0.res[r].bands) {
                const uint32_t nb = p.irreversible ? (p.numres - 1) - (r ? r - 1 : 0) : 1u;
                B = std::max(B, Bd.expn + p.numgbits - nb);
            }
        // an ROI upshift adds its bit-planes to the magnitudes (15444-15 A.2: MAGBp bounds the
        // coded magnitude bit-planes; Grok's encoder never applies the shift)
        uint32_t rmax = 0;
        for (uint32_t c = 0; c < im.nc; ++c) rmax = std::max(rmax, p.roi(c));
        B += rmax;
        uint32_t Bp = B <= 8 ? 0 : B < 28 ? B - 8 : B < 48 ? 13 + (B >> 2) : 31;
        put16(o, 0xff50); put16(o, 8); put32(o, 0x00020000); put16(o, (p.irreversible ? 0x20 : 0) | Bp);
    }
    bool custom_prc = false;
    for (uint32_t r = 0; r < p.numres; ++r) if (p.prcw_exp[r] != 15 || p.prch_exp[r] != 15) custom_prc = true;
    put16(o, 0xff52); put16(o, 12 + (custom_prc ? p.numres : 0));  // COD
    o.push_back((uint8_t)((custom_prc ? 1 : 0) | p.sop_eph));   // Scod: precincts, SOP, EPH
    o.push_back((uint8_t)p.prog);                   // progression order
    put16(o, p.nlayers);
    o.push_back((uint8_t)((p.mct && im.nc >= 3) ? 1 : 0));
    o.push_back((uint8_t)(p.numres - 1));
    o.push_back((uint8_t)(p.cbw_exp - 2)); o.push_back((uint8_t)(p.cbh_exp - 2));
    o.push_back((uint8_t)p.cblk_sty);               // cblk style
    o.push_back(p.irreversible ? 0 : 1);
    if (custom_prc) for (uint32_t r = 0; r < p.numres; ++r) o.push_back((uint8_t)(p.prcw_exp[r] | (p.prch_exp[r] << 4)));
    uint32_t nbands = 3 * p.numres - 2;              // QCD
    // Sqcd + SPqcd of a component: no quantisation (5/3), scalar expounded, or scalar derived (LL only)
    auto quant_body = [&](const Comp& cc, uint32_t gbits) {
        std::vector<uint8_t> q;
        if (!p.irreversible) {
            q.push_back((uint8_t)(gbits << 5));
            for (uint32_t r = 0; r < p.numres; ++r) for (auto& B : cc.res[r].bands) q.push_back((uint8_t)(B.expn << 3));
        } else {
            q.push_back((uint8_t)((gbits << 5) | (p.qderived ? 1 : 2)));
            for (uint32_t r = 0; r < (p.qderived ? 1u : p.numres); ++r)
                for (auto& B : cc.res[r].bands) {
                    const uint32_t v = (B.expn << 11) | B.mant;
                    q.push_back((uint8_t)(v >> 8)); q.push_back((uint8_t)(v & 0xff));
                }
        }
        return q;
    };
    (void)nbands;
    const std::vector<uint8_t> q0 = quant_body(c0, p.gb(0));
    put16(o, 0xff5c); put16(o, (uint32_t)(2 + q0.size()));
    o.insert(o.end(), q0.begin(), q0.end());
    // QCC for every component whose quantisation differs from component 0's (write_all_qcc,
    // CodeStreamCompress.cpp:1384-1396): Cqcc (one byte below 257 components), Sqcc, SPqcc
    for (uint32_t c = 1; c < im.nc; ++c) {
        if (p.gb(c) == p.gb(0) && p.qshift(c) == p.qshift(0)) continue;
        Comp cc = c0;
        assign_steps(cc, p, im.prec, true, nullptr, im.sgnd ? 1 : 0, 0, c);
        const std::vector<uint8_t> qc = quant_body(cc, p.gb(c));
        if (qc == q0) continue;
        const uint32_t cw = im.nc <= 256 ? 1 : 2;
        put16(o, 0xff5d); put16(o, (uint32_t)(2 + cw + qc.size()));
        if (cw == 2) put16(o, c); else o.push_back((uint8_t)c);
        o.insert(o.end(), qc.begin(), qc.end());
    }
    if (p.tlm) {                                     // TLM (TileLengthMarkers::writeBegin)
        uint32_t nt = tile_count(p, im.w, im.h) * (uint32_t)std::max(1, num_parts(p, im.nc));   // entries per tile part
        put16(o, 0xff55); put16(o, 4 + 6 * nt); o.push_back(0); o.push_back(0x60);
        if (tlm_pos) *tlm_pos = o.size();
        o.insert(o.end(), (size_t)6 * nt, 0);
    }
    // POC of tile 0 in the main header (init_header_writing :839-840), as given: writePoc
    // (:1278-1340) writes each entry before clamping it to the tile's layers / resolutions /
    // components; every tile here shares tile 0's list
    if (!p.pocs.empty()) write_poc(o, p.pocs, im.nc);
    for (uint32_t c = 0; c < im.nc; ++c)            // RGN (CodeStreamCompress::write_rgn :746-780)
        if (p.roi(c)) {
            const uint32_t cw = im.nc <= 256 ? 1 : 2;
            put16(o, 0xff5e); put16(o, 4 + cw);
            if (cw == 1) o.push_back((uint8_t)c); else put16(o, c);
            o.push_back(0); o.push_back((uint8_t)p.roi(c));
        }
    if (!p.comments.empty()) {
        for (const auto& c : p.comments) {
            put16(o, 0xff64); put16(o, 4 + (uint32_t)c.second.size()); put16(o, c.first);
            o.insert(o.end(), c.second.begin(), c.second.end());
        }
    } else if (p.write_com) {                        // COM (CodeStreamCompress.cpp:334, 1114)
        const char* txt = "Created by Grok     version 9.2.0";
        put16(o, 0xff64); put16(o, 4 + (uint32_t)strlen(txt)); put16(o, 1);
        o.insert(o.end(), txt, txt + strlen(txt));
    }
}

// Packet header + body for one (comp, res, precinct, layer) (T2Compress.cpp:113-260,
// compressPacket / compressPacketSimulate :262-430).  Block k contributes
// K.layer_np[layno] passes.  With a byte budget, fails like Grok's bounded
// BitIO (the header must stay below the budget) and body check.  Appends the
// packet to *o when o is non-null.  Updates the per-block T2 state.
// Packet iterator (ISO 15444-1 B.12.1; PacketIter::next_* PacketIter.cpp:100-266): the
// position-driven orders walk y, x from the tile origin in steps of the smallest precinct
// (then at the step's multiples, `y += dy - y % dy`) and emit a precinct of resolution r
// where the position is a multiple of its size, or the tile origin when the resolution's
// origin is not (generatePrecinctIndex, :287-335).  Each packet at most once.
struct PktRef { uint32_t l, r, c, pi; };
// One progression over layers [0, nlayers), resolutions [r0, r1), components [c0, c1); packets
// already in `seen` (per (c, r, pi, l)) are skipped (PacketIter::update_include).
static void packet_iter_one(const std::vector<Comp>& comps, const Params& p, uint32_t prog, uint32_t tx0, uint32_t ty0,
                            uint32_t tx1, uint32_t ty1, uint32_t nlayers, uint32_t L, uint32_t r0, uint32_t r1,
                            uint32_t c0, uint32_t c1, std::vector<uint8_t>& seen, const std::vector<uint32_t>& base,
                            std::vector<PktRef>& v, std::vector<uint32_t>* entry = nullptr, uint32_t ei = 0,
                            uint32_t* iter = nullptr) {
    // (per-component resolution counts: a COC may give a component fewer decomposition levels;
    // resolution r of a component without it has no packets, PacketIter.cpp:160-162)
    const uint32_t nc = (uint32_t)comps.size();
    uint32_t nr = 0;
    for (const Comp& C : comps) nr = std::max<uint32_t>(nr, (uint32_t)C.res.size());
    auto nres = [&](uint32_t c) { return (uint32_t)comps[c].res.size(); };
    auto nprc = [&](uint32_t c, uint32_t r) {
        if (r >= nres(c)) return 0u;
        const Res& R = comps[c].res[r];
        return (R.x1 > R.x0 && R.y1 > R.y0) ? R.pw * R.ph : 0u;
    };
    auto put = [&](uint32_t l, uint32_t r, uint32_t c, uint32_t pi) {
        uint8_t& f = seen[((size_t)base[c * nr + r] + pi) * L + l];
        const uint32_t it = iter ? (*iter)++ : 0;
        if (f) return;
        f = 1;
        v.push_back({l, r, c, pi});
        if (entry) { entry->push_back(ei); entry->push_back(it); }
    };
    if (prog == 0 || prog == 1) {
        for (uint32_t a = (prog == 0 ? 0 : r0); a < (prog == 0 ? nlayers : r1); ++a)
            for (uint32_t b = (prog == 0 ? r0 : 0); b < (prog == 0 ? r1 : nlayers); ++b)
                for (uint32_t c = c0; c < c1; ++c) {
                    const uint32_t l = prog == 0 ? a : b, r = prog == 0 ? b : a;
                    for (uint32_t pi = 0; pi < nprc(c, r); ++pi) put(l, r, c, pi);
                }
        return;
    }
    // the walk's step: the smallest precinct on the canvas, XRsiz * 2^(PPx + level) over the
    // components (update_dxy, PacketIter.cpp:366-388; CPRL takes its component's alone, :63-65)
    uint64_t dx = ~0ull, dy = ~0ull;
    auto steps = [&](uint32_t ca, uint32_t cb) {
        dx = ~0ull; dy = ~0ull;
        for (uint32_t c = ca; c < cb; ++c)
            for (uint32_t r = 0; r < nres(c); ++r) {
                const uint32_t lv = nres(c) - 1 - r;
                dx = std::min<uint64_t>(dx, (uint64_t)p.sx(c) << (comps[c].res[r].prcw_exp + lv));
                dy = std::min<uint64_t>(dy, (uint64_t)p.sy(c) << (comps[c].res[r].prch_exp + lv));
            }
    };
    steps(0, nc);
    // generatePrecinctIndex (:287-335): a precinct of resolution r of component c starts where the
    // canvas position is a multiple of XRsiz * 2^(PPx + level), or at the tile origin when the
    // resolution's origin is off its precinct grid (that test without XRsiz, as there)
    auto prc_at = [&](uint32_t c, uint32_t r, uint64_t x, uint64_t y, uint32_t& pi) {
        if (!nprc(c, r)) return false;
        const Res& R = comps[c].res[r];
        const uint32_t lv = nres(c) - 1 - r;
        const uint64_t rpx = R.prcw_exp + lv, rpy = R.prch_exp + lv, sxc = p.sx(c), syc = p.sy(c);
        if (!((x % (sxc << rpx)) == 0 || (x == tx0 && (((uint64_t)R.x0 << lv) % (1ull << rpx)) != 0))) return false;
        if (!((y % (syc << rpy)) == 0 || (y == ty0 && (((uint64_t)R.y0 << lv) % (1ull << rpy)) != 0))) return false;
        const uint64_t i = (((x + (sxc << lv) - 1) / (sxc << lv)) >> R.prcw_exp) - (R.x0 >> R.prcw_exp);
        const uint64_t j = (((y + (syc << lv) - 1) / (syc << lv)) >> R.prch_exp) - (R.y0 >> R.prch_exp);
        if (i >= R.pw || j >= R.ph) return false;
        pi = (uint32_t)(i + j * R.pw);
        return true;
    };
    auto emit = [&](uint32_t c, uint32_t r, uint64_t x, uint64_t y) {
        uint32_t pi;
        if (!prc_at(c, r, x, y, pi)) return;
        for (uint32_t l = 0; l < nlayers; ++l) put(l, r, c, pi);
    };
    auto walk = [&](const std::function<void(uint64_t, uint64_t)>& f) {
        for (uint64_t y = ty0; y < ty1; y += dy - (y % dy))
            for (uint64_t x = tx0; x < tx1; x += dx - (x % dx)) f(x, y);
    };
    if (prog == 2) {          // RPCL
        for (uint32_t r = r0; r < r1; ++r)
            walk([&](uint64_t x, uint64_t y) { for (uint32_t c = c0; c < c1; ++c) emit(c, r, x, y); });
    } else if (prog == 3) {   // PCRL
        walk([&](uint64_t x, uint64_t y) {
            for (uint32_t c = c0; c < c1; ++c) for (uint32_t r = r0; r < r1; ++r) emit(c, r, x, y);
        });
    } else {                  // CPRL
        for (uint32_t c = c0; c < c1; ++c) {
            steps(c, c + 1);
            walk([&](uint64_t x, uint64_t y) { for (uint32_t r = r0; r < r1; ++r) emit(c, r, x, y); });
        }
    }
}

// The tile's packet sequence: its progression, or the POC entries' progressions in turn
// (layers clamped to the stream's, each packet once); entry (optional) receives, per packet,
// the index of the POC entry that emits it and its position in the entries' concatenated
// sequences, packets already written counted (Grok's final pass runs each entry's iterator
// afresh and skips a packet written before through the tile's packet tracker,
// T2Compress.cpp:46-54, 278-280, still counting it in tile->numProcessedPackets: SOP's Nsop).
static std::vector<PktRef> packet_iter(const std::vector<Comp>& comps, const Params& p, uint32_t tx0, uint32_t ty0,
                                       uint32_t tx1, uint32_t ty1, uint32_t nlayers,
                                       const std::vector<PocE>* pocs = nullptr, std::vector<uint32_t>* entry = nullptr) {
    std::vector<PktRef> v;
    const uint32_t nc = (uint32_t)comps.size();
    uint32_t nr = 0;
    for (const Comp& C : comps) nr = std::max<uint32_t>(nr, (uint32_t)C.res.size());
    std::vector<uint32_t> base(nc * nr + 1, 0);
    for (uint32_t c = 0, k = 0; c < nc; ++c)
        for (uint32_t r = 0; r < nr; ++r, ++k) {
            const bool has = r < comps[c].res.size();
            const Res* R = has ? &comps[c].res[r] : nullptr;
            base[k + 1] = base[k] + ((has && R->x1 > R->x0 && R->y1 > R->y0) ? R->pw * R->ph : 0u);
        }
    std::vector<uint8_t> seen((size_t)base[nc * nr] * nlayers + 1, 0);
    if (!pocs || pocs->empty()) {
        packet_iter_one(comps, p, p.prog, tx0, ty0, tx1, ty1, nlayers, nlayers, 0, nr, 0, nc, seen, base, v);
        return v;
    }
    uint32_t iter = 0;
    for (uint32_t ei = 0; ei < (uint32_t)pocs->size(); ++ei) {
        const PocE& e = (*pocs)[ei];
        const uint32_t le = std::min(e.lye, nlayers), r1 = std::min(e.re, nr), c1 = std::min(e.ce, nc);
        if (e.rs >= r1 || e.cs >= c1 || !le) continue;
        packet_iter_one(comps, p, e.prog, tx0, ty0, tx1, ty1, le, nlayers, e.rs, r1, e.cs, c1, seen, base, v, entry, ei,
                        &iter);
    }
    return v;
}

// Tile parts (CodeStreamCompress::getNumTilePartsForProgression, :1899-1958): the indices
// of the progression string up to the divider each open a new part; part count = product of
// their ranges (-1: unsupported divider, one behind P).
static int tile_parts(const Params& p, uint32_t nc) {
    if (!p.tp_div) return 1;
    static const char* names[5] = {"LRCP", "RLCP", "RPCL", "PCRL", "CPRL"};
    int n = 1;
    for (const char* q = names[p.prog]; *q; ++q) {
        if (*q == 'P') return -1;
        n *= *q == 'L' ? (int)p.nlayers : *q == 'R' ? (int)p.numres : (int)nc;
        if (*q == p.tp_div) return n;
    }
    return -1;
}
// With progression order changes each entry is a tile part of its own
// (CodeStreamCompress::writeTileParts :902-946: one part per progression when no divider
// is given, getNumTilePartsForProgression :1899-1958 returning 1 for each).
static int num_parts(const Params& p, uint32_t nc) {
    if (!p.pocs.empty()) return p.tp_div ? -1 : (int)p.pocs.size();
    return tile_parts(p, nc);
}
static uint32_t tile_part_of(const Params& p, uint32_t nc, const PktRef& k) {
    if (!p.tp_div) return 0;
    static const char* names[5] = {"LRCP", "RLCP", "RPCL", "PCRL", "CPRL"};
    uint32_t v = 0;
    for (const char* q = names[p.prog]; *q; ++q) {
        if (*q == 'L') v = v * p.nlayers + k.l;
        else if (*q == 'R') v = v * p.numres + k.r;
        else if (*q == 'C') v = v * nc + k.c;
        if (*q == p.tp_div) break;
    }
    return v;
}

struct PrecTrees { std::vector<TagTree> incl, imsb; };

// sop_eph: Scod's SOP (2) / EPH (4) bits; pkt: the packet's index in its tile (SOP's Nsop,
// tile->numProcessedPackets, T2Compress.cpp:286-320)
static bool write_packet(std::vector<uint8_t>* o, Res& R, uint32_t pi, uint32_t layno, PrecTrees& T,
                         uint64_t* budget, uint32_t sop_eph = 0, uint32_t pkt = 0, uint64_t* counted_bytes = nullptr,
                         std::vector<uint8_t>* ho = nullptr) {   // ho: the header (+ EPH) goes there (PPT / PPM)
    if (layno == 0) {
        for (size_t bi = 0; bi < R.bands.size(); ++bi) {
            Band& B = R.bands[bi]; Precinct& P = B.prcs[pi];
            if (B.empty() || P.cblks.empty()) continue;
            T.incl[bi].reset(); T.imsb[bi].reset();
            for (size_t k = 0; k < P.cblks.size(); ++k) {
                P.cblks[k].passes_in_prev = 0;
                T.imsb[bi].setvalue((uint32_t)k, B.numbps - P.cblks[k].numbps);
            }
        }
    }
    BitWriter bw; std::vector<uint8_t> hdr; bw.out = &hdr;
    std::vector<uint64_t> ops;
    if (budget) bw.ops = &ops;
    bw.write(1, 1);  // non-empty packet (Grok always writes 1)
    for (size_t bi = 0; bi < R.bands.size(); ++bi) {
        Band& B = R.bands[bi]; Precinct& P = B.prcs[pi];
        if (B.empty() || P.cblks.empty()) continue;
        for (size_t k = 0; k < P.cblks.size(); ++k) {
            Cblk& K = P.cblks[k];
            if (!K.passes_in_prev && K.layer_np[layno]) T.incl[bi].setvalue((uint32_t)k, layno);
        }
        for (size_t k = 0; k < P.cblks.size(); ++k) {
            Cblk& K = P.cblks[k];
            uint32_t np = K.layer_np[layno];
            if (!K.passes_in_prev) T.incl[bi].encode(bw, (uint32_t)k, layno + 1);
            else bw.write(np != 0, 1);
            if (!np) continue;
            if (!K.passes_in_prev) { K.numlenbits = 3; T.imsb[bi].encode(bw, (uint32_t)k, 0xffffffffu); }
            bw.numpasses(np);
            uint32_t first = K.passes_in_prev, last = first + np;
            int increment = 0; uint32_t len = 0, nump = 0;
            for (uint32_t q = first; q < last; ++q) {
                ++nump; len += K.passes[q].len;
                if (K.passes[q].term || q == last - 1) {
                    increment = std::max(increment, floorlog2(len) + 1 - ((int)K.numlenbits + floorlog2(nump)));
                    len = 0; nump = 0;
                }
            }
            bw.commacode((uint32_t)increment);
            K.numlenbits += (uint32_t)increment;
            for (uint32_t q = first; q < last; ++q) {
                ++nump; len += K.passes[q].len;
                if (K.passes[q].term || q == last - 1) {
                    bw.write(len, (int)K.numlenbits + floorlog2(nump));
                    len = 0; nump = 0;
                }
            }
        }
    }
    bw.flush();
    if (budget) {
        // compressPacketSimulate (T2Compress.cpp:347-434) in its own uint32 arithmetic: SOP's 6
        // and EPH's 2 bytes are taken without a test; the header's BitIO fails when its byte
        // count reaches the bytes left (BitIO::writeByte, BitIO.cpp:35-52), a test that never
        // fires when no byte is left (its count starts above 0), so a packet met with 0 bytes
        // left passes and the subtraction wraps: everything after it fits
        // (GrkSimBitIO: a budget reached inside a number-of-passes or comma code is not seen, the
        // header's count passes it and the subtraction wraps as well).  M is the packet's bytes
        // left, decremented unless it is UINT_MAX; *budget (compressPacketsSimulate's maxBytes)
        // takes the packet's counted bytes at the end, under the same guard.
        uint32_t M = (uint32_t)*budget;
        if (sop_eph & 2) { if (M != 0xffffffffu) M -= 6; }
        uint64_t nb = 0;
        if (!grk_sim_header(ops, M, &nb)) return false;
        if (M != 0xffffffffu) M -= (uint32_t)nb;
        if (sop_eph & 4) { if (M != 0xffffffffu) M -= 2; }
        uint64_t counted = ((sop_eph & 2) ? 6 : 0) + nb + ((sop_eph & 4) ? 2 : 0);
        for (size_t bi = 0; bi < R.bands.size(); ++bi) {
            Band& B = R.bands[bi]; Precinct& P = B.prcs[pi];
            if (B.empty() || P.cblks.empty()) continue;
            for (auto& K : P.cblks) {
                const uint32_t np = K.layer_np[layno];
                if (!np) continue;
                const uint32_t r0 = K.passes_in_prev ? K.passes[K.passes_in_prev - 1].rate : 0;
                const uint32_t len = K.passes[K.passes_in_prev + np - 1].rate - r0;
                if (len > M) return false;
                if (M != 0xffffffffu) M -= len;
                counted += len;
            }
        }
        if (*budget != 0xffffffffu) *budget = (uint32_t)(*budget - counted);
        if (counted_bytes) *counted_bytes = counted;
    }
    if (o) {
        if (sop_eph & 2) {   // SOP: FF91, Lsop 4, Nsop = packet index mod 2^16
            put16(*o, 0xff91); put16(*o, 4); put16(*o, pkt & 0xffff);
        }
        std::vector<uint8_t>& hd = ho ? *ho : *o;
        hd.insert(hd.end(), hdr.begin(), hdr.end());
        if (sop_eph & 4) put16(hd, 0xff92);   // EPH
    }
    for (size_t bi = 0; bi < R.bands.size(); ++bi) {   // packet body
        Band& B = R.bands[bi]; Precinct& P = B.prcs[pi];
        if (B.empty() || P.cblks.empty()) continue;
        for (auto& K : P.cblks) {
            uint32_t np = K.layer_np[layno];
            if (!np) continue;
            uint32_t r0 = K.passes_in_prev ? K.passes[K.passes_in_prev - 1].rate : 0;
            uint32_t r1 = K.passes[K.passes_in_prev + np - 1].rate;
            if (o) o->insert(o->end(), K.data.begin() + r0, K.data.begin() + r1);
            K.passes_in_prev += np;
        }
    }
    return true;
}


// ----------------------------------------------------------------------------
// HTJ2K block coder, cleanup pass only (ISO/IEC 15444-15; Grok calls OpenJPH
// 0.7.2: ojph_encode_codeblock ojph_block_encoder.cpp:470-947, decode
// ojph_block_decoder.cpp:989-1700).  Restated from the standard's structure:
// quads of 2x2 samples scanned in pairs along 2-row stripes; per quad the
// significance pattern rho and the EMB pattern are CxtVLC coded (backward VLC
// segment), the exponent offsets u_q are U-VLC coded (same segment), zero
// contexts use the adaptive MEL run coder, magnitudes/signs go to the forward
// MagSgn segment.  The segment layout and termination follow OpenJPH so the
// bytes are identical to Grok's.
// ----------------------------------------------------------------------------
#include "ht_tables.h"

static const int MEL_EXP[13] = {0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 4, 5};

struct HtMelEnc {
    std::vector<uint8_t> b; int rem = 8, tmp = 0, run = 0, k = 0, thr = 1;
    void bit(int v) {
        tmp = (tmp << 1) + v;
        if (--rem == 0) { b.push_back((uint8_t)tmp); rem = (tmp == 0xFF) ? 7 : 8; tmp = 0; }
    }
    void code(bool e) {
        if (!e) {
            if (++run >= thr) { bit(1); run = 0; k = std::min(12, k + 1); thr = 1 << MEL_EXP[k]; }
        } else {
            bit(0);
            for (int t = MEL_EXP[k]; t > 0;) bit((run >> --t) & 1);
            run = 0; k = std::max(0, k - 1); thr = 1 << MEL_EXP[k];
        }
    }
};
struct HtVlcEnc {   // grows backward; b holds bytes in emission order
    std::vector<uint8_t> b; int used = 4, tmp = 0xF; bool gt8f = true;
    void code(int cwd, int len) {
        while (len > 0) {
            int avail = 8 - (gt8f ? 1 : 0) - used;
            int t = std::min(avail, len);
            tmp |= (cwd & ((1 << t) - 1)) << used;
            used += t; avail -= t; len -= t; cwd >>= t;
            if (avail == 0) {
                if (gt8f && tmp != 0x7F) { gt8f = false; continue; }
                b.push_back((uint8_t)tmp); gt8f = tmp > 0x8F; tmp = 0; used = 0;
            }
        }
    }
};
struct HtMsEnc {
    std::vector<uint8_t> b; int maxb = 8, used = 0; uint32_t tmp = 0;
    void code(uint32_t cwd, int len) {
        while (len > 0) {
            int t = std::min(maxb - used, len);
            tmp |= (cwd & ((1u << t) - 1)) << used;
            used += t; cwd >>= t; len -= t;
            if (used >= maxb) { b.push_back((uint8_t)tmp); maxb = (tmp == 0xFF) ? 7 : 8; tmp = 0; used = 0; }
        }
    }
    void terminate() {
        if (used) {
            int t = maxb - used;
            tmp |= (0xFFu & ((1u << t) - 1)) << used;
            if (tmp != 0xFF) b.push_back((uint8_t)tmp);
        } else if (maxb == 7) b.pop_back();
    }
};
// U-VLC prefix/suffix codes for u in 0..32 (Annex C, OpenJPH uvlc tables)
static void uvlc_code(int u, int& pre, int& pre_len, int& suf, int& suf_len) {
    static const int P[5] = {0, 1, 2, 4, 4}, PL[5] = {0, 1, 2, 3, 3}, S[5] = {0, 0, 0, 0, 1}, SL[5] = {0, 0, 0, 1, 1};
    if (u < 5) { pre = P[u]; pre_len = PL[u]; suf = S[u]; suf_len = SL[u]; }
    else { pre = 0; pre_len = 3; suf = u - 5; suf_len = 5; }
}

// coef: signed integer coefficients (HT reversible: the full magnitude is coded)
static std::vector<uint8_t> ht_encode_block(const int32_t* coef, uint32_t w, uint32_t h, uint32_t stride) {
    HtMelEnc mel; HtVlcEnc vlc; HtMsEnc ms;
    std::vector<uint8_t> e_val(w / 2 + 4, 0), cx_val(w / 2 + 4, 0);
    auto sample = [&](uint32_t x, uint32_t y, int& rho, int bit, int& e, uint32_t& sv, int& emax) {
        if (x >= w || y >= h) return;
        int32_t v = coef[(size_t)y * stride + x];
        uint32_t mu = (uint32_t)(v < 0 ? -v : v);
        if (!mu) return;
        rho |= bit;
        e = 32 - __builtin_clz(2 * mu - 1);
        emax = std::max(emax, e);
        sv = 2 * mu - 2 + (v < 0 ? 1u : 0u);
    };
    auto uvlc = [&](int u) { int a, b, c, d; uvlc_code(u, a, b, c, d); vlc.code(a, b); };
    auto uvlc_suf = [&](int u) { int a, b, c, d; uvlc_code(u, a, b, c, d); vlc.code(c, d); };
    auto ms_quad = [&](int rho, int Uq, uint16_t tup, const uint32_t* sv) {
        for (int n = 0; n < 4; ++n) {
            int m = (rho >> n & 1) ? Uq - ((tup >> n) & 1) : 0;
            ms.code(sv[n] & ((1u << m) - 1), m);
        }
    };
    int c_q0 = 0;
    for (uint32_t y = 0; y < h; y += 2) {
        const bool first = y == 0;
        const uint16_t* tbl = first ? HT_VLC_ENC0 : HT_VLC_ENC1;
        int max_e = 0;
        if (!first) { max_e = std::max(e_val[0], e_val[1]) - 1; e_val[0] = 0; c_q0 = cx_val[0] + (cx_val[1] << 2); cx_val[0] = 0; }
        else { e_val[0] = 0; cx_val[0] = 0; }
        size_t li = 0;   // line-state index (one entry per column pair)
        for (uint32_t x = 0; x < w; x += 4) {
            int rho[2] = {0, 0}, emax[2] = {0, 0}, e[8] = {0}; uint32_t sv[8] = {0};
            sample(x, y, rho[0], 1, e[0], sv[0], emax[0]);
            sample(x, y + 1, rho[0], 2, e[1], sv[1], emax[0]);
            sample(x + 1, y, rho[0], 4, e[2], sv[2], emax[0]);
            sample(x + 1, y + 1, rho[0], 8, e[3], sv[3], emax[0]);
            int kappa0 = first ? 1 : ((rho[0] & (rho[0] - 1)) ? std::max(1, max_e) : 1);
            int Uq0 = std::max(emax[0], kappa0), u0 = Uq0 - kappa0, u1 = 0;
            int eps0 = 0;
            if (u0 > 0) for (int n = 0; n < 4; ++n) eps0 |= (e[n] == emax[0]) << n;
            e_val[li] = (uint8_t)std::max<int>(e_val[li], e[1]); ++li;
            if (!first) max_e = std::max(e_val[li], e_val[li + 1]) - 1;
            e_val[li] = (uint8_t)e[3];
            cx_val[li - 1] = (uint8_t)(cx_val[li - 1] | ((rho[0] & 2) >> 1));
            int c_q1 = first ? 0 : cx_val[li] + (cx_val[li + 1] << 2);
            cx_val[li] = (uint8_t)((rho[0] & 8) >> 3);
            uint16_t t0 = tbl[(c_q0 << 8) + (rho[0] << 4) + eps0];
            vlc.code(t0 >> 8, (t0 >> 4) & 7);
            if (c_q0 == 0) mel.code(rho[0] != 0);
            ms_quad(rho[0], Uq0, t0, sv);
            if (x + 2 < w) {
                sample(x + 2, y, rho[1], 1, e[4], sv[4], emax[1]);
                sample(x + 2, y + 1, rho[1], 2, e[5], sv[5], emax[1]);
                sample(x + 3, y, rho[1], 4, e[6], sv[6], emax[1]);
                sample(x + 3, y + 1, rho[1], 8, e[7], sv[7], emax[1]);
                int kappa1 = first ? 1 : ((rho[1] & (rho[1] - 1)) ? std::max(1, max_e) : 1);
                if (first) c_q1 = (rho[0] >> 1) | (rho[0] & 1);
                else c_q1 |= ((rho[0] & 4) >> 1) | ((rho[0] & 8) >> 2);
                int Uq1 = std::max(emax[1], kappa1);
                u1 = Uq1 - kappa1;
                int eps1 = 0;
                if (u1 > 0) for (int n = 0; n < 4; ++n) eps1 |= (e[4 + n] == emax[1]) << n;
                e_val[li] = (uint8_t)std::max<int>(e_val[li], e[5]); ++li;
                if (!first) max_e = std::max(e_val[li], e_val[li + 1]) - 1;
                e_val[li] = (uint8_t)e[7];
                cx_val[li - 1] = (uint8_t)(cx_val[li - 1] | ((rho[1] & 2) >> 1));
                if (!first) c_q0 = cx_val[li] + (cx_val[li + 1] << 2);
                cx_val[li] = (uint8_t)((rho[1] & 8) >> 3);
                uint16_t t1 = tbl[(c_q1 << 8) + (rho[1] << 4) + eps1];
                vlc.code(t1 >> 8, (t1 >> 4) & 7);
                if (c_q1 == 0) mel.code(rho[1] != 0);
                ms_quad(rho[1], Uq1, t1, sv + 4);
            }
            if (first) {
                if (u0 > 0 && u1 > 0) mel.code(std::min(u0, u1) > 2);
                if (u0 > 2 && u1 > 2) { uvlc(u0 - 2); uvlc(u1 - 2); uvlc_suf(u0 - 2); uvlc_suf(u1 - 2); }
                else if (u0 > 2 && u1 > 0) { uvlc(u0); vlc.code(u1 - 1, 1); uvlc_suf(u0); }
                else { uvlc(u0); uvlc(u1); uvlc_suf(u0); uvlc_suf(u1); }
                c_q0 = (rho[1] >> 1) | (rho[1] & 1);
            } else {
                uvlc(u0); uvlc(u1); uvlc_suf(u0); uvlc_suf(u1);
                c_q0 |= ((rho[1] & 4) >> 1) | ((rho[1] & 8) >> 2);
            }
        }
        if (first) e_val[li + 1] = 0;
    }
    // termination of MEL + VLC (terminate_mel_vlc) and MagSgn
    if (mel.run > 0) mel.bit(1);
    mel.tmp = mel.tmp << mel.rem;
    int mel_mask = (0xFF << mel.rem) & 0xFF, vlc_mask = 0xFF >> (8 - vlc.used);
    if ((mel_mask | vlc_mask) != 0) {
        int fuse = mel.tmp | vlc.tmp;
        if ((((fuse ^ mel.tmp) & mel_mask) | ((fuse ^ vlc.tmp) & vlc_mask)) == 0 && fuse != 0xFF && !vlc.b.empty())
            mel.b.push_back((uint8_t)fuse);
        else { mel.b.push_back((uint8_t)mel.tmp); vlc.b.push_back((uint8_t)vlc.tmp); }
    }
    ms.terminate();
    std::vector<uint8_t> out(ms.b);
    out.insert(out.end(), mel.b.begin(), mel.b.end());
    for (size_t i = vlc.b.size(); i > 0; --i) out.push_back(vlc.b[i - 1]);
    out.push_back(0xFF);
    uint32_t scup = (uint32_t)(mel.b.size() + vlc.b.size() + 1);
    size_t L = out.size();
    out[L - 1] = (uint8_t)(scup >> 4);
    out[L - 2] = (uint8_t)((out[L - 2] & 0xF0) | (scup & 0xF));
    return out;
}

// HT cleanup-pass decoder (mirror of ht_encode_block; ISO/IEC 15444-15
// clause 7; Grok: T1HT::decompress T1HT.cpp:134-187 -> ojph_decode_codeblock).
// Writes signed coefficients.  Returns false on a malformed segment.
struct HtMelDec {   // forward, MSB first, bit-unstuffing after 0xFF
    const uint8_t* p; uint32_t n, pos = 0; int bits = 0; uint32_t cur = 0; bool ff = false;
    int k = 0, run = 0; bool pending_one = false;
    int bit() {
        if (bits == 0) {
            uint32_t b = pos < n ? p[pos] : 0xFF; ++pos;
            bits = ff ? 7 : 8; cur = b & ((1u << bits) - 1); ff = b == 0xFF;
        }
        --bits; return (cur >> bits) & 1;
    }
    int event() {   // next MEL symbol (0 = no significance / "min(u) <= 2")
        if (run > 0) { --run; return 0; }
        if (pending_one) { pending_one = false; return 1; }
        for (;;) {
            if (bit()) {   // a full run of 2^e zeros
                int r = 1 << MEL_EXP[k]; k = std::min(12, k + 1);
                run = r - 1; return 0;
            }
            int e = MEL_EXP[k], r = 0;
            for (int t = 0; t < e; ++t) r = (r << 1) | bit();
            k = std::max(0, k - 1);
            if (r == 0) return 1;
            run = r - 1; pending_one = true; return 0;
        }
    }
};
struct HtVlcDec {   // backward from the end of the Scup region, LSB first
    const uint8_t* p; int pos; uint64_t acc = 0; int nb = 0; bool gt8f;
    void init(const uint8_t* base, uint32_t lcup) {
        p = base; pos = (int)lcup - 2;
        uint8_t d = base[lcup - 2];
        int t = d >> 4;
        int n = ((t & 7) == 7) ? 3 : 4;
        acc = (uint64_t)(t & ((1 << n) - 1)); nb = n; gt8f = d > 0x8F;
        --pos;
    }
    void fill() {
        while (nb <= 56) {
            uint8_t d = pos >= 0 ? p[pos] : 0; --pos;
            int n = (gt8f && (d & 0x7F) == 0x7F) ? 7 : 8;
            acc |= (uint64_t)(d & ((1 << n) - 1)) << nb; nb += n; gt8f = d > 0x8F;
        }
    }
    uint32_t peek(int n) { fill(); return (uint32_t)(acc & ((1ull << n) - 1)); }
    void skip(int n) { acc >>= n; nb -= n; }
    uint32_t get(int n) { uint32_t v = peek(n); skip(n); return v; }
};
struct HtMsDec {    // forward, LSB first, unstuffing after 0xFF, 0xFF beyond the end
    const uint8_t* p; uint32_t n, pos = 0; uint64_t acc = 0; int nb = 0; bool ff = false;
    uint32_t get(int m) {
        while (nb < m) {
            uint8_t d = pos < n ? p[pos] : 0xFF; ++pos;
            int k = ff ? 7 : 8;
            acc |= (uint64_t)(d & ((1 << k) - 1)) << nb; nb += k; ff = d == 0xFF;
        }
        uint32_t v = (uint32_t)(acc & ((1ull << m) - 1)); acc >>= m; nb -= m; return v;
    }
};
static int uvlc_decode_prefix(HtVlcDec& v) {   // returns 1,2,3(→3|4),5(→5+)
    if (v.get(1)) return 1;
    if (v.get(1)) return 2;
    return v.get(1) ? 3 : 5;
}
static int uvlc_decode_suffix(HtVlcDec& v, int pre) {
    if (pre == 3) return 3 + (int)v.get(1);
    if (pre == 5) return 5 + (int)v.get(5);
    return pre;
}

static bool ht_decode_block(const uint8_t* d, uint32_t lcup, uint32_t w, uint32_t h, uint32_t k_msbs,
                            int32_t* out, uint32_t stride) {
    for (uint32_t y = 0; y < h; ++y) for (uint32_t x = 0; x < w; ++x) out[(size_t)y * stride + x] = 0;
    if (lcup < 2) return lcup == 0;
    uint32_t scup = ((uint32_t)d[lcup - 1] << 4) | (d[lcup - 2] & 0xF);
    if (scup < 2 || scup > lcup || scup > 4079) return false;
    uint32_t pcup = lcup - scup;
    HtMelDec mel; mel.p = d + pcup; mel.n = scup;
    HtVlcDec vlc; vlc.init(d, lcup);
    HtMsDec ms; ms.p = d; ms.n = pcup;
    const int umax = (int)k_msbs + 2;
    std::vector<uint8_t> e_val(w / 2 + 4, 0), cx_val(w / 2 + 4, 0);
    auto emit = [&](uint32_t x, uint32_t y, int rho, int bit, int Uq, int ek, int e1, int& e) -> bool {
        e = 0;
        if (!(rho & bit)) return true;
        int m = Uq - ((ek & bit) ? 1 : 0);
        if (m < 0 || m > 31) return false;
        uint32_t v = ms.get(m) | ((uint32_t)((e1 & bit) ? 1 : 0) << m);
        uint32_t mu = (v >> 1) + 1;
        e = 32 - __builtin_clz(2 * mu - 1);
        if (x < w && y < h) out[(size_t)y * stride + x] = (v & 1) ? -(int32_t)mu : (int32_t)mu;
        return true;
    };
    int c_q0 = 0;
    for (uint32_t y = 0; y < h; y += 2) {
        const bool first = y == 0;
        const uint16_t* tbl = first ? HT_VLC_DEC0 : HT_VLC_DEC1;
        int max_e = 0;
        if (!first) { max_e = std::max(e_val[0], e_val[1]) - 1; e_val[0] = 0; c_q0 = cx_val[0] + (cx_val[1] << 2); cx_val[0] = 0; }
        else { e_val[0] = 0; cx_val[0] = 0; }
        size_t li = 0;
        for (uint32_t x = 0; x < w; x += 4) {
            int rho[2] = {0, 0}, uoff[2] = {0, 0}, ek[2] = {0, 0}, e1[2] = {0, 0}, u[2] = {0, 0};
            const bool two = x + 2 < w;
            // quad 0 significance + EMB
            auto decode_quad = [&](int cq, int j) {
                if (cq == 0 && !mel.event()) return;   // insignificant quad, no codeword
                uint16_t t = tbl[(cq << 7) | vlc.peek(7)];
                vlc.skip(t & 7);
                rho[j] = (t >> 4) & 15; uoff[j] = (t >> 3) & 1; e1[j] = (t >> 8) & 15; ek[j] = (t >> 12) & 15;
            };
            decode_quad(c_q0, 0);
            int c_q1 = 0;
            if (!first) {
                // context of quad 1 depends only on the previous row and on quad 0
                c_q1 = cx_val[li + 1] + (cx_val[li + 2] << 2);
            }
            // the encoder updates the line state after each quad; replay that order
            int e_q[8] = {0};
            auto finish_row_state0 = [&]() {};
            (void)finish_row_state0;
            if (two) {
                if (first) c_q1 = (rho[0] >> 1) | (rho[0] & 1);
                else c_q1 |= ((rho[0] & 4) >> 1) | ((rho[0] & 8) >> 2);
                decode_quad(c_q1, 1);
            }
            // U-VLC exponent offsets (clause 7.3.6)
            if (first && uoff[0] && uoff[1]) {
                if (mel.event()) {
                    int p0 = uvlc_decode_prefix(vlc), p1 = uvlc_decode_prefix(vlc);
                    u[0] = uvlc_decode_suffix(vlc, p0) + 2; u[1] = uvlc_decode_suffix(vlc, p1) + 2;
                } else {
                    int p0 = uvlc_decode_prefix(vlc);
                    if (p0 > 2) { u[1] = (int)vlc.get(1) + 1; u[0] = uvlc_decode_suffix(vlc, p0); }
                    else { int p1 = uvlc_decode_prefix(vlc); u[0] = uvlc_decode_suffix(vlc, p0); u[1] = uvlc_decode_suffix(vlc, p1); }
                }
            } else {
                int p0 = uoff[0] ? uvlc_decode_prefix(vlc) : 0, p1 = uoff[1] ? uvlc_decode_prefix(vlc) : 0;
                u[0] = uoff[0] ? uvlc_decode_suffix(vlc, p0) : 0; u[1] = uoff[1] ? uvlc_decode_suffix(vlc, p1) : 0;
            }
            // quad 0 magnitudes/signs, then line state, as the encoder orders them
            int kappa0 = first ? 1 : ((rho[0] & (rho[0] - 1)) ? std::max(1, max_e) : 1);
            int Uq0 = kappa0 + u[0];
            if (Uq0 > umax && rho[0]) return false;
            if (!emit(x, y, rho[0], 1, Uq0, ek[0], e1[0], e_q[0]) || !emit(x, y + 1, rho[0], 2, Uq0, ek[0], e1[0], e_q[1]) ||
                !emit(x + 1, y, rho[0], 4, Uq0, ek[0], e1[0], e_q[2]) || !emit(x + 1, y + 1, rho[0], 8, Uq0, ek[0], e1[0], e_q[3]))
                return false;
            e_val[li] = (uint8_t)std::max<int>(e_val[li], e_q[1]); ++li;
            if (!first) max_e = std::max(e_val[li], e_val[li + 1]) - 1;
            e_val[li] = (uint8_t)e_q[3];
            cx_val[li - 1] = (uint8_t)(cx_val[li - 1] | ((rho[0] & 2) >> 1));
            cx_val[li] = (uint8_t)((rho[0] & 8) >> 3);
            if (two) {
                int kappa1 = first ? 1 : ((rho[1] & (rho[1] - 1)) ? std::max(1, max_e) : 1);
                int Uq1 = kappa1 + u[1];
                if (Uq1 > umax && rho[1]) return false;
                if (!emit(x + 2, y, rho[1], 1, Uq1, ek[1], e1[1], e_q[4]) || !emit(x + 2, y + 1, rho[1], 2, Uq1, ek[1], e1[1], e_q[5]) ||
                    !emit(x + 3, y, rho[1], 4, Uq1, ek[1], e1[1], e_q[6]) || !emit(x + 3, y + 1, rho[1], 8, Uq1, ek[1], e1[1], e_q[7]))
                    return false;
                e_val[li] = (uint8_t)std::max<int>(e_val[li], e_q[5]); ++li;
                if (!first) max_e = std::max(e_val[li], e_val[li + 1]) - 1;
                e_val[li] = (uint8_t)e_q[7];
                cx_val[li - 1] = (uint8_t)(cx_val[li - 1] | ((rho[1] & 2) >> 1));
                if (!first) c_q0 = cx_val[li] + (cx_val[li + 1] << 2);
                cx_val[li] = (uint8_t)((rho[1] & 8) >> 3);
            }
            if (first) c_q0 = (rho[1] >> 1) | (rho[1] & 1);
            else c_q0 |= ((rho[1] & 4) >> 1) | ((rho[1] & 8) >> 2);
        }
        if (first) e_val[li + 1] = 0;
    }
    return true;
}

}  // namespace orc

using namespace orc;

// ============================================================================
// C ABI for the tests (ctypes)
// ============================================================================
extern "C" {

typedef struct {
    uint32_t numres, cbw_exp, cbh_exp, irreversible, mct, nlayers, write_com;
    uint32_t prcw_exp[33], prch_exp[33];
    double layer_rate[100];
    uint32_t cblk_sty;
    uint32_t tile_w, tile_h, tlm, plt;
    uint32_t cod_format;   // 0 = raw codestream (GRK_CODEC_J2K), 2 = JP2 file (GRK_CODEC_JP2)
    uint32_t prog_order;   // GRK_PROG_ORDER
    uint32_t tp_div;       // tile-part divider character ('L', 'R', 'C') or 0
    uint32_t numpocs;      // progression order changes: pocs[i] = resS, compS, layE, resE, compE, prog
    uint32_t pocs[32][6];
    int32_t roi_compno;    // grk_cparameters::roi_compno (-1 none) / roi_shift
    uint32_t roi_shift;
    uint32_t csty;         // grk_cparameters::csty SOP (2) / EPH (4) bits (the precinct bit follows prcw_exp)
    uint32_t by_quality;   // grk_cparameters::allocationByQuality: layer_distortion holds PSNR targets
    double layer_distortion[100];
    uint32_t image_x0, image_y0;   // canvas offset of the image area (grk_image::x0 / y0, -d)
    uint32_t tile_x0, tile_y0;     // tile grid origin (grk_cparameters::tx0 / ty0, -T)
    // per-component quantisation (QCC; Params::comp_gb / comp_qshift / qderived), first nq components
    uint32_t nq;
    uint32_t comp_gb[16];
    int32_t comp_qshift[16];
    uint32_t qderived;
    // component subsampling (grk_image_comp::dx / dy), first nsub components (others 1)
    uint32_t nsub;
    uint32_t sub_dx[16], sub_dy[16];
    uint32_t ppx;          // packed packet headers: 1 PPT, 2 PPM (Params::ppx)
    // caller comments: ncom entries, bytes back to back at com_data
    uint32_t ncom;
    const uint8_t* com_data;
    uint32_t com_len[16], com_binary[16];
} orc_cparams;

void orc_set_threads(unsigned n) { g_threads = n ? n : 1; }
void orc_set_decode_layers(uint32_t n) { g_dec_layers = n; }
void orc_set_decode_reduce(uint32_t n) { g_dec_reduce = n; }
unsigned orc_get_threads(void) { return g_threads; }

static Params to_params(const orc_cparams* cp) {
    Params p;
    if (!cp) return p;
    p.numres = cp->numres; p.cbw_exp = cp->cbw_exp; p.cbh_exp = cp->cbh_exp;
    p.irreversible = cp->irreversible; p.mct = cp->mct; p.nlayers = cp->nlayers ? cp->nlayers : 1;
    p.write_com = (int)cp->write_com;
    p.cblk_sty = cp->cblk_sty;
    p.prog = cp->prog_order;
    p.tp_div = (char)cp->tp_div;
    if (cp->roi_compno >= 0 && cp->roi_shift) {
        p.roishift.assign((size_t)cp->roi_compno + 1, 0);
        p.roishift[(size_t)cp->roi_compno] = cp->roi_shift;
    }
    for (uint32_t i = 0; i < cp->numpocs && i < 32; ++i)
        p.pocs.push_back({cp->pocs[i][0], cp->pocs[i][1], cp->pocs[i][2], cp->pocs[i][3], cp->pocs[i][4], cp->pocs[i][5]});
    if (p.ht()) p.numgbits = 1;   // grk_compress.cpp:1123-1124
    p.tw = cp->tile_w; p.th = cp->tile_h; p.tlm = (int)cp->tlm; p.plt = (int)cp->plt;
    p.x0 = cp->image_x0; p.y0 = cp->image_y0; p.gx0 = cp->tile_x0; p.gy0 = cp->tile_y0;
    p.sop_eph = cp->csty & 6;
    p.quality = cp->by_quality != 0;
    // CodeStreamCompress.cpp:387-393: a tile takes the PSNR targets under allocationByQuality,
    // the compression ratios otherwise
    for (uint32_t i = 0; i < 100; ++i) p.rates[i] = (i < p.nlayers && !p.quality) ? cp->layer_rate[i] : 0.0;
    for (uint32_t i = 0; i < 100; ++i) p.dist[i] = (i < p.nlayers && p.quality) ? cp->layer_distortion[i] : 0.0;
    // exponents as given: 15 (orc_default_params) is the default 2^15 partition, 0 is a legal
    // exponent at resolution 0 (CodeStreamCompress.cpp:573-590 writes it when the halved size
    // reaches 1); at a higher resolution it has no band partition (B.6 PPx - 1) and is refused
    for (int i = 0; i < 33; ++i) { p.prcw_exp[i] = cp->prcw_exp[i] & 15; p.prch_exp[i] = cp->prch_exp[i] & 15; }
    for (uint32_t c = 0; c < cp->nq && c < 16; ++c) { p.comp_gb.push_back(cp->comp_gb[c]); p.comp_qshift.push_back(cp->comp_qshift[c]); }
    p.qderived = cp->qderived != 0;
    for (uint32_t c = 0; c < cp->nsub && c < 16; ++c) { p.cdx.push_back(std::max(1u, cp->sub_dx[c])); p.cdy.push_back(std::max(1u, cp->sub_dy[c])); }
    p.ppx = cp->ppx;
    for (uint32_t i = 0, at = 0; i < cp->ncom && i < 16; at += cp->com_len[i], ++i)
        p.comments.push_back({cp->com_binary[i] ? 0u : 1u, std::string((const char*)cp->com_data + at, cp->com_len[i])});
    return p;
}

void orc_default_params(orc_cparams* cp) {
    memset(cp, 0, sizeof(*cp));
    cp->numres = 6; cp->cbw_exp = 6; cp->cbh_exp = 6; cp->irreversible = 0; cp->mct = 1; cp->nlayers = 1; cp->write_com = 1;
    for (int i = 0; i < 33; ++i) { cp->prcw_exp[i] = 15; cp->prch_exp[i] = 15; }
}

// Per-block record exported for parity checks (canonical order: comp, res, band, precinct, cblk).
typedef struct {
    uint32_t comp, res, band, prc, cblk;
    uint32_t x0, y0, x1, y1;
    uint32_t numbps, npasses, len;
    uint64_t data_off;
} orc_block;

struct EncodeState {
    Image im; Params p;
    uint32_t tile = 0, tx0 = 0, ty0 = 0, tx1 = 0, ty1 = 0;   // tile index and rectangle
    std::vector<Comp> comps;
    std::vector<std::vector<int32_t>> coefs;   // reversible Mallat coefficients
    std::vector<std::vector<float>> fcoefs;    // irreversible Mallat coefficients
    size_t header_size = 0;
    // the rate control's final simulation (pcrdBisectSimple :1352-1357): each packet's length as
    // compressPacketSimulate counts it, in the tile's progression; they fill the PLT marker
    // (pushNextPacketLength) and their sum the tile-part length written in SOT / TLM
    // (preCalculatedTileLen, TileProcessor.cpp:243-259) - not always the bytes written, see
    // GrkSimBitIO
    std::vector<uint32_t> sim_lens;
    bool have_sim = false;
    std::vector<uint8_t> pkt_headers;   // PPT / PPM: the tile's packet headers in packet order
};

// Rate control is active when any layer has a target rate (TileProcessor.cpp:952-967).
static bool layer_needs_rc(const Params& p, uint32_t l) {   // TileProcessor::layerNeedsRateControl (:952-957)
    return p.quality ? p.dist[l] > 0.0 : p.rates[l] > 0.0;
}
static bool needs_rate_control(const Params& p) {
    for (uint32_t l = 0; l < p.nlayers; ++l) if (layer_needs_rc(p, l)) return true;
    return false;
}

static void t1_encode_all(EncodeState& E) {
    const bool rc = needs_rate_control(E.p);
    static const double norms_irrev[3] = {1.732, 1.805, 1.573};   // mct.cpp:689-704
    static const double norms_rev[3] = {1.732, .8292, .8292};
    const bool mct = E.p.mct && E.im.nc >= 3;
    struct Job { uint32_t c, r; Band* B; Cblk* K; };
    std::vector<Job> jobs;
    for (uint32_t c = 0; c < E.im.nc; ++c)
        for (uint32_t r = 0; r < E.p.numres; ++r)
            for (auto& B : E.comps[c].res[r].bands)
                for (auto& P : B.prcs)
                    for (auto& K : P.cblks) jobs.push_back({c, r, &B, &K});
    par_for(jobs.size(), [&](size_t ji) {
                        const uint32_t c = jobs[ji].c, r = jobs[ji].r;
                        Comp& C = E.comps[c];
                        Band& B = *jobs[ji].B;
                        Cblk& K = *jobs[ji].K;
                        uint32_t w = K.x1 - K.x0, h = K.y1 - K.y0;
                        if (E.p.ht()) {   // T1HT::compress (T1HT.cpp:109-133): one cleanup pass
                            const size_t o0 = (size_t)(B.offy + K.y0 - B.y0) * C.w + (B.offx + K.x0 - B.x0);
                            // ROI maxshift (standard-correct, the component is the region: every
                            // index magnitude scaled up by 2^shift, the band's bit-plane count raised
                            // by it; Grok refuses nothing but its encoder only raises the count,
                            // CodeStreamCompress.cpp:538-541)
                            const uint32_t rs = E.p.roi(c);
                            auto roi_up = [&](int32_t v) { return rs ? (v < 0 ? -(int32_t)((uint32_t)-v << rs) : (int32_t)((uint32_t)v << rs)) : v; };
                            if (E.p.irreversible || rs) {
                                // T1HT::preCompress irreversible branch (T1HT.cpp:88-104) on the 9/7
                                // coefficients as floats (R-BUG-2: Grok reads the float bits as
                                // int32): index = trunc(x * (1 / stepsize))
                                const float inv = E.p.irreversible ? 1.0f / B.stepsize : 0.0f;
                                std::vector<int32_t> q((size_t)w * h);
                                for (uint32_t y = 0; y < h; ++y)
                                    for (uint32_t x = 0; x < w; ++x) {
                                        const size_t o = o0 + (size_t)y * C.w + x;
                                        q[(size_t)y * w + x] = roi_up(E.p.irreversible ? (int32_t)(E.fcoefs[c][o] * inv) : E.coefs[c][o]);
                                    }
                                K.data = ht_encode_block(q.data(), w, h, w);
                            } else
                            K.data = ht_encode_block(E.coefs[c].data() + o0, w, h, C.w);
                            uint32_t L = (uint32_t)K.data.size();
                            K.numbps = 1; K.npasses = 1; K.passes.assign(1, PassInfo{L, L, 1, 0.0});
                            return;
                        }
                        std::vector<uint32_t> mag(w * h); std::vector<uint8_t> neg(w * h);
                        for (uint32_t y = 0; y < h; ++y)
                            for (uint32_t x = 0; x < w; ++x) {
                                size_t o = (size_t)(B.offy + K.y0 - B.y0 + y) * C.w + (B.offx + K.x0 - B.x0 + x);
                                int64_t sv;
                                if (!E.p.irreversible) sv = (int64_t)E.coefs[c][o] * (1 << FRACBITS);
                                else {   // T1Part1::preCompress (T1Part1.cpp:70-86)
                                    float q = (E.fcoefs[c][o] / B.stepsize) * (float)(1 << FRACBITS);
                                    sv = (int64_t)lrintf(q);
                                }
                                // ROI maxshift (standard-correct: the whole component is the region,
                                // the integer part of its indices scaled up by 2^shift, the six
                                // fractional distortion bits kept below; Grok's encoder only raises
                                // the band bit-plane count, CodeStreamCompress.cpp:538-541)
                                const uint64_t a0 = (uint64_t)(sv < 0 ? -sv : sv);
                                const uint64_t a1 = ((a0 >> FRACBITS) << (FRACBITS + E.p.roi(c))) | (a0 & 63u);
                                neg[y * w + x] = sv < 0;
                                mag[y * w + x] = (uint32_t)a1;
                            }
                        DistCtx dc{c, E.p.numres - 1 - r, B.orient, E.p.irreversible ? 0u : 1u, (double)B.stepsize,
                                   mct ? (E.p.irreversible ? norms_irrev : norms_rev) : nullptr, mct ? 3u : E.im.nc};
                        BlockEncResult res;
                        t1_encode_block(mag.data(), neg.data(), w, h, B.orient, res, rc ? &dc : nullptr, E.p.cblk_sty);
                        K.numbps = res.numbps; K.npasses = res.npasses; K.data = res.data; K.passes = res.passes;
    });
}

// planes: nc planes of `rows` rows (row stride w) holding image rows [row0, row0 + rows);
// rows = 0 means the whole image
static void prepare_encode(EncodeState& E, const int32_t* planes, uint32_t w, uint32_t h, uint32_t nc,
                           uint32_t prec, int sgnd, const orc_cparams* cp, uint32_t tile = 0, uint32_t row0 = 0,
                           uint32_t rows = 0) {
    if (!rows) rows = h;
    E.im = Image{w, h, nc, prec, sgnd != 0};
    E.p = to_params(cp);
    settle_mct(E.p, nc);
    E.tile = tile;
    tile_rect(E.p, w, h, tile, E.tx0, E.ty0, E.tx1, E.ty1);
    E.comps.assign(nc, Comp());
    // tile-component c: the tile's rectangle divided by the subsampling (TileProcessor.cpp:116-131)
    std::vector<uint32_t> tcx0(nc), tcy0(nc);
    for (uint32_t c = 0; c < nc; ++c) {
        const uint32_t sx = E.p.sx(c), sy = E.p.sy(c);
        tcx0[c] = ceildiv(E.tx0, sx); tcy0[c] = ceildiv(E.ty0, sy);
        build_geometry(E.comps[c], tcx0[c], tcy0[c], ceildiv(E.tx1, sx), ceildiv(E.ty1, sy), E.p);
        assign_steps(E.comps[c], E.p, prec, true, nullptr, sgnd, E.p.roi(c), c);
    }
    // planes: subsampled components back to back at their own sizes (the whole image only)
    const std::vector<size_t> off = plane_offsets(E.p, w, h, nc);
    E.coefs.assign(nc, {});
    for (uint32_t c = 0; c < nc; ++c) {   // tile-local copy (TileProcessor::ingestImage, TileProcessor.cpp:410-431)
        const Comp& C = E.comps[c];
        uint32_t cw = w, ch = h;
        size_t coff = (size_t)c * w * rows;
        if (E.p.subsampled()) { comp_size(E.p, w, h, c, cw, ch); coff = off[c]; }
        const uint32_t ox = ceildiv(E.p.x0, E.p.sx(c)), oy = ceildiv(E.p.y0, E.p.sy(c));
        E.coefs[c].resize((size_t)C.w * C.h);
        for (uint32_t y = 0; y < C.h; ++y)
            memcpy(&E.coefs[c][(size_t)y * C.w], planes + coff + (size_t)(tcy0[c] - oy - row0 + y) * cw + (tcx0[c] - ox),
                   (size_t)C.w * 4);
    }
    if (!E.p.irreversible) {
        dc_rct_fwd(E.coefs, prec, sgnd != 0, E.p.mct != 0);
        for (uint32_t c = 0; c < nc; ++c)
            dwt2d<int32_t>(E.coefs[c].data(), E.comps[c].w, E.comps[c], E.p.numres, true, fwd53_1d);
    } else {
        dc_ict_fwd(E.fcoefs, E.coefs, prec, sgnd != 0, E.p.mct != 0);
        for (uint32_t c = 0; c < nc; ++c)
            dwt2d<float>(E.fcoefs[c].data(), E.comps[c].w, E.comps[c], E.p.numres, true, fwd97_1d);
    }
}

// ---------------------------------------------------------------------------
// Layer formation and PCRD rate control (TileProcessor.cpp:1196-1515,
// pcrdBisectSimple / makeLayerSimple / makeLayerFinal; rates from
// CodeStreamCompress::updateRates :951-1025; T2 simulation
// T2Compress.cpp:59-112, 114-260, 347-430).
// ---------------------------------------------------------------------------
static void for_blocks(EncodeState& E, const std::function<void(Cblk&)>& f) {
    for (uint32_t c = 0; c < E.im.nc; ++c)
        for (uint32_t r = 0; r < E.p.numres; ++r)
            for (auto& B : E.comps[c].res[r].bands)
                for (auto& P : B.prcs)
                    for (auto& K : P.cblks) f(K);
}

// Passes included up to threshold `thresh` (makeLayerSimple's per-block rule).
static uint32_t included_passes(const Cblk& K, uint32_t prev, double thresh) {
    if (thresh == 0) return K.npasses;
    uint32_t inc = prev;
    for (uint32_t q = prev; q < K.npasses; ++q) {
        uint32_t dr; double dd;
        if (inc == 0) { dr = K.passes[q].rate; dd = K.passes[q].dist; }
        else { dr = K.passes[q].rate - K.passes[inc - 1].rate; dd = K.passes[q].dist - K.passes[inc - 1].dist; }
        if (!dr) { if (dd != 0) inc = q + 1; continue; }
        double slope = dd / dr;
        if (thresh - slope < 2.220446049250313e-16) inc = q + 1;
    }
    return inc;
}

static std::vector<std::vector<std::vector<PrecTrees>>> make_trees(EncodeState& E) {
    std::vector<std::vector<std::vector<PrecTrees>>> trees(E.im.nc);
    for (uint32_t c = 0; c < E.im.nc; ++c) {
        trees[c].resize(E.p.numres);
        for (uint32_t r = 0; r < E.p.numres; ++r) {
            Res& R = E.comps[c].res[r];
            trees[c][r].resize(R.pw * R.ph);
            for (uint32_t pi = 0; pi < R.pw * R.ph; ++pi) {
                PrecTrees& t = trees[c][r][pi];
                t.incl.resize(R.bands.size()); t.imsb.resize(R.bands.size());
                for (size_t bi = 0; bi < R.bands.size(); ++bi) {
                    Precinct& P = R.bands[bi].prcs[pi];
                    if (P.cw && P.ch) { t.incl[bi].build(P.cw, P.ch); t.imsb[bi].build(P.cw, P.ch); }
                }
            }
        }
    }
    return trees;
}

// T2Compress::compressPacketsSimulate (:59-112): do layers [0, max_layers) fit in max_bytes?
// The simulation walks every packet in the tile's own progression (COD's), whatever the
// progression order changes say: its PacketManager is built in THRESH_CALC mode, where
// updateCompressTcpProgressions (PacketManager.cpp:565-589, called at :123-125 with poc =
// false) sets each entry's progression to tcp->prg and its ranges to the whole tile, and
// only the first iterator runs (pocno = 1 outside Cinema 4K).
static bool simulate(EncodeState& E, uint32_t max_layers, uint64_t max_bytes, std::vector<uint32_t>* lens = nullptr) {
    auto trees = make_trees(E);
    uint64_t budget = max_bytes;
    uint64_t* bp = (max_bytes == 0xffffffffull) ? nullptr : &budget;
    for (const PktRef& k : packet_iter(E.comps, E.p, E.tx0, E.ty0, E.tx1, E.ty1, max_layers)) {
        std::vector<uint8_t> tmp;
        uint64_t counted = 0;
        if (!write_packet(lens && !bp ? &tmp : nullptr, E.comps[k.c].res[k.r], k.pi, k.l, trees[k.c][k.r][k.pi], bp,
                          E.p.sop_eph, 0, &counted))
            return false;
        if (lens) lens->push_back((uint32_t)(bp ? counted : tmp.size()));
    }
    return true;
}

// makeLayerSimple (thresh >= 0) / makeLayerFinal (thresh < 0); returns the layer's distortion
// decrease, tile->layerDistoration[layno], summed in block order as there
static double make_layer(EncodeState& E, uint32_t layno, double thresh, bool final_attempt,
                         std::vector<uint32_t>& prev) {
    size_t i = 0;
    double ld = 0.0;
    for_blocks(E, [&](Cblk& K) {
        if (layno == 0) prev[i] = 0;
        uint32_t inc = thresh < 0 ? std::max(prev[i], K.npasses) : included_passes(K, prev[i], thresh);
        K.layer_np[layno] = inc - prev[i];
        if (inc > prev[i]) ld += prev[i] ? K.passes[inc - 1].dist - K.passes[prev[i] - 1].dist : K.passes[inc - 1].dist;
        if (final_attempt) prev[i] = inc;
        ++i;
    });
    return ld;
}

// CodeStreamCompress::updateRates (:951-1025): compression ratios -> cumulative byte budgets of
// the tile, from its pixel count; the SOT adjustment shares the header bytes written before the
// first tile (JP2 boxes, jp2c box header, main header: the stream position) by tile area.
static void update_rates(const EncodeState& E, double* rates) {
    const Params& p = E.p;
    // bits_empty = 8 x component 0's subsampling (updateRates, CodeStreamCompress.cpp:961)
    const double size_pixel = (double)E.im.nc * E.im.prec, bits_empty = 8.0 * p.sx(0) * p.sy(0);
    const double npix = (double)((uint64_t)(E.tx1 - E.tx0) * (E.ty1 - E.ty0));
    // tile-part generation: (parts - 1) x 14 bytes of SOT + SOD, spread over the layers
    const double offset = (double)((std::max(1, tile_parts(p, E.im.nc)) - 1) * 14) / (double)p.nlayers;
    for (uint32_t k = 0; k < p.nlayers; ++k)
        rates[k] = p.rates[k] > 0.0 ? (size_pixel * npix) / (p.rates[k] * bits_empty) - offset : 0.0;
    double sot_adjust = (npix * (double)E.header_size) / ((double)E.im.w * (double)E.im.h);
    uint32_t k = 0;
    if (rates[0] > 0.0) { rates[0] -= sot_adjust; if (rates[0] < 30.0f) rates[0] = 30.0f; }
    for (k = 1; k + 1 < p.nlayers; ++k)
        if (rates[k] > 0.0) { rates[k] -= sot_adjust; if (rates[k] < rates[k - 1] + 10.0) rates[k] = rates[k - 1] + 20.0; }
    k = std::max(1u, p.nlayers - 1);
    if (p.nlayers > 1 && rates[k] > 0.0) {
        rates[k] -= (sot_adjust + 2.0);
        if (rates[k] < rates[k - 1] + 10.0) rates[k] = rates[k - 1] + 20.0;
    }
}

// TileProcessor::pcrdBisectSimple
static void rate_allocate(EncodeState& E) {
    size_t nb = 0;
    for_blocks(E, [&](Cblk& K) { K.layer_np.assign(E.p.nlayers, 0); ++nb; });
    std::vector<uint32_t> prev(nb, 0);
    if (!needs_rate_control(E.p)) {
        for (uint32_t l = 0; l < E.p.nlayers; ++l) make_layer(E, l, -1.0, true, prev);
        return;
    }
    double rates[100];
    update_rates(E, rates);
    // fixed quality (TileProcessor.cpp:1263-1267, 1299-1322): the layer's target is the tile's
    // distortion less maxSE / 10^(PSNR/10), maxSE = sum over components of (2^prec - 1)^2 x
    // the component's code-block area; tile->distortion is the blocks' total distortion
    // decrease in block order (T1CompressScheduler::compress, single-threaded order)
    double tile_dist = 0.0, maxSE = 0.0;
    if (E.p.quality) {
        for (uint32_t c = 0; c < E.im.nc; ++c) {
            uint64_t numpix = 0;
            for (uint32_t r = 0; r < E.p.numres; ++r)
                for (auto& B : E.comps[c].res[r].bands)
                    for (auto& P : B.prcs)
                        for (auto& K : P.cblks) {
                            numpix += (uint64_t)(K.x1 - K.x0) * (K.y1 - K.y0);
                            if (K.npasses) tile_dist += K.passes[K.npasses - 1].dist;
                        }
            const double m = (double)((1ull << E.im.prec) - 1);
            maxSE += m * m * (double)numpix;
        }
    }
    double cum[100] = {0};
    double min_slope = 1.7976931348623157e308, max_slope = -1;
    for_blocks(E, [&](Cblk& K) {
        for (uint32_t q = 0; q < K.npasses; ++q) {
            int32_t dr; double dd;
            if (q == 0) { dr = (int32_t)K.passes[q].rate; dd = K.passes[q].dist; }
            else { dr = (int32_t)(K.passes[q].rate - K.passes[q - 1].rate); dd = K.passes[q].dist - K.passes[q - 1].dist; }
            if (dr == 0) continue;
            double sl = dd / dr;
            min_slope = std::min(min_slope, sl); max_slope = std::max(max_slope, sl);
        }
    });
    double upper = max_slope;
    uint64_t last_len = 0xffffffffull;   // maxLayerLength after the loop: the last layer's
    for (uint32_t l = 0; l < E.p.nlayers; ++l) {
        uint64_t max_len = rates[l] > 0.0f ? (uint64_t)(uint32_t)ceil(rates[l]) : 0xffffffffull;
        last_len = max_len;
        if (const char* fb = getenv("ORC_FORCE_BUDGET")) {   // debugging aid: "tile:layer:bytes,..."
            for (const char* q = fb; *q;) {
                unsigned ft, fl; unsigned long long fv; int n = 0;
                if (sscanf(q, "%u:%u:%llu%n", &ft, &fl, &fv, &n) != 3) break;
                if (ft == E.tile && fl == l) max_len = fv;
                q += n; if (*q == ',') ++q;
            }
        }
        // layerNeedsRateControl reads the tile's byte budget, not the ratio asked for: where the
        // tile-part offset exceeds a small tile's budget (updateRates leaves it negative) the
        // layer takes every remaining pass
        if (E.p.quality ? layer_needs_rc(E.p, l) : rates[l] > 0.0) {
            double lower = min_slope, prevthresh = -1, thresh = 0;
            const double target = E.p.quality ? tile_dist - maxSE / pow(10.0, E.p.dist[l] / 10.0) : 0.0;
            for (uint32_t it = 0; it < 128; ++it) {
                thresh = (upper == -1) ? lower : (lower + upper) / 2;
                const double ld = make_layer(E, l, thresh, false, prev);
                if (prevthresh != -1 && fabs(prevthresh - thresh) < 0.001) break;
                prevthresh = thresh;
                if (E.p.quality) {
                    const double achieved = l == 0 ? ld : cum[l - 1] + ld;
                    if (achieved < target) { upper = thresh; continue; }
                    lower = thresh;
                } else {
                    const bool fits = simulate(E, l + 1, max_len);
                    if (getenv("ORC_RC_TRACE"))   // debugging aid: the bisection's steps
                        fprintf(stderr, "  tile %u layer %u it %u thresh %.17g lower %.17g upper %.17g %s budget %llu\n",
                                E.tile, l, it, thresh, lower, upper, fits ? "fits" : "fails", (unsigned long long)max_len);
                    if (!fits) { lower = thresh; continue; }
                    upper = thresh;
                }
            }
            double good = (upper == -1) ? thresh : upper;
            if (const char* ft = getenv("ORC_FORCE_THRESH")) {   // debugging aid: "layer:thresh,..."
                for (const char* q = ft; *q;) {
                    unsigned fl, ftile; double fv; int n = 0;
                    if (sscanf(q, "%u:%u:%lf%n", &ftile, &fl, &fv, &n) == 3) {
                        if (fl == l && ftile == E.tile) good = fv;
                    } else if (sscanf(q, "%u:%lf%n", &fl, &fv, &n) == 2) {
                        if (fl == l) good = fv;
                    } else break;
                    q += n; if (*q == ',') ++q;
                }
            }
            const double ld = make_layer(E, l, good, true, prev);
            cum[l] = l == 0 ? ld : cum[l - 1] + ld;
            upper = lower - 1;
        } else {
            make_layer(E, l, -1.0, true, prev);
        }
    }
    if (!E.p.quality) {   // the final simulation (with fixed quality maxLayerLength stays UINT_MAX there too)
        E.sim_lens.clear();
        E.have_sim = simulate(E, E.p.nlayers, last_len, &E.sim_lens);
    }
}

// One tile's packets in LRCP order (T2Compress::compressPackets); packet lengths
// are recorded for PLT.
// With progression order changes the packets of entry k form tile part k, and the PLT lengths
// (plt) are listed in the tile's own progression: Grok's PLT is filled by the rate-control
// simulation (compressPacketSimulate :427-428, THRESH_CALC order, see simulate()), not by the
// packets as written.
static void tile_packets(EncodeState& E, std::vector<uint8_t>& body, std::vector<uint32_t>& plens,
                         std::vector<uint32_t>* pparts = nullptr, std::vector<uint32_t>* plt = nullptr) {
    auto trees = make_trees(E);
    const bool poc = !E.p.pocs.empty();
    std::vector<uint32_t> entry;
    const std::vector<PktRef> order =
        packet_iter(E.comps, E.p, E.tx0, E.ty0, E.tx1, E.ty1, E.p.nlayers, &E.p.pocs, poc ? &entry : nullptr);
    for (size_t i = 0; i < order.size(); ++i) {
        const PktRef& k = order[i];
        size_t before = body.size();
        write_packet(&body, E.comps[k.c].res[k.r], k.pi, k.l, trees[k.c][k.r][k.pi], nullptr, E.p.sop_eph,
                     poc ? entry[2 * i + 1] : (uint32_t)plens.size(), nullptr, E.p.ppx ? &E.pkt_headers : nullptr);
        plens.push_back((uint32_t)(body.size() - before));
        if (pparts) pparts->push_back(poc ? entry[2 * i] : tile_part_of(E.p, E.im.nc, k));
    }
    if (!plt) return;
    if (!poc) { *plt = plens; return; }
    std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>, uint32_t> len;   // (c, r, pi, l) -> bytes
    for (size_t i = 0; i < order.size(); ++i) len[{order[i].c, order[i].r, order[i].pi, order[i].l}] = plens[i];
    plt->clear();
    for (const PktRef& k : packet_iter(E.comps, E.p, E.tx0, E.ty0, E.tx1, E.ty1, E.p.nlayers)) {
        auto it = len.find({k.c, k.r, k.pi, k.l});
        if (it != len.end()) plt->push_back(it->second);
    }
}

// A POC list must name every packet of the tile: CodeStreamCompress::validateProgressionOrders
// (:1685-1747) refuses a list that misses one.  (A packet two entries name is written once, in
// the first entry's part: the tile's packet tracker, T2Compress.cpp:278-280.)
// B.6: a resolution above 0 splits its precinct partition among the bands at PPx - 1, so its
// exponent must be at least 1 (Grok never writes 0 there; CodeStreamCompress.cpp:575-590 clamps
// sizes below 1 to exponent 1 and only a size of exactly 1 reaches 0, at the lowest resolution)
static bool prc_exps_ok(const Params& p) {
    for (uint32_t r = 1; r < p.numres; ++r)
        if (p.prcw_exp[r] == 0 || p.prch_exp[r] == 0) return false;
    return true;
}

static bool pocs_cover(const Params& p, uint32_t nc) {
    if (p.pocs.empty()) return true;
    std::vector<uint8_t> n((size_t)p.nlayers * p.numres * nc, 0);
    for (const PocE& e : p.pocs)
        for (uint32_t l = 0; l < std::min(e.lye, p.nlayers); ++l)
            for (uint32_t r = e.rs; r < std::min(e.re, p.numres); ++r)
                for (uint32_t c = e.cs; c < std::min(e.ce, nc); ++c) n[((size_t)l * p.numres + r) * nc + c] = 1;
    for (uint8_t v : n) if (!v) return false;
    return true;
}

// Tile part: SOT [PLT] SOD packets (CodeStreamCompress::writeTilePart :862-900; SOT with
// TPsot = 0, TNsot = 1; PLT from PacketLengthMarkers::write, PacketLengthMarkers.cpp:107-175:
// Zplt = 0, each length as 7-bit groups MSB first with a continuation bit).
// The tile's tile parts (CodeStreamCompress::writeTileParts / writeTilePart, :858-946): SOT
// (TPsot = part, TNsot = parts) [PLT of every packet of the tile, first part only
// (TileProcessor::writeTilePartT2)] SOD, packets.  Returns each part's Psot.
static std::vector<uint32_t> write_tile_part(std::vector<uint8_t>& o, EncodeState& E) {
    std::vector<uint8_t> body; std::vector<uint32_t> plens, pparts, plt;
    tile_packets(E, body, plens, &pparts, &plt);
    if (E.have_sim) plt = E.sim_lens;   // PLT from the rate control's final simulation
    const int np = num_parts(E.p, E.im.nc);
    // CodeStreamCompress::writeTilePart (:858-900): a tile in one part with one progression
    // writes the length TileProcessor precalculated (SOT + [PLT] + SOD + the simulation's
    // packet bytes) as Psot and in TLM (canPreCalculateTileLen :54-57)
    const bool precalc = np == 1 && E.p.pocs.empty();
    std::vector<uint32_t> psots;
    size_t pk = 0, boff = 0;
    for (int part = 0; part < np; ++part) {
        size_t sot = o.size();
        put16(o, 0xff90); put16(o, 10); put16(o, E.tile); put32(o, 0); o.push_back((uint8_t)part); o.push_back((uint8_t)np);
        if (part == 0 && !E.p.pocs.empty()) {
            // POC in the tile's first tile part (writeTilePart :870-875): writePoc writes tile 0's
            // list (tcp = m_cp.tcps), clamped by the main header's writePoc; each entry's
            // progression is what tile 0's last PacketManager left there - for tile 0 its own
            // rate-control simulation (THRESH_CALC: tcp->prg), for later tiles tile 0's final
            // pass (the given progression)
            std::vector<PocE> w = E.p.pocs;
            for (PocE& e : w) {
                e.lye = std::min(e.lye, E.p.nlayers); e.re = std::min(e.re, E.p.numres); e.ce = std::min(e.ce, E.im.nc);
                if (E.tile == 0) e.prog = E.p.prog;
            }
            write_poc(o, w, E.im.nc);
        }
        if (E.p.ppx == 1) {   // PPT: the tile's packet headers, Zppt 0, 1, ... of at most 65533 bytes each
            for (size_t at = 0, z = 0; at < E.pkt_headers.size() || z == 0; ++z) {
                const size_t n = std::min<size_t>(65532, E.pkt_headers.size() - at);
                put16(o, 0xff61); put16(o, (uint32_t)(3 + n)); o.push_back((uint8_t)z);
                o.insert(o.end(), E.pkt_headers.begin() + at, E.pkt_headers.begin() + at + n);
                at += n;
            }
        }
        if (E.p.plt && part == 0) {
            std::vector<uint8_t> v;
            for (uint32_t L : plt) {
                int nbits = floorlog2(L) + 1, nbytes = (nbits + 6) / 7;
                for (int k = nbytes - 1; k >= 0; --k) v.push_back((uint8_t)(((L >> (7 * k)) & 0x7F) | (k ? 0x80 : 0)));
            }
            put16(o, 0xff58); put16(o, (uint32_t)(3 + v.size())); o.push_back(0);
            o.insert(o.end(), v.begin(), v.end());
        }
        put16(o, 0xff93);
        size_t bl = 0;
        while (pk < plens.size() && pparts[pk] == (uint32_t)part) bl += plens[pk++];
        o.insert(o.end(), body.begin() + boff, body.begin() + boff + bl);
        boff += bl;
        uint32_t psot = (uint32_t)(o.size() - sot);
        if (precalc && E.have_sim) {
            uint64_t sum = 0;
            for (uint32_t L : E.sim_lens) sum += L;
            psot = (uint32_t)(psot - bl + sum);
        }
        o[sot + 6] = (uint8_t)(psot >> 24); o[sot + 7] = (uint8_t)(psot >> 16); o[sot + 8] = (uint8_t)(psot >> 8); o[sot + 9] = (uint8_t)psot;
        psots.push_back(psot);
    }
    return psots;
}

// ----------------------------------------------------------------------------
// Encode refusal by precision: a band whose largest reachable magnitude the coder
// cannot hold.  The largest magnitude of a band is the largest input magnitude times the band's
// BIBO analysis gain (the largest sum of absolute weights with which input samples enter one of
// its coefficients): the 5/3 gains of HTParams.cpp:134-145 above, the 9/7 gains below for the
// lifting as fwd97_1d scales it (low band / K, high band * K).  Containers:
//  - Part 1: t1_encode_all keeps magnitude << 6 (T1_NMSEDEC_FRACBITS) in a uint32: 26 bits;
//  - HT: the decoders place a block's magnitudes under 30 - k_msbs, k_msbs = numbps - 1 <= 29: 30 bit-planes;
//  - QCD / QCC: a 5-bit exponent;
//  - 9/7: float32 samples, exact up to 2^24 after the DC shift: 25 bits of precision.
// The bands judged are those of at least two resolutions, so that numres = 1 accepts nothing
// that a transform would refuse.  Returns the reason, empty when the encode is accepted.
// ----------------------------------------------------------------------------
static const double bibo97_l[5] = {1.0000, 1.3803, 1.3328, 1.3067, 1.3028};   // past [4]: smaller
static const double bibo97_h[5] = {2.5953, 2.6253, 2.5514, 2.4703, 2.4625};
static thread_local std::string t_last_error;
static std::string precision_refusal(const Params& p0, uint32_t nc, uint32_t prec, int sgnd) {
    char msg[256];
    if (prec == 0 || prec > 31) {
        snprintf(msg, sizeof msg, "precision %u: component precision must be 1..31 bits", prec);
        return msg;
    }
    if (p0.irreversible && prec > 25) {
        snprintf(msg, sizeof msg, "precision %u: the 9/7 transform's float32 samples are exact up to 25 bits", prec);
        return msg;
    }
    Params p = p0;
    settle_mct(p, nc);
    p.numres = std::max(p0.numres, 2u);
    const uint32_t nd = p.numres - 1;
    const double margin = 1.0 + 1.0 / 1024;   // the gain tables' four decimals
    static const char* const oname[4] = {"LL", "HL", "LH", "HH"};
    for (uint32_t c = 0; c < nc; ++c) {
        Comp C;
        build_geometry(C, 0, 0, 64, 64, p);
        assign_steps(C, p, prec, true, nullptr, sgnd, 0, c);
        // input range after the DC shift: [-2^(p-1), 2^(p-1) - 1]; RCT chroma is a difference of
        // two samples, +-(2^p - 1); ICT rows have absolute sums <= 1
        const bool chroma = p.mct && !p.irreversible && (c == 1 || c == 2);
        const double full = chroma ? ldexp(1.0, (int)prec) - 1.0 : ldexp(1.0, (int)prec - 1);
        // a band without a low-pass step has no DC gain: the range counts from its centre
        const double centred = chroma ? full : full - 0.5;
        for (uint32_t r = 0; r < p.numres; ++r)
            for (const Band& B : C.res[r].bands) {
                const uint32_t d = r ? nd - r : nd;
                double g, in = full, slack;
                if (!p.irreversible) {
                    auto L = [](uint32_t i) { return (double)bibo53_l[std::min(i, 15u)]; };
                    auto H = [](uint32_t i) { return (double)bibo53_h[std::min(i, 15u)]; };
                    g = r == 0 ? L(nd) * L(nd) : B.orient == 3 ? H(d) * H(d) : H(d) * L(d + 1);
                    // the finest HH is two exact integer high-pass steps (gain 2 * 2); every other
                    // band passes low-pass steps that round, each by less than 1
                    const bool exact = r == nd && B.orient == 3;
                    if (exact) in = centred;
                    slack = exact ? 0.0 : 16.0 * p.numres;
                    if (!exact) g *= margin;
                } else {
                    auto L = [](uint32_t i) { return bibo97_l[std::min(i, 4u)]; };
                    auto H = [](uint32_t i) { return bibo97_h[std::min(i, 4u)]; };
                    g = (r == 0 ? L(nd) * L(nd) : B.orient == 3 ? H(d) * H(d) : H(d) * L(d + 1)) * margin / (double)B.stepsize;
                    slack = 1.0;   // the quantiser's rounding
                }
                const double bound = g * in + slack;
                const int need = (int)floor(log2(bound)) + 1;
                const int hold = p.ht() ? 30 : 26;
                if (B.expn > 31) {
                    snprintf(msg, sizeof msg, "precision %u: exponent %u of the %s band (component %u, resolution %u) "
                             "does not fit the 5-bit QCD field", prec, B.expn, oname[B.orient], c, r);
                    return msg;
                }
                if (p.ht() && B.numbps > 30) {
                    snprintf(msg, sizeof msg, "precision %u: %u bit-planes in the %s band (component %u, resolution %u), "
                             "the HT coder holds 30", prec, B.numbps, oname[B.orient], c, r);
                    return msg;
                }
                if (!(bound < ldexp(1.0, hold))) {
                    snprintf(msg, sizeof msg, "precision %u: the %s band (component %u, resolution %u) can reach %d "
                             "magnitude bits, the %s coder holds %d", prec, oname[B.orient], c, r, need,
                             p.ht() ? "HT" : "Part-1", hold);
                    return msg;
                }
            }
    }
    return std::string();
}
const char* orc_last_error() { return t_last_error.c_str(); }

// Full encode (5/3 or 9/7, Part 1 or HT, any number of layers, one or more tiles).
// Returns the codestream size, or 0 on failure / insufficient capacity.
static void jp2_prefix(std::vector<uint8_t>& o, uint32_t w, uint32_t h, uint32_t nc, uint32_t prec, int sgnd,
                       uint64_t cs_len);

size_t orc_encode(const int32_t* planes, uint32_t w, uint32_t h, uint32_t nc, uint32_t prec, int sgnd,
                  const orc_cparams* cp, uint8_t* out, size_t cap) {
    std::vector<uint8_t> o;
    size_t tlm_pos = 0;
    uint32_t nt = 0;
    const Params p0 = to_params(cp);
    t_last_error = precision_refusal(p0, nc, prec, sgnd);
    if (!t_last_error.empty()) return 0;
    if (!prc_exps_ok(p0) || !pocs_cover(p0, nc) || num_parts(p0, nc) < 1) return 0;
    // packed packet headers: one tile part per tile, no rate control or PLT (test streams)
    if (p0.ppx && (num_parts(p0, nc) != 1 || needs_rate_control(p0) || p0.plt)) return 0;
    std::vector<std::vector<uint8_t>> ppm_tiles;   // PPM: each tile's packet headers
    if (!needs_rate_control(p0) && tile_count(p0, w, h) > 1) {
        // independent tiles coded in parallel, written in tile order
        nt = tile_count(p0, w, h);
        {
            EncodeState E0;
            E0.im = Image{w, h, nc, prec, sgnd != 0};
            E0.p = p0;
            settle_mct(E0.p, nc);
            E0.comps.assign(1, Comp());
            uint32_t x0, y0, x1, y1;
            tile_rect(E0.p, w, h, 0, x0, y0, x1, y1);
            build_geometry(E0.comps[0], x0, y0, x1, y1, E0.p);
            assign_steps(E0.comps[0], E0.p, prec, true, nullptr, sgnd);
            write_main_header(o, E0.im, E0.p, E0.comps[0], &tlm_pos);
        }
        std::vector<std::vector<uint8_t>> parts(nt);
        std::vector<std::vector<uint32_t>> psl(nt);
        ppm_tiles.assign(nt, {});
        par_for(nt, [&](size_t t) {
            EncodeState E;
            prepare_encode(E, planes, w, h, nc, prec, sgnd, cp, (uint32_t)t);
            t1_encode_all(E);
            rate_allocate(E);
            psl[t] = write_tile_part(parts[t], E);
            ppm_tiles[t].swap(E.pkt_headers);
        });
        for (uint32_t t = 0; t < nt; ++t) {
            for (size_t k = 0; p0.tlm && k < psl[t].size(); ++k) {
                const uint32_t psot = psl[t][k];
                size_t q = tlm_pos + (size_t)6 * (t * psl[t].size() + k);
                o[q] = (uint8_t)(t >> 8); o[q + 1] = (uint8_t)t;
                o[q + 2] = (uint8_t)(psot >> 24); o[q + 3] = (uint8_t)(psot >> 16); o[q + 4] = (uint8_t)(psot >> 8); o[q + 5] = (uint8_t)psot;
            }
            o.insert(o.end(), parts[t].begin(), parts[t].end());
            std::vector<uint8_t>().swap(parts[t]);
        }
        put16(o, 0xffd9);
    } else {
    size_t header_size = 0;
    for (uint32_t t = 0;; ++t) {
        EncodeState E;
        prepare_encode(E, planes, w, h, nc, prec, sgnd, cp, t);
        if (t == 0) {
            nt = tile_count(E.p, w, h);
            write_main_header(o, E.im, E.p, E.comps[0], &tlm_pos);
            header_size = o.size();   // updateRates runs once, after the main header
            if (cp && cp->cod_format == 2) {
                std::vector<uint8_t> J0;
                jp2_prefix(J0, w, h, nc, prec, sgnd, 0);
                header_size += J0.size();
            }
        }
        E.header_size = header_size;
        t1_encode_all(E);
        rate_allocate(E);
        const std::vector<uint32_t> psl = write_tile_part(o, E);
        ppm_tiles.push_back(std::move(E.pkt_headers));
        for (size_t k = 0; E.p.tlm && k < psl.size(); ++k) {
            const uint32_t psot = psl[k];
            size_t q = tlm_pos + (size_t)6 * (t * psl.size() + k);
            o[q] = (uint8_t)(t >> 8); o[q + 1] = (uint8_t)t;
            o[q + 2] = (uint8_t)(psot >> 24); o[q + 3] = (uint8_t)(psot >> 16); o[q + 4] = (uint8_t)(psot >> 8); o[q + 5] = (uint8_t)psot;
        }
        if (t + 1 >= nt) { put16(o, 0xffd9); break; }
    }
    }
    if (p0.ppx == 2) {
        // PPM in the main header, before the first SOT: Nppm (4 bytes) + the headers of each tile
        // part in codestream order (one per tile here), split over markers of Zppm 0, 1, ...
        std::vector<uint8_t> v, m;
        for (const auto& t : ppm_tiles) { put32(v, (uint32_t)t.size()); v.insert(v.end(), t.begin(), t.end()); }
        for (size_t at = 0, z = 0; at < v.size(); ++z) {
            if (z > 255) return 0;
            const size_t n = std::min<size_t>(65532, v.size() - at);
            put16(m, 0xff60); put16(m, (uint32_t)(3 + n)); m.push_back((uint8_t)z);
            m.insert(m.end(), v.begin() + at, v.begin() + at + n);
            at += n;
        }
        size_t sot = 2;
        while (get16(o.data() + sot) != 0xff90) sot += 2 + get16(o.data() + sot + 2);
        o.insert(o.begin() + sot, m.begin(), m.end());
    }
    std::vector<uint8_t> J;
    if (cp && cp->cod_format == 2) jp2_prefix(J, w, h, nc, prec, sgnd, o.size());
    if (J.size() + o.size() > cap) return 0;
    memcpy(out, J.data(), J.size());
    memcpy(out + J.size(), o.data(), o.size());
    return J.size() + o.size();
}

// ----------------------------------------------------------------------------
// JP2 file format (ISO 15444-1 Annex I) as Grok writes it for PNM input:
// signature box, ftyp (brand/compat 'jp2 '), jp2h = ihdr (22 B) + colr (15 B,
// METH 1, EnumCS sRGB 16 / greyscale 17), then the jp2c box, whose header has an
// 8-byte XLBox when the raw image exceeds 2^30 bytes (FileFormatCompress.cpp:
// write_jp :43-58, write_ftyp :103-148, write_jp2h :176-264, write_colr :344-403,
// write_ihdr :619-665, startCompress :678-686, write_jp2c :59-102).
// ----------------------------------------------------------------------------
static void jp2_prefix(std::vector<uint8_t>& o, uint32_t w, uint32_t h, uint32_t nc, uint32_t prec, int sgnd,
                       uint64_t cs_len) {
    auto box = [&](uint32_t len, const char* type) { put32(o, len); o.insert(o.end(), type, type + 4); };
    box(12, "jP  "); put32(o, 0x0d0a870a);
    box(20, "ftyp"); o.insert(o.end(), {'j', 'p', '2', ' '}); put32(o, 0); o.insert(o.end(), {'j', 'p', '2', ' '});
    box(45, "jp2h");
    box(22, "ihdr"); put32(o, h); put32(o, w); put16(o, nc);
    o.push_back((uint8_t)((prec - 1) + (sgnd ? 128 : 0))); o.push_back(7); o.push_back(0); o.push_back(0);
    box(15, "colr"); o.push_back(1); o.push_back(0); o.push_back(0); put32(o, nc < 3 ? 17 : 16);
    const bool xl = (uint64_t)nc * w * h * ((prec + 7) / 8) > (1ull << 30);
    if (xl) { box(1, "jp2c"); put32(o, (uint32_t)((cs_len + 16) >> 32)); put32(o, (uint32_t)(cs_len + 16)); }
    else box(cs_len + 8 < (1ull << 32) ? (uint32_t)(cs_len + 8) : 0, "jp2c");
}

size_t orc_jp2_header(uint32_t w, uint32_t h, uint32_t nc, uint32_t prec, int sgnd, uint64_t cs_len, uint8_t* out) {
    std::vector<uint8_t> J;
    jp2_prefix(J, w, h, nc, prec, sgnd, cs_len);
    if (out) memcpy(out, J.data(), J.size());
    return J.size();
}

// Main header alone (SOC .. TLM placeholder .. COM), for assembling tile parts coded separately.
size_t orc_main_header(uint32_t w, uint32_t h, uint32_t nc, uint32_t prec, int sgnd, const orc_cparams* cp, uint8_t* out,
                       size_t cap, size_t* tlm_offset) {
    EncodeState E0;
    E0.im = Image{w, h, nc, prec, sgnd != 0};
    E0.p = to_params(cp);
    settle_mct(E0.p, nc);
    E0.comps.assign(1, Comp());
    uint32_t x0, y0, x1, y1;
    tile_rect(E0.p, w, h, 0, x0, y0, x1, y1);
    build_geometry(E0.comps[0], x0, y0, x1, y1, E0.p);
    assign_steps(E0.comps[0], E0.p, prec, true, nullptr, sgnd);
    std::vector<uint8_t> o;
    size_t tlm = 0;
    write_main_header(o, E0.im, E0.p, E0.comps[0], &tlm);
    if (tlm_offset) *tlm_offset = E0.p.tlm ? tlm : 0;
    if (o.size() > cap) return 0;
    memcpy(out, o.data(), o.size());
    return o.size();
}

// Tile parts of tiles [tb, te) (no rate control) from a slab holding image rows
// [row0, row0 + rows) of every component (component stride w * rows); part_lens[i]
// = Psot of tile tb + i.  Returns the bytes written, 0 if cap is too small.
size_t orc_encode_tile_parts(const int32_t* slab, uint32_t w, uint32_t h, uint32_t nc, uint32_t prec, int sgnd,
                             const orc_cparams* cp, uint32_t row0, uint32_t rows, uint32_t tb, uint32_t te,
                             uint8_t* out, size_t cap, uint32_t* part_lens) {
    t_last_error = precision_refusal(to_params(cp), nc, prec, sgnd);
    if (!t_last_error.empty()) return 0;
    if (!prc_exps_ok(to_params(cp)) || to_params(cp).subsampled()) return 0;   // (whole-image planes only)
    std::vector<std::vector<uint8_t>> parts(te - tb);
    par_for(te - tb, [&](size_t q) {
        EncodeState E;
        prepare_encode(E, slab, w, h, nc, prec, sgnd, cp, tb + (uint32_t)q, row0, rows);
        t1_encode_all(E);
        rate_allocate(E);
        write_tile_part(parts[q], E);
    });
    size_t n = 0;
    for (size_t q = 0; q < parts.size(); ++q) {
        if (n + parts[q].size() > cap) return 0;
        memcpy(out + n, parts[q].data(), parts[q].size());
        part_lens[q] = (uint32_t)parts[q].size();
        n += parts[q].size();
    }
    return n;
}

// Stage dump: forward DC+RCT+DWT coefficients (Mallat, stride w), nc planes.
void orc_forward_coefs(const int32_t* planes, uint32_t w, uint32_t h, uint32_t nc, uint32_t prec, int sgnd,
                       const orc_cparams* cp, int32_t* out) {
    EncodeState E;
    prepare_encode(E, planes, w, h, nc, prec, sgnd, cp);
    for (uint32_t c = 0; c < nc; ++c)   // 9/7: the float coefficients' bits
        memcpy(out + (size_t)c * w * h, E.p.irreversible ? (const void*)E.fcoefs[c].data() : (const void*)E.coefs[c].data(),
               (size_t)w * h * 4);
}

// Stage dump: per-block T1 results in canonical order.  Two calls: first with
// blocks==NULL to get counts (*nblocks, *nbytes).
int orc_encode_blocks(const int32_t* planes, uint32_t w, uint32_t h, uint32_t nc, uint32_t prec, int sgnd,
                      const orc_cparams* cp, orc_block* blocks, uint32_t* nblocks, uint8_t* data, uint64_t* nbytes) {
    EncodeState E;
    prepare_encode(E, planes, w, h, nc, prec, sgnd, cp);
    t1_encode_all(E);
    uint32_t n = 0; uint64_t off = 0;
    for (uint32_t c = 0; c < nc; ++c)
        for (uint32_t r = 0; r < E.p.numres; ++r) {
            Res& R = E.comps[c].res[r];
            for (uint32_t bi = 0; bi < R.bands.size(); ++bi)
                for (uint32_t pi = 0; pi < R.bands[bi].prcs.size(); ++pi) {
                    Precinct& P = R.bands[bi].prcs[pi];
                    for (uint32_t k = 0; k < P.cblks.size(); ++k) {
                        Cblk& K = P.cblks[k];
                        if (blocks) {
                            orc_block& b = blocks[n];
                            b.comp = c; b.res = r; b.band = bi; b.prc = pi; b.cblk = k;
                            b.x0 = K.x0; b.y0 = K.y0; b.x1 = K.x1; b.y1 = K.y1;
                            b.numbps = K.numbps; b.npasses = K.npasses; b.len = (uint32_t)K.data.size();
                            b.data_off = off;
                            if (data) memcpy(data + off, K.data.data(), K.data.size());
                        }
                        ++n; off += K.data.size();
                    }
                }
        }
    *nblocks = n; *nbytes = off;
    return 0;
}

// Per-pass rates and cumulative distortion decreases of every code-block, concatenated in
// the canonical order of orc_encode_blocks (CodePass::rate / distortiondec after
// T1::compress_cblk's rate rules, T1.cpp:856-930).  rates / dists may be NULL (count only).
int orc_encode_block_passes(const int32_t* planes, uint32_t w, uint32_t h, uint32_t nc, uint32_t prec, int sgnd,
                            const orc_cparams* cp, uint32_t* rates, double* dists, uint64_t* npasses) {
    EncodeState E;
    prepare_encode(E, planes, w, h, nc, prec, sgnd, cp);
    t1_encode_all(E);
    uint64_t n = 0;
    for (uint32_t c = 0; c < nc; ++c)
        for (uint32_t r = 0; r < E.p.numres; ++r)
            for (auto& B : E.comps[c].res[r].bands)
                for (auto& P : B.prcs)
                    for (auto& K : P.cblks)
                        for (uint32_t q = 0; q < K.npasses; ++q, ++n) {
                            if (rates) rates[n] = K.passes[q].rate;
                            if (dists) dists[n] = K.passes[q].dist;
                        }
    *npasses = n;
    return 0;
}

// Single code-block T1 encode from signed integer coefficients (reversible
// convention: value << 6 to SMR).  Returns the byte length; pass rates in rates[].
int orc_t1_encode_cblk(const int32_t* coef, uint32_t w, uint32_t h, uint32_t stride, uint32_t orient,
                       uint8_t* out, uint32_t cap, uint32_t* numbps, uint32_t* npasses, uint32_t* rates, uint32_t* lens) {
    std::vector<uint32_t> mag(w * h); std::vector<uint8_t> neg(w * h);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            int64_t s = (int64_t)coef[(size_t)y * stride + x] * (1 << FRACBITS);
            neg[y * w + x] = s < 0; mag[y * w + x] = (uint32_t)(s < 0 ? -s : s);
        }
    BlockEncResult r;
    t1_encode_block(mag.data(), neg.data(), w, h, orient, r, nullptr);
    *numbps = r.numbps; *npasses = r.npasses;
    for (uint32_t i = 0; i < r.npasses; ++i) { if (rates) rates[i] = r.passes[i].rate; if (lens) lens[i] = r.passes[i].len; }
    if (r.data.size() > cap) return -1;
    memcpy(out, r.data.data(), r.data.size());
    return (int)r.data.size();
}

// Single code-block HT cleanup-pass encode / decode (signed coefficients).
int orc_ht_encode_cblk(const int32_t* coef, uint32_t w, uint32_t h, uint32_t stride, uint8_t* out, uint32_t cap) {
    std::vector<uint8_t> d = ht_encode_block(coef, w, h, stride);
    if (d.size() > cap) return -1;
    memcpy(out, d.data(), d.size());
    return (int)d.size();
}
int orc_ht_decode_cblk(const uint8_t* data, uint32_t len, uint32_t w, uint32_t h, uint32_t k_msbs, int32_t* out) {
    return ht_decode_block(data, len, w, h, k_msbs, out, w) ? 0 : -1;
}

// Instrumentation: decisions at the start of every (pass, stripe) of a block decode
// (counts[npasses * nstripes] = total).  Used by tools/t1_simt_stats.py only.
void orc_t1_decode_stripe_counts(const uint8_t* data, uint32_t len, uint32_t npasses, uint32_t numbps, uint32_t orient,
                                 uint32_t w, uint32_t h, uint32_t* counts) {
    std::vector<int32_t> out((size_t)w * h);
    t1_decode_block(data, len, npasses, numbps, orient, w, h, out.data(), counts);
}

// Single code-block T1 decode -> Grok's pre-filter values (2x magnitude with half bit).
void orc_t1_decode_cblk(const uint8_t* data, uint32_t len, uint32_t npasses, uint32_t numbps, uint32_t orient,
                        uint32_t w, uint32_t h, int32_t* out) {
    t1_decode_block(data, len, npasses, numbps, orient, w, h, out);
}

// ----------------------------------------------------------------------------
// Decoder: main header, then one tile part per tile (SOT [PLT/other] SOD
// packets), LRCP, any number of layers, Part-1 default style or HT.  Output
// planes are int32 at the image precision.  (CodeStreamDecompress.cpp marker
// handlers; T2Decompress.cpp:216-570; TileProcessor decompress path.)
// ----------------------------------------------------------------------------
// ranges: the packet bytes [data, end) of the tile's tile parts in TPsot order (a tile's
// packet sequence continues across its parts, A.4.2)
static int decode_tile(const uint8_t* cs, const std::vector<std::pair<size_t, size_t>>& ranges, const Params& p,
                       const std::vector<Params>& pcs, const Image& im, const std::vector<Quant>& cq, uint32_t tile,
                       int32_t* out, const std::vector<PocE>* tpocs = nullptr, const std::vector<uint8_t>* hdr = nullptr) {
    size_t data = ranges[0].first, tile_end = ranges[0].second, next_range = 1;
    size_t hpos = 0;   // read position in the packed packet headers (hdr: PPM / PPT)
    uint32_t tx0, ty0, tx1, ty1;
    tile_rect(p, im.w, im.h, tile, tx0, ty0, tx1, ty1);
    const uint32_t nlayers = p.nlayers;
    const uint32_t red = g_dec_reduce;   // grk_dparameters::cp_reduce
    size_t i = data;
    // tile-component c: the tile divided by the component's subsampling (TileProcessor.cpp:116-131)
    std::vector<Comp> comps(im.nc);
    std::vector<uint32_t> tcx0(im.nc), tcy0(im.nc), tcx1(im.nc), tcy1(im.nc);
    for (uint32_t c = 0; c < im.nc; ++c) {
        tcx0[c] = ceildiv(tx0, p.sx(c)); tcy0[c] = ceildiv(ty0, p.sy(c));
        tcx1[c] = ceildiv(tx1, p.sx(c)); tcy1[c] = ceildiv(ty1, p.sy(c));
        build_geometry(comps[c], tcx0[c], tcy0[c], tcx1[c], tcy1[c], pcs[c]);
        assign_steps(comps[c], pcs[c], im.pr(c), false, &cq[c], 0, p.roi(c));
    }
    // T2 decode (LRCP)
    struct TT { std::vector<TagTree> incl, imsb; };
    std::vector<std::vector<std::vector<TT>>> trees(im.nc);
    for (uint32_t c = 0; c < im.nc; ++c) {
        trees[c].resize(pcs[c].numres);
        for (uint32_t r = 0; r < pcs[c].numres; ++r) {
            Res& R = comps[c].res[r];
            trees[c][r].resize(R.pw * R.ph);
            for (uint32_t pi = 0; pi < R.pw * R.ph; ++pi) {
                TT& t = trees[c][r][pi];
                t.incl.resize(R.bands.size()); t.imsb.resize(R.bands.size());
                for (size_t bi = 0; bi < R.bands.size(); ++bi) {
                    Precinct& P = R.bands[bi].prcs[pi];
                    if (P.cw && P.ch) { t.incl[bi].build(P.cw, P.ch); t.imsb[bi].build(P.cw, P.ch); }
                }
            }
        }
    }
    size_t pos = i;
    uint32_t npkt = 0;   // tile->numProcessedPackets: SOP's expected Nsop (T2Decompress.cpp:114, 239-246)
    for (const PktRef& pk : packet_iter(comps, p, tx0, ty0, tx1, ty1, nlayers, tpocs ? tpocs : &p.pocs)) {
                const uint32_t l = pk.l, r = pk.r, c = pk.c, pi = pk.pi;
                Res& R = comps[c].res[r];
                // layers past the limit and resolutions past the reduction: header parsed for
                // the coding state, data skipped (T2Decompress::processPacket, T2Decompress.cpp:55-116)
                const bool skip_l = (g_dec_layers && l >= g_dec_layers) || r + red >= pcs[c].numres;
                const uint32_t sty = pcs[c].cblk_sty;
                {
                    while (pos >= tile_end && next_range < ranges.size()) {
                        pos = ranges[next_range].first; tile_end = ranges[next_range].second; ++next_range;
                    }
                    if (pos >= tile_end) goto t2done;
                    if (p.sop_eph & 2) {   // SOP: FF91 0004 Nsop (T2Decompress::readPacketHeader :226-250)
                        if (tile_end - pos < 6 || cs[pos] != 0xff || cs[pos + 1] != 0x91) return -5;
                        if (get16(cs + pos + 4) != (npkt & 0xffff)) return -5;
                        pos += 6;
                    }
                    ++npkt;
                    // the header from the packed headers (PPM / PPT) when the stream has them, else
                    // in front of the body (T2Decompress.cpp:255-270)
                    BitReader br;
                    if (hdr) { br.p = hdr->data() + hpos; br.len = hdr->size() - hpos; }
                    else { br.p = cs + pos; br.len = tile_end - pos; }
                    std::vector<std::pair<Cblk*, uint32_t>> contrib;  // block, bytes in this packet
                    if (br.read(1)) {
                        for (size_t bi = 0; bi < R.bands.size(); ++bi) {
                            Band& B = R.bands[bi]; Precinct& P = B.prcs[pi];
                            if (B.empty() || P.cblks.empty()) continue;
                            TT& t = trees[c][r][pi];
                            for (size_t k = 0; k < P.cblks.size(); ++k) {
                                Cblk& K = P.cblks[k];
                                uint32_t included;
                                if (!K.included_before) {
                                    uint32_t v = t.incl[bi].decode(br, (uint32_t)k, l + 1);
                                    included = (v <= l) ? 1 : 0;
                                } else included = br.read(1);
                                if (!included) continue;
                                if (!K.included_before) {
                                    uint32_t kmsbs = 0, v = t.imsb[bi].decode(br, (uint32_t)k, kmsbs);
                                    while (v >= kmsbs) { ++kmsbs; v = t.imsb[bi].decode(br, (uint32_t)k, kmsbs); }
                                    kmsbs--;
                                    K.numbps = B.numbps - kmsbs;
                                    K.numlenbits = 3;
                                    K.included_before = true;
                                }
                                uint32_t np = br.numpasses();
                                K.numlenbits += br.commacode();
                                // codeword segments (T2Decompress.cpp:388-466): a new segment starts
                                // when the last one holds its maximum pass count
                                uint32_t nb = 0, left = np;
                                while (left) {
                                    if (K.segpasses.empty() || K.segpasses.back() == seg_maxpasses(sty, (uint32_t)K.segpasses.size() - 1)) {
                                        K.segpasses.push_back(0); K.seglens.push_back(0);
                                    }
                                    const uint32_t room = seg_maxpasses(sty, (uint32_t)K.segpasses.size() - 1) - K.segpasses.back();
                                    const uint32_t n = std::min(room, left);
                                    const uint32_t sl = br.read((int)K.numlenbits + floorlog2(n));
                                    K.segpasses.back() += n;
                                    if (!skip_l) K.seglens.back() += sl;
                                    nb += sl; left -= n;
                                }
                                if (!skip_l) K.npasses += np;
                                contrib.push_back({&K, skip_l ? ~0u - nb : nb});
                            }
                        }
                    }
                    br.align();
                    if (hdr) {
                        hpos += br.off;
                        if (hpos > hdr->size()) return -5;
                        if (p.sop_eph & 4) {   // EPH after the header, in the packed headers
                            if (hdr->size() - hpos < 2 || (*hdr)[hpos] != 0xff || (*hdr)[hpos + 1] != 0x92) return -5;
                            hpos += 2;
                        }
                    } else {
                    pos += br.off;
                    if (p.sop_eph & 4) {   // EPH after the header (:469-486)
                        if (tile_end - pos < 2 || cs[pos] != 0xff || cs[pos + 1] != 0x92) return -5;
                        pos += 2;
                    }
                    }
                    for (auto& ct : contrib) {
                        const bool skip = ct.second > 0x7fffffffu;   // skipped layer: ~bytes
                        const uint32_t want = skip ? ~ct.second : ct.second;
                        uint32_t nb = (uint32_t)std::min<size_t>(want, tile_end - pos);
                        if (!skip) ct.first->data.insert(ct.first->data.end(), cs + pos, cs + pos + nb);
                        pos += nb;
                    }
                }
            }
t2done:
    // T1 decode + dequantisation + inverse DWT + inverse MCT
    std::vector<std::vector<int32_t>> ip(im.nc);
    std::vector<std::vector<float>> fp(im.nc);
    struct Job { uint32_t c; Band* B; Cblk* K; };
    std::vector<Job> jobs;
    for (uint32_t c = 0; c < im.nc; ++c) {
        const size_t n = (size_t)comps[c].w * comps[c].h;
        if (!pcs[c].irreversible) ip[c].assign(n, 0); else fp[c].assign(n, 0.f);
        for (uint32_t r = 0; r < pcs[c].numres; ++r)
            for (auto& B : comps[c].res[r].bands)
                for (auto& P : B.prcs)
                    for (auto& K : P.cblks) jobs.push_back({c, &B, &K});
    }
    std::vector<int> jrc(jobs.size(), 0);
    par_for(jobs.size(), [&](size_t ji) {
                        const uint32_t c = jobs[ji].c;
                        Band& B = *jobs[ji].B;
                        Cblk& K = *jobs[ji].K;
                        const uint32_t TW = comps[c].w;   // tile-component row stride
                        const Params& p = pcs[c];         // the component's coding (COD / COC)
                        uint32_t w = K.x1 - K.x0, h = K.y1 - K.y0;
                        std::vector<int32_t> blk(w * h);
                        if (p.ht()) {   // T1HT::decompress: k_msbs = band numbps - cblk numbps
                            // refinement passes: Grok passes lengths2 = 0 (T1HT.cpp:169-173), which
                            // ojph_decode_codeblock rejects (ojph_block_decoder.cpp:1014-1019)
                            if (K.npasses > 1 && !K.data.empty()) { jrc[ji] = -4; return; }
                            // missing_msbs > 29: 32 bits cannot hold the samples (ojph_block_decoder.cpp:1028-1030)
                            if (K.npasses && !K.data.empty() && B.numbps - K.numbps > 29) { jrc[ji] = -4; return; }
                            if (K.npasses && !ht_decode_block(K.data.data(), (uint32_t)K.data.size(), w, h,
                                                              B.numbps - K.numbps, blk.data(), w)) {
                                jrc[ji] = -4;
                                return;
                            }
                            // ROI maxshift on the indices (standard-correct: a magnitude at or above
                            // 2^shift is the region's, scaled back down; Grok's RoiShiftHTFilter /
                            // RoiScaleHTFilter, PostDecompressFilters.h:92-158, AND the shifted
                            // magnitude with the sign bit, R-BUG-9, and are not reproduced)
                            if (const uint32_t rs = p.roi(c))
                                for (auto& v : blk) {
                                    const uint32_t m = (uint32_t)(v < 0 ? -v : v);
                                    if (m >= (1u << rs)) v = v < 0 ? -(int32_t)(m >> rs) : (int32_t)(m >> rs);
                                }
                            if (!p.irreversible) {   // ShiftHTFilter: the index is the coefficient
                                for (uint32_t y = 0; y < h; ++y)
                                    for (uint32_t x = 0; x < w; ++x)
                                        ip[c][(size_t)(B.offy + K.y0 - B.y0 + y) * TW + (B.offx + K.x0 - B.x0 + x)] = blk[y * w + x];
                                return;
                            }
                            else {
                                // ScaleHTFilter (PostDecompressFilters.h:161-176): the decoder's 32-bit
                                // sample (magnitude LSB at p = 30 - k_msbs, ojph_block_decoder.cpp:1222)
                                // times stepsize / 2^(31 - band numbps) (Quantizer.cpp:52-62).  That
                                // sample carries the centre of the bin, one bit under the magnitude
                                // (v_n |= 1, :1219): a non-zero index q is rebuilt at (q + 1/2) * step,
                                // as Grok's grk_decompress shows on these streams
                                if (B.numbps > 31) { jrc[ji] = -4; return; }
                                const uint32_t kmsbs = B.numbps - K.numbps, pp = 30 - kmsbs;
                                const float scale = B.stepsize / (float)(1u << (31 - B.numbps));
                                for (uint32_t y = 0; y < h; ++y)
                                    for (uint32_t x = 0; x < w; ++x) {
                                        const int32_t v = blk[y * w + x];
                                        const uint32_t mag = v ? ((((uint32_t)(v < 0 ? -v : v) << pp) | (1u << (pp - 1))) & 0x7fffffffu) : 0u;
                                        const float f = (float)mag * scale;
                                        const size_t o = (size_t)(B.offy + K.y0 - B.y0 + y) * TW + (B.offx + K.x0 - B.x0 + x);
                                        fp[c][o] = v < 0 ? -f : f;
                                    }
                                return;
                            }
                        } else
                        t1_decode_block(K.data.data(), (uint32_t)K.data.size(), K.npasses, K.numbps, B.orient, w, h, blk.data(),
                                        nullptr, p.cblk_sty, &K.seglens);
                        const uint32_t rs = p.roi(c);   // RoiShiftFilter / RoiScaleFilter (PostDecompressFilters.h:7-72)
                        for (uint32_t y = 0; y < h; ++y)
                            for (uint32_t x = 0; x < w; ++x) {
                                size_t o = (size_t)(B.offy + K.y0 - B.y0 + y) * TW + (B.offx + K.x0 - B.x0 + x);
                                int32_t v = blk[y * w + x];
                                if (rs && std::abs(v) >= (1 << rs)) v = v < 0 ? -(std::abs(v) >> rs) : (v >> rs);
                                if (!p.irreversible) ip[c][o] = v / 2;                 // ShiftFilter
                                else fp[c][o] = (float)v * B.stepsize / 2.0f;          // ScaleFilter
                            }
    });
    for (int rc : jrc) if (rc) return rc;
    for (uint32_t c = 0; c < im.nc; ++c) {
        Comp& C = comps[c];
        // reduced-resolution decode: the inverse transform stops at resolution numres-1-reduce,
        // whose samples sit at the tile buffer's corner (resolutions_to_decompress)
        if (!pcs[c].irreversible) dwt2d<int32_t>(ip[c].data(), C.w, C, pcs[c].numres - red, false, inv53_1d);
        else dwt2d<float>(fp[c].data(), C.w, C, pcs[c].numres - red, false, inv97_1d);
    }
    // DC level shift and clamp per component (its precision and signedness, SIZ Ssiz;
    // mct::decompress_dc_shift_rev / _irrev per component)
    auto shift_of = [&](uint32_t c) { return im.sg(c) ? 0 : (1 << (im.pr(c) - 1)); };
    auto mn_of = [&](uint32_t c) { return im.sg(c) ? -(1 << (im.pr(c) - 1)) : 0; };
    auto mx_of = [&](uint32_t c) { return im.sg(c) ? (1 << (im.pr(c) - 1)) - 1 : (int32_t)((1u << im.pr(c)) - 1); };
    // component c's reduced area: [ceil(ceil(x0 / XRsiz) / 2^r), ...) on its reduced grid, the
    // output planes back to back (one image-sized plane each without subsampling)
    std::vector<size_t> ooff(im.nc + 1, 0);
    std::vector<uint32_t> Wr(im.nc), tx0r(im.nc), ty0r(im.nc), TWr(im.nc), THr(im.nc);
    for (uint32_t c = 0; c < im.nc; ++c) {
        const uint32_t ox = ceildivpow2(ceildiv(p.x0, p.sx(c)), red), oy = ceildivpow2(ceildiv(p.y0, p.sy(c)), red);
        Wr[c] = ceildivpow2(ceildiv(p.x0 + im.w, p.sx(c)), red) - ox;
        const uint32_t Hr = ceildivpow2(ceildiv(p.y0 + im.h, p.sy(c)), red) - oy;
        ooff[c + 1] = ooff[c] + (size_t)Wr[c] * Hr;
        tx0r[c] = ceildivpow2(tcx0[c], red) - ox; ty0r[c] = ceildivpow2(tcy0[c], red) - oy;
        TWr[c] = ceildivpow2(tcx1[c], red) - ceildivpow2(tcx0[c], red); THr[c] = ceildivpow2(tcy1[c], red) - ceildivpow2(tcy0[c], red);
    }
    auto put = [&](uint32_t c, size_t k, int32_t v) {
        const uint32_t x = (uint32_t)(k % comps[c].w), y = (uint32_t)(k / comps[c].w);
        if (x >= TWr[c] || y >= THr[c]) return;
        out[ooff[c] + (size_t)(ty0r[c] + y) * Wr[c] + tx0r[c] + x] = std::min(mx_of(c), std::max(mn_of(c), v + shift_of(c)));
    };
    // the inverse MCT needs the first three tile-components of one size (needsMctDecompress,
    // TileProcessor.cpp:432-456: Grok skips it with a warning otherwise)
    const bool mct = p.mct && im.nc >= 3 && comps[1].w == comps[0].w && comps[2].w == comps[0].w &&
                     comps[1].h == comps[0].h && comps[2].h == comps[0].h;
    const size_t n = (size_t)comps[0].w * comps[0].h;
    auto nof = [&](uint32_t c) { return (size_t)comps[c].w * comps[c].h; };
    if (mct && !pcs[0].irreversible)
        for (size_t k = 0; k < n; ++k) {
            int32_t y = ip[0][k], u = ip[1][k], v = ip[2][k];
            int32_t g = y - ((u + v) >> 2), rr = v + g, b = u + g;
            ip[0][k] = rr; ip[1][k] = g; ip[2][k] = b;
        }
    if (mct && pcs[0].irreversible)
        for (size_t k = 0; k < n; ++k) {
            float y = fp[0][k], u = fp[1][k], v = fp[2][k];
            fp[0][k] = y + 1.402f * v;
            fp[1][k] = y - 0.34413f * u - 0.71414f * v;
            fp[2][k] = y + 1.772f * u;
        }
    for (uint32_t c = 0; c < im.nc; ++c)   // (each component by its own transform)
        for (size_t k = 0; k < nof(c); ++k) put(c, k, pcs[c].irreversible ? (int32_t)lrintf(fp[c][k]) : ip[c][k]);
    return 0;
}

// COC / QCC and tile-part COD / QCD (CodeStreamDecompress read_coc / read_qcc override the main
// COD / QCD per component or per tile).
// ccod: each component's coding as a COC body would state it (Scoc precinct flag, then SPcoc):
// its main COC, else the COD's
static std::vector<uint8_t> cod_as_coc(const std::vector<uint8_t>& cod) {
    std::vector<uint8_t> v{(uint8_t)(cod[0] & 1)};
    v.insert(v.end(), cod.begin() + 5, cod.end());
    return v;
}
// COD body (Scod, SGcod, SPcod; CodeStreamDecompress::read_cod :2521-2623) into the stream-level
// fields of p (SOP / EPH, layers, MCT, progression) and its default coding; false when malformed
// or not restated here (a Part-2 array MCT)
static bool read_cod(const std::vector<uint8_t>& v, Params& p) {
    if (v.size() < 10) return false;
    const uint8_t* s = v.data();
    const uint32_t scod = s[0];
    if (scod & ~7u) return false;            // unknown Scod bits (read_cod :2548)
    p.sop_eph = scod & 6;
    p.nlayers = get16(s + 2); p.mct = s[4];
    if (!p.nlayers || p.mct > 1) return false;   // (MCT 2: Part-2 decompress_custom, not restated)
    p.numres = s[5] + 1; p.cbw_exp = s[6] + 2; p.cbh_exp = s[7] + 2; p.irreversible = s[9] == 0;
    p.cblk_sty = s[8];
    if (s[1] > 4) return false;                                   // progression order
    p.prog = s[1];
    if ((s[8] & 0x40) && s[8] != 0x40) return false;  // HT with Part-1 mode switches (CodeStreamDecompress.cpp:1781)
    if (s[8] & 0x80) return false;
    if (p.numres > 33 || p.cbw_exp > 10 || p.cbh_exp > 10 || p.cbw_exp + p.cbh_exp > 12) return false;
    for (uint32_t r = 0; r < 33; ++r) { p.prcw_exp[r] = 15; p.prch_exp[r] = 15; }
    if (scod & 1) {
        if (v.size() < 10 + p.numres) return false;
        for (uint32_t r = 0; r < p.numres; ++r) { p.prcw_exp[r] = s[10 + r] & 15; p.prch_exp[r] = s[10 + r] >> 4; }
    }
    return prc_exps_ok(p);
}

// A tile's coding and quantisation: the main header's (cod, ccod, qbody) changed by the COD / COC /
// QCD / QCC of its tile-part headers.  The tile's tcp starts as a copy of the main header's; read_cod
// (CodeStreamDecompress.cpp:2521-2623) sets the tile's stream fields and copies its SPcod to every
// component, read_coc (:2631-2670) sets one component's, both in marker order; quantisation follows
// read_SQcd_SQcc's scoping (Quantizer.cpp:208-235): a tile QCC wins over a tile QCD, which wins over
// the main header's QCC / QCD, in any marker order.
// A tile-part RGN sets the tile's ROI shift of its component (read_rgn, :1476-1520).
struct TileCoding { std::vector<uint8_t> cod; std::vector<std::vector<uint8_t>> ccod, qbody; std::vector<uint32_t> roi; };
static bool tile_coding(const std::vector<std::pair<uint32_t, std::vector<uint8_t>>>& marks, uint32_t nc, TileCoding& tc) {
    const uint32_t cw = nc <= 256 ? 1 : 2;
    std::vector<uint8_t> tqcc(nc, 0);
    for (const auto& mk : marks) {
        const std::vector<uint8_t>& v = mk.second;
        if (mk.first == 0xff52) {
            if (v.size() < 10) return false;
            tc.cod = v;
            for (auto& q : tc.ccod) q = cod_as_coc(v);
        } else if (mk.first == 0xff5c) {
            if (v.size() < 2) return false;
            for (uint32_t c = 0; c < nc; ++c) if (!tqcc[c]) tc.qbody[c] = v;
        } else if (mk.first == 0xff5e) {   // Crgn, Srgn (0: implicit), SPrgn (< 32)
            if (v.size() != cw + 2) return false;
            const uint32_t c = cw == 1 ? v[0] : get16(v.data());
            if (c >= nc || v[cw] != 0 || v[cw + 1] >= 32) return false;
            tc.roi[c] = v[cw + 1];
        } else {
            if (v.size() < cw + 2) return false;
            const uint32_t c = cw == 1 ? v[0] : get16(v.data());
            if (c >= nc) return false;
            std::vector<uint8_t> b(v.begin() + cw, v.end());
            if (mk.first == 0xff5d) { tc.qbody[c] = std::move(b); tqcc[c] = 1; }
            else { if (b.size() < 6) return false; tc.ccod[c] = std::move(b); }
        }
    }
    return true;
}

// A component's coding parameters from its COC-form body (Scoc, SPcoc: decomposition levels,
// code-block size and style, transform, [precinct sizes]; CodeStreamDecompress read_coc /
// read_SPCod_SPCoc), over the stream's parameters; false when malformed
static bool comp_params(const std::vector<uint8_t>& v, Params& pc) {
    if (v.size() < 6) return false;
    pc.numres = v[1] + 1u; pc.cbw_exp = v[2] + 2u; pc.cbh_exp = v[3] + 2u; pc.cblk_sty = v[4];
    pc.irreversible = v[5] == 0;
    if (pc.numres > 33 || pc.cbw_exp > 10 || pc.cbh_exp > 10 || pc.cbw_exp + pc.cbh_exp > 12) return false;
    if ((pc.cblk_sty & 0x40) && pc.cblk_sty != 0x40) return false;
    if (pc.cblk_sty & 0x80) return false;
    for (uint32_t r = 0; r < 33; ++r) { pc.prcw_exp[r] = 15; pc.prch_exp[r] = 15; }
    if (v[0] & 1) {
        if (v.size() < 6 + pc.numres) return false;
        for (uint32_t r = 0; r < pc.numres; ++r) { pc.prcw_exp[r] = v[6 + r] & 15; pc.prch_exp[r] = v[6 + r] >> 4; }
    }
    return prc_exps_ok(pc);
}

// A tile part's end from its Psot, checked: the next SOT (Lsot 10, a tile index below nt) or
// EOC must start there, or the data end.  Grok writes Psot from its rate-control simulation's
// count when its BitIO swallowed a failure, a few bytes off the part's
// real length; the nearest such marker within 8 bytes is taken instead.
static size_t resync_part_end(const uint8_t* cs, size_t len, size_t pos, size_t end, uint32_t nt) {
    auto ok = [&](size_t q) {
        if (q == len || (q + 2 == len && get16(cs + q) == 0xffd9)) return true;
        return q + 12 <= len && get16(cs + q) == 0xff90 && get16(cs + q + 2) == 10 && get16(cs + q + 4) < nt;
    };
    if (end <= len && ok(end)) return end;
    for (size_t d = 1; d <= 8; ++d) {
        if (end >= pos + 14 + d && end - d <= len && ok(end - d)) return end - d;
        if (end + d <= len && ok(end + d)) return end + d;
    }
    return end;
}

// the (reduced) plane sizes of the last orc_decode's components, (w, h) each; returns the count
static thread_local std::vector<uint32_t> t_comp_dims;
static thread_local std::vector<uint32_t> t_comp_prec;   // precision | signed << 8 per component
uint32_t orc_last_comp_prec(uint32_t* out) {
    if (out) std::copy(t_comp_prec.begin(), t_comp_prec.end(), out);
    return (uint32_t)t_comp_prec.size();
}
uint32_t orc_last_comp_dims(uint32_t* out) {
    if (out) std::copy(t_comp_dims.begin(), t_comp_dims.end(), out);
    return (uint32_t)(t_comp_dims.size() / 2);
}
// the next decodes as through a decode window (Grok's partial-tile inverse), or not
extern "C" void orc_set_partial(int on) { g_partial_inverse = on != 0; }
// the inverse 5/3 of a single-sample line holding v (test hook for the rule above)
extern "C" int32_t orc_inv53_single(int32_t v, uint32_t par, int vertical, int partial) {
    const bool was = g_partial_inverse;
    g_partial_inverse = partial != 0;
    std::vector<int32_t> tmp;
    inv53_1d(&v, 1, tmp, par, vertical != 0);
    g_partial_inverse = was;
    return v;
}
int orc_decode(const uint8_t* cs, size_t len, int32_t* out, uint32_t* W, uint32_t* H, uint32_t* NC, uint32_t* PREC) {
    size_t i = 0;
    if (len >= 12 && get32(cs) == 12 && get32(cs + 4) == 0x6a502020) {   // JP2: find the jp2c box
        size_t pos = 12;
        bool found = false;
        while (pos + 8 <= len) {
            uint64_t L = get32(cs + pos);
            size_t hdr = 8;
            if (L == 1) { L = ((uint64_t)get32(cs + pos + 8) << 32) | get32(cs + pos + 12); hdr = 16; }
            else if (L == 0) L = len - pos;
            if (L < hdr || L > len - pos) return -6;
            if (get32(cs + pos + 4) == 0x6a703263) { cs += pos + hdr; len = (size_t)L - hdr; found = true; break; }
            pos += (size_t)L;
        }
        if (!found) return -6;
    }
    if (len < 4 || get16(cs) != 0xff4f) return -1;
    i = 2;
    Image im{}; Params p; p.write_com = 0;
    size_t first_sot = 0;
    std::vector<uint8_t> cod_body, qcd_body;
    std::vector<size_t> coc_qcc;
    std::vector<std::pair<uint32_t, std::vector<uint8_t>>> qccs;   // main-header QCC: (component, Sqcc + SPqcc)
    std::map<uint32_t, std::vector<uint8_t>> ppm;                   // PPM bodies by Zppm
    while (i + 4 <= len) {
        uint32_t m = get16(cs + i);
        if (m == 0xff90) { first_sot = i; break; }
        uint32_t L = get16(cs + i + 2);
        const uint8_t* s = cs + i + 4;
        if (m == 0xff51) {
            im.w = get32(s + 2) - get32(s + 10); im.h = get32(s + 6) - get32(s + 14);
            p.x0 = get32(s + 10); p.y0 = get32(s + 14); p.gx0 = get32(s + 26); p.gy0 = get32(s + 30);
            // B.3: the tile grid origin lies at or above-left of the image origin, its first tile reaches it
            p.tw = get32(s + 18); p.th = get32(s + 22);
            if (get32(s + 2) <= p.x0 || get32(s + 6) <= p.y0 || p.gx0 > p.x0 || p.gy0 > p.y0 || !p.tw || !p.th ||
                (uint64_t)p.gx0 + p.tw <= p.x0 || (uint64_t)p.gy0 + p.th <= p.y0)
                return -2;
            im.nc = get16(s + 34);
            if (!im.nc || L < 38 + 3 * im.nc) return -2;
            im.prec = (s[36] & 0x7f) + 1; im.sgnd = (s[36] & 0x80) != 0;
            im.cprec.assign(im.nc, 0); im.csgnd.assign(im.nc, 0);
            for (uint32_t c = 0; c < im.nc; ++c) {   // Ssiz per component (1..38 bits; 31 here)
                im.cprec[c] = (s[36 + 3 * c] & 0x7f) + 1u; im.csgnd[c] = (s[36 + 3 * c] & 0x80) != 0;
                if (im.cprec[c] > 31) return -2;
            }
            p.cdx.assign(im.nc, 1); p.cdy.assign(im.nc, 1);
            for (uint32_t c = 0; c < im.nc; ++c) {   // XRsiz / YRsiz (1..255)
                p.cdx[c] = s[37 + 3 * c]; p.cdy[c] = s[38 + 3 * c];
                if (!p.cdx[c] || !p.cdy[c]) return -2;
            }
        } else if (m == 0xff52) {
            cod_body.assign(s, s + L - 2);
            if (!read_cod(cod_body, p)) return -2;
        } else if (m == 0xff5f) {
            if (!read_poc(s, L, im.nc, p.pocs)) return -2;
        } else if (m == 0xff5e) {                          // RGN: Crgn, Srgn (0), SPrgn
            const uint32_t cw = im.nc <= 256 ? 1 : 2;
            const uint32_t c = cw == 1 ? s[0] : get16(s);
            if (L != 4 + cw || c >= im.nc || s[cw] != 0 || s[cw + 1] >= 32) return -2;
            if (p.roishift.size() < im.nc) p.roishift.resize(im.nc, 0);
            p.roishift[c] = s[cw + 1];
        } else if (m == 0xff5c) {
            if (L < 3) return -2;
            p.numgbits = s[0] >> 5;
            qcd_body.assign(s, s + L - 2);
        } else if (m == 0xff5d) {   // QCC (A.6.5): this component's quantisation replaces the QCD's
            const uint32_t cw = im.nc <= 256 ? 1 : 2;
            if (!im.nc || L < 3 + cw) return -2;
            const uint32_t c = cw == 1 ? s[0] : get16(s);
            if (c >= im.nc) return -2;
            qccs.push_back({c, std::vector<uint8_t>(s + cw, s + L - 2)});
        } else if (m == 0xff53) {
            coc_qcc.push_back(i);
        } else if (m == 0xff72 || m == 0xff73 || (m >= 0xff74 && m <= 0xff79)) {
            return -2;   // Part-2 extension markers (ISO 15444-2 A.2): not restated
        } else if (m == 0xff60) {   // PPM (A.7.4): Zppm, then (Nppm, Ippm) runs (PPMMarker::read)
            if (L < 3) return -2;
            if (!ppm.emplace(s[0], std::vector<uint8_t>(s + 1, s + L - 2)).second) return -2;   // Zppm read twice
        }
        i += 2 + L;   // CAP, TLM, COM and other main-header markers are skipped
    }
    if (!first_sot || qcd_body.empty()) return -3;
    // per component: the QCD's quantisation, replaced by a main-header QCC (read_SQcd_SQcc with
    // Grok's precedence: a main QCC wins over the main QCD, Quantizer.cpp:215-235)
    std::vector<std::vector<uint8_t>> qbody(im.nc, qcd_body);
    for (const auto& q : qccs) qbody[q.first] = q.second;
    // per component: the COD's coding, replaced by its main-header COC (A.6.2; Grok's read_coc
    // fills the component's tccp, a main COC winning over the main COD in either order)
    if (cod_body.size() < 10) return -3;
    std::vector<std::vector<uint8_t>> ccod(im.nc, cod_as_coc(cod_body));
    for (size_t k : coc_qcc) {
        const uint32_t L = get16(cs + k + 2), cw = im.nc <= 256 ? 1 : 2;
        if (L < 2 + cw + 6) return -2;
        const uint8_t* b = cs + k + 4;
        const uint32_t c = cw == 1 ? b[0] : get16(b);
        if (c >= im.nc) return -2;
        ccod[c].assign(b + cw, b + L - 2);
    }
    // a tile's parameters from its coding: stream fields from its COD, each component's from its
    // COC-form body, quantisation per component; 0, or the error code
    auto setup = [&](const TileCoding& tc, Params& pt, std::vector<Params>& pcs_t, std::vector<Quant>& cq_t,
                     uint32_t& min_res) -> int {
        if (!read_cod(tc.cod, pt)) return -2;
        pt.roishift = tc.roi;
        pcs_t.assign(im.nc, pt);
        min_res = 33;
        for (uint32_t c = 0; c < im.nc; ++c) {
            if (!comp_params(tc.ccod[c], pcs_t[c])) return -2;
            min_res = std::min(min_res, pcs_t[c].numres);
        }
        // the inverse MCT picks RCT / ICT by component 0's transform (TileProcessor::mctDecompress):
        // first three components coded with different transforms are refused
        if (pt.mct && im.nc >= 3 && (pcs_t[1].irreversible != pcs_t[0].irreversible || pcs_t[2].irreversible != pcs_t[0].irreversible))
            return -2;
        // (an MCT over components of different precisions or signs: refused, as by the engine)
        if (pt.mct && im.nc >= 3 && (im.pr(1) != im.pr(0) || im.pr(2) != im.pr(0) || im.sg(1) != im.sg(0) || im.sg(2) != im.sg(0)))
            return -2;
        cq_t.assign(im.nc, Quant());
        for (uint32_t c = 0; c < im.nc; ++c)
            if (!parse_quant(tc.qbody[c].data(), tc.qbody[c].size(), pcs_t[c].numres, cq_t[c])) return -2;
        return g_dec_reduce >= min_res ? -7 : 0;   // reduce must leave one resolution of every component
    };
    std::vector<uint32_t> main_roi(im.nc, 0);
    for (uint32_t c = 0; c < im.nc; ++c) main_roi[c] = p.roi(c);
    const TileCoding main_tc{cod_body, ccod, qbody, main_roi};
    std::vector<Params> pcs;
    std::vector<Quant> cq;
    uint32_t min_res = 33;
    if (int rc = setup(main_tc, p, pcs, cq, min_res)) return rc;
    if (g_dec_reduce >= min_res) return -7;   // reduce must leave one resolution of every component
    *W = ceildivpow2(p.x0 + im.w, g_dec_reduce) - ceildivpow2(p.x0, g_dec_reduce);
    *H = ceildivpow2(p.y0 + im.h, g_dec_reduce) - ceildivpow2(p.y0, g_dec_reduce);
    *NC = im.nc; *PREC = im.prec;
    // each component's (reduced) plane size: orc_last_comp_dims
    t_comp_dims.clear();
    t_comp_prec.clear();
    for (uint32_t c = 0; c < im.nc; ++c) t_comp_prec.push_back(im.pr(c) | (im.sg(c) ? 0x100u : 0u));
    size_t total = 0;
    for (uint32_t c = 0; c < im.nc; ++c) {
        const uint32_t sx = p.sx(c), sy = p.sy(c);
        const uint32_t cw = ceildivpow2(ceildiv(p.x0 + im.w, sx), g_dec_reduce) - ceildivpow2(ceildiv(p.x0, sx), g_dec_reduce);
        const uint32_t ch = ceildivpow2(ceildiv(p.y0 + im.h, sy), g_dec_reduce) - ceildivpow2(ceildiv(p.y0, sy), g_dec_reduce);
        t_comp_dims.push_back(cw); t_comp_dims.push_back(ch);
        total += (size_t)cw * ch;
    }
    if (!out) return 0;
    if (p.gx0 + p.tw >= p.x0 + im.w && p.gy0 + p.th >= p.y0 + im.h) p.tw = p.th = 0;   // one tile
    std::fill(out, out + total, 0);
    const uint32_t nt = tile_count(p, im.w, im.h);
    size_t pos = first_sot;
    struct Part { size_t data, end; uint32_t tile, tpsot; std::vector<PocE> pocs;
                  std::vector<std::pair<uint32_t, std::vector<uint8_t>>> ppt, marks; };
    std::vector<Part> parts;
    while (pos + 12 <= len && get16(cs + pos) == 0xff90) {
        const uint8_t* s = cs + pos + 4;
        uint32_t isot = get16(s), psot = get32(s + 2);
        size_t tile_end = psot ? pos + psot : len - 2;
        if (tile_end > len + 8 || isot >= nt) return -5;
        tile_end = resync_part_end(cs, len, pos, tile_end, nt);
        if (tile_end > len) return -5;
        size_t j = pos + 12;   // tile-part header markers (PLT, POC, ...) until SOD
        std::vector<PocE> tp_pocs;
        std::vector<std::pair<uint32_t, std::vector<uint8_t>>> tp_ppt, tp_marks;
        while (j + 2 <= tile_end && get16(cs + j) != 0xff93) {
            const uint32_t tm = get16(cs + j);
            if (tm == 0xff61) {   // PPT (A.7.5): Zppt, Ippt; not with PPM (read_ppt's error)
                const uint32_t Lp = get16(cs + j + 2);
                if (Lp < 3 || !ppm.empty()) return -2;
                tp_ppt.push_back({cs[j + 4], std::vector<uint8_t>(cs + j + 5, cs + j + 2 + Lp)});
            }
            if (tm == 0xff5f && !read_poc(cs + j + 4, get16(cs + j + 2), im.nc, tp_pocs)) return -5;
            if (tm == 0xff52 || tm == 0xff53 || tm == 0xff5c || tm == 0xff5d || tm == 0xff5e) {   // the tile's coding / quantisation / ROI
                const uint32_t Lm = get16(cs + j + 2);
                if (Lm < 3 || j + 2 + Lm > tile_end) return -5;
                tp_marks.push_back({tm, std::vector<uint8_t>(cs + j + 4, cs + j + 2 + Lm)});
            }
            j += 2 + get16(cs + j + 2);
        }
        if (j + 2 > tile_end) return -5;
        parts.push_back({j + 2, tile_end, isot, s[6], std::move(tp_pocs), std::move(tp_ppt), std::move(tp_marks)});
        pos = tile_end;
    }
    // a tile's parts in order (TPsot 0, 1, ...)
    std::vector<uint32_t> tiles;
    std::vector<std::vector<std::pair<size_t, size_t>>> ranges;
    // a tile's progression order changes: the main header's list, extended by the POC of each of
    // its tile-part headers in turn (read_poc appends to the tile's tcp, a copy of the main
    // header's, CodeStreamDecompress.cpp:1171-1172; OpenJPEG's opj_j2k_read_poc does the same)
    std::vector<std::vector<PocE>> tpocs;
    std::vector<int> slot(nt, -1);
    for (Part& q : parts) {
        if (slot[q.tile] < 0) {
            if (q.tpsot != 0) return -5;
            slot[q.tile] = (int)tiles.size(); tiles.push_back(q.tile); ranges.emplace_back();
            tpocs.push_back(p.pocs);
        } else if (q.tpsot != ranges[slot[q.tile]].size()) return -5;
        std::vector<PocE>& tl = tpocs[slot[q.tile]];
        tl.insert(tl.end(), q.pocs.begin(), q.pocs.end());
        if (tl.size() > 33) return -5;   // GRK_J2K_MAXRLVLS progressions (read_poc :1173-1178)
        ranges[slot[q.tile]].push_back({q.data, q.end});
    }
    // packed packet headers per tile: PPT markers of the tile's parts in Zppt order (merge_ppt, one
    // index space per tile), or PPM's Nppm runs, the k-th taken by tile k (T2Decompress.cpp:257-266
    // indexes m_tile_packet_headers by tile: kept to one tile part per tile here)
    std::vector<std::vector<uint8_t>> hdrs(tiles.size());
    std::vector<uint8_t> has_hdr(tiles.size(), 0);
    if (!ppm.empty()) {
        std::vector<uint8_t> v;
        for (auto& kv : ppm) v.insert(v.end(), kv.second.begin(), kv.second.end());
        std::vector<std::vector<uint8_t>> runs;
        for (size_t at = 0; at < v.size();) {
            if (v.size() - at < 4) return -2;
            const uint32_t n = get32(v.data() + at);
            at += 4;
            if (v.size() - at < n) return -2;
            runs.emplace_back(v.begin() + at, v.begin() + at + n);
            at += n;
        }
        for (size_t q = 0; q < tiles.size(); ++q) {
            if (ranges[q].size() != 1 || tiles[q] >= runs.size()) return -2;
            hdrs[q] = runs[tiles[q]]; has_hdr[q] = 1;
        }
    }
    for (const Part& pt : parts)
        if (!pt.ppt.empty()) has_hdr[(size_t)slot[pt.tile]] = 1;
    for (size_t q = 0; q < tiles.size(); ++q) {
        if (!has_hdr[q] || !ppm.empty()) continue;
        std::map<uint32_t, std::vector<uint8_t>> z;
        for (const Part& pt : parts)
            if (pt.tile == tiles[q])
                for (const auto& e : pt.ppt) if (!z.emplace(e.first, e.second).second) return -2;   // Zppt read twice
        for (auto& kv : z) hdrs[q].insert(hdrs[q].end(), kv.second.begin(), kv.second.end());
    }
    // tiles with COD / COC / QCD / QCC in their tile-part headers: their own parameters
    struct TileParams { Params p; std::vector<Params> pcs; std::vector<Quant> cq; };
    std::vector<std::unique_ptr<TileParams>> own(tiles.size());
    for (size_t q = 0; q < tiles.size(); ++q) {
        std::vector<std::pair<uint32_t, std::vector<uint8_t>>> marks;
        for (const Part& pt : parts)
            if (pt.tile == tiles[q]) marks.insert(marks.end(), pt.marks.begin(), pt.marks.end());
        if (marks.empty()) continue;
        TileCoding tc = main_tc;
        if (!tile_coding(marks, im.nc, tc)) return -2;
        if (tc.cod == main_tc.cod && tc.ccod == main_tc.ccod && tc.qbody == main_tc.qbody && tc.roi == main_tc.roi)
            continue;   // restated
        own[q].reset(new TileParams{p, {}, {}});
        uint32_t tmin = 33;
        if (int rc = setup(tc, own[q]->p, own[q]->pcs, own[q]->cq, tmin)) return rc;
        own[q]->p.pocs = p.pocs;
    }
    std::vector<int> rcs(tiles.size(), 0);   // tiles write disjoint rectangles of out
    par_for(tiles.size(), [&](size_t q) {
        const TileParams* o = own[q].get();
        rcs[q] = decode_tile(cs, ranges[q], o ? o->p : p, o ? o->pcs : pcs, im, o ? o->cq : cq, tiles[q], out, &tpocs[q],
                             has_hdr[q] ? &hdrs[q] : nullptr);
    });
    for (int rc : rcs) if (rc) return rc;
    return 0;
}

}  // extern "C"
