// gk_icc.h — the ICC profiles a JP2 colr box may carry (METH 2: Part 1 restricts it to the
// Monochrome Input and Three-Component Matrix-Based Input classes), read into a small transform
// description: a tone curve per channel and a 3 x 3 matrix into linear sRGB.  Host code with no
// HIP dependency (tools/icc_check.cpp compiles it alone); every offset is checked against the
// profile before it is read, and a profile this reader does not hold is refused by a message
// that names the reason.
//
// The transform is what lcms2 builds for such a profile against its built-in sRGB profile
// (cmsCreateTransform as color_apply_icc_profile calls it, bin/common/color.cpp:423-776):
// curve -> profile colorants -> inverse of the sRGB colorants -> clip to [0, 1] -> sRGB encoding.
// The header's rendering intent does not change it for these profile classes.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>

struct GkIccCurve {
    enum Kind { IDENTITY = 0, PARA = 1, TABLE = 2 } kind = IDENTITY;
    // PARA: y = x >= d ? pow(a * x + b, g) + e : c * x + f (`para` types 0-4 and a `curv` gamma
    // all reduce to it)
    double g = 1, a = 1, b = 0, c = 0, d = 0, e = 0, f = 0;
    // TABLE: 2..32767 entries over [0, 1], read as lcms2 reads a 16-bit table (cmsEvalToneCurveFloat ->
    // LinLerp1D, cmsintrp.c): the input rounded to 16 bits, fixed-point linear interpolation, a
    // 16-bit result
    std::vector<uint16_t> table;
    // the 16-bit input word of sample v of a precision whose largest value is vmax: v * 65535 / vmax, rounded half up
    static uint32_t in16(uint32_t v, uint32_t vmax) { return (uint32_t)((2ull * v * 65535ull + vmax) / (2ull * vmax)); }
    // LinLerp1D on table entries e(i), i < n
    template <class E> static uint32_t lerp16(uint32_t in, uint32_t n, E e) {
        if (in == 0xffffu) return e(n - 1);
        uint32_t v3 = (n - 1) * in;
        v3 = v3 + (v3 + 0x7fffu) / 0xffffu;   // _cmsToFixedDomain
        const uint32_t cell = v3 >> 16, rest = v3 & 0xffffu;
        const uint32_t y0 = e(cell), y1 = e(cell + 1);
        return ((((y1 - y0) * rest + 0x8000u) >> 16) + y0) & 0xffffu;   // LinearInterp (unsigned wrap as in lcms2)
    }
    // the curve's value for sample v of [0, vmax]
    double eval(uint32_t v, uint32_t vmax) const {
        const double x = (double)v / (double)vmax;
        if (kind == IDENTITY) return x;
        if (kind == PARA) return x >= d ? pow(a * x + b, g) + e : c * x + f;
        return (double)lerp16(in16(v, vmax), (uint32_t)table.size(), [&](uint32_t i) { return (uint32_t)table[i]; }) / 65535.0;
    }
};
struct GkIccTransform {
    bool grey = false;          // GRAY + kTRC: R = G = B = encoding(curve(v))
    GkIccCurve curve[3];        // grey: curve[0]
    double colorant[3][3] = {}; // rows X, Y, Z; columns rXYZ, gXYZ, bXYZ
    double m[3][3] = {};        // inverse(sRGB colorants) x colorant: curve output -> linear sRGB
    uint32_t intent = 0;
};

// lcms2's built-in sRGB colorants (cmsCreate_sRGBProfile: Rec. 709 primaries adapted to D50 and
// rounded to s15Fixed16), rows X, Y, Z
static const double GK_SRGB_COLORANTS[3][3] = {{0.43604125, 0.38511291, 0.14304584},
                                               {0.22248454, 0.71690508, 0.06061038},
                                               {0.01392019, 0.09706724, 0.71391257}};
// the sRGB encoding of a linear value (clipped to [0, 1] by the caller)
static inline double gk_srgb_encode(double v) { return v <= 0.0031308 ? 12.92 * v : 1.055 * pow(v, 1.0 / 2.4) - 0.055; }
static inline void gk_inv3(const double s[3][3], double o[3][3]) {
    const double det = s[0][0] * (s[1][1] * s[2][2] - s[1][2] * s[2][1]) - s[0][1] * (s[1][0] * s[2][2] - s[1][2] * s[2][0]) +
                       s[0][2] * (s[1][0] * s[2][1] - s[1][1] * s[2][0]);
    o[0][0] = (s[1][1] * s[2][2] - s[1][2] * s[2][1]) / det; o[0][1] = (s[0][2] * s[2][1] - s[0][1] * s[2][2]) / det;
    o[0][2] = (s[0][1] * s[1][2] - s[0][2] * s[1][1]) / det; o[1][0] = (s[1][2] * s[2][0] - s[1][0] * s[2][2]) / det;
    o[1][1] = (s[0][0] * s[2][2] - s[0][2] * s[2][0]) / det; o[1][2] = (s[0][2] * s[1][0] - s[0][0] * s[1][2]) / det;
    o[2][0] = (s[1][0] * s[2][1] - s[1][1] * s[2][0]) / det; o[2][1] = (s[0][1] * s[2][0] - s[0][0] * s[2][1]) / det;
    o[2][2] = (s[0][0] * s[1][1] - s[0][1] * s[1][0]) / det;
}

namespace gk_icc_detail {
static inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
static inline uint32_t be16(const uint8_t* p) { return ((uint32_t)p[0] << 8) | p[1]; }
static inline double s15f16(const uint8_t* p) { return (double)(int32_t)be32(p) / 65536.0; }
static inline uint32_t sig(const char* s) { return be32((const uint8_t*)s); }
static inline std::string sig_name(uint32_t v) {
    std::string s;
    for (int k = 3; k >= 0; --k) { const char ch = (char)(v >> (8 * k)); s += (ch >= 32 && ch < 127) ? ch : '?'; }
    return s;
}
struct Tag { uint32_t off = 0, size = 0; bool found = false; };
}  // namespace gk_icc_detail

// Reads profile p[0, n) into T.  Returns "" or the reason the profile is refused.
static inline std::string gk_icc_read(const uint8_t* p, size_t n, GkIccTransform& T) {
    using namespace gk_icc_detail;
    T = GkIccTransform();
    if (!p || n < 132) return "not a profile: " + std::to_string(n) + " bytes are too few for a header and a tag count";
    if (be32(p + 36) != sig("acsp")) return "not a profile: no 'acsp' signature";
    const uint32_t size = be32(p);
    if (size > n) return "not a profile: its size field (" + std::to_string(size) + ") runs past the box (" + std::to_string(n) + " bytes)";
    if (size < 132) return "not a profile: its size field (" + std::to_string(size) + ") is too small";
    const uint32_t space = be32(p + 16), pcs = be32(p + 20);
    T.intent = be32(p + 64);
    const uint32_t ntags = be32(p + 128);
    if (ntags > (size - 132) / 12) return "not a profile: a tag table of " + std::to_string(ntags) + " entries runs past the profile";
    auto find = [&](const char* name, Tag& t) -> std::string {
        const uint32_t want = sig(name);
        for (uint32_t i = 0; i < ntags; ++i) {
            const uint8_t* e = p + 132 + (size_t)12 * i;
            if (be32(e) != want) continue;
            t.off = be32(e + 4); t.size = be32(e + 8); t.found = true;
            if (t.off > size || t.size > size - t.off) return std::string("not a profile: tag '") + name + "' lies outside the profile";
            return "";
        }
        return "";
    };
    for (const char* lut : {"A2B0", "A2B1", "A2B2"}) {
        Tag t;
        const std::string r = find(lut, t);
        if (!r.empty()) return r;
        if (t.found) return std::string("a profile with a lookup table (tag '") + lut + "') is not supported: only matrix / tone-curve profiles are";
    }
    if (space != sig("RGB ") && space != sig("GRAY"))
        return "a profile for the data colour space '" + sig_name(space) + "' is not supported (only 'RGB ' and 'GRAY' are)";
    if (pcs != sig("XYZ ")) return "a profile with the connection space '" + sig_name(pcs) + "' is not supported (only 'XYZ ' is)";
    auto curve = [&](const char* name, GkIccCurve& C) -> std::string {
        Tag t;
        std::string r = find(name, t);
        if (!r.empty()) return r;
        if (!t.found) return std::string("the profile has no '") + name + "' tag";
        if (t.size < 12) return std::string("not a profile: tag '") + name + "' is too short for a curve";
        const uint8_t* q = p + t.off;
        const uint32_t type = be32(q);
        if (type == sig("curv")) {
            const uint32_t cnt = be32(q + 8);
            if (cnt > (t.size - 12) / 2) return std::string("not a profile: the curve count of tag '") + name + "' (" + std::to_string(cnt) + ") overruns the tag";
            if (cnt == 0) { C.kind = GkIccCurve::IDENTITY; return ""; }
            if (cnt == 1) { C.kind = GkIccCurve::PARA; C.g = (double)be16(q + 12) / 256.0; return ""; }
            if (cnt > 0x7fff) return std::string("tag '") + name + "': a curve table of " + std::to_string(cnt) + " entries (lcms2 reads at most 32767)";
            C.kind = GkIccCurve::TABLE;
            C.table.resize(cnt);
            for (uint32_t i = 0; i < cnt; ++i) C.table[i] = (uint16_t)be16(q + 12 + 2 * (size_t)i);
            return "";
        }
        if (type == sig("para")) {
            const uint32_t ft = be16(q + 8);
            static const uint32_t np[5] = {1, 3, 4, 5, 7};
            if (ft > 4) return std::string("tag '") + name + "': parametric curve type " + std::to_string(ft) + " is not supported (0..4 are)";
            if (t.size < 12 + 4 * np[ft]) return std::string("not a profile: the parameters of tag '") + name + "' overrun the tag";
            double v[7] = {0, 0, 0, 0, 0, 0, 0};
            for (uint32_t i = 0; i < np[ft]; ++i) v[i] = s15f16(q + 12 + 4 * (size_t)i);
            C.kind = GkIccCurve::PARA;
            C.g = v[0];
            if (ft == 0) return "";
            C.a = v[1]; C.b = v[2];
            if (ft <= 2) {
                if (C.a == 0) return std::string("tag '") + name + "': a parametric curve with a = 0";
                C.d = -C.b / C.a;
                if (ft == 2) { C.e = v[3]; C.f = v[3]; }
                return "";
            }
            C.c = v[3]; C.d = v[4];
            if (ft == 4) { C.e = v[5]; C.f = v[6]; }
            return "";
        }
        return std::string("tag '") + name + "': the curve type '" + sig_name(type) + "' is not supported ('curv' and 'para' are)";
    };
    if (space == sig("GRAY")) {
        T.grey = true;
        const std::string r = curve("kTRC", T.curve[0]);
        if (!r.empty()) return r;
        T.curve[1] = T.curve[2] = T.curve[0];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) T.m[i][j] = i == j ? 1.0 : 0.0;
        return "";
    }
    static const char* const xyz[3] = {"rXYZ", "gXYZ", "bXYZ"};
    static const char* const trc[3] = {"rTRC", "gTRC", "bTRC"};
    for (int k = 0; k < 3; ++k) {
        Tag t;
        std::string r = find(xyz[k], t);
        if (!r.empty()) return r;
        if (!t.found) return std::string("the profile has no '") + xyz[k] + "' tag";
        if (t.size < 20 || be32(p + t.off) != sig("XYZ ")) return std::string("not a profile: tag '") + xyz[k] + "' is not an XYZ value";
        for (int i = 0; i < 3; ++i) T.colorant[i][k] = s15f16(p + t.off + 8 + 4 * i);
        r = curve(trc[k], T.curve[k]);
        if (!r.empty()) return r;
    }
    double inv[3][3];
    gk_inv3(GK_SRGB_COLORANTS, inv);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += inv[i][k] * T.colorant[k][j];
            T.m[i][j] = s;
        }
    return "";
}
