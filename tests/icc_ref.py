"""float64 restatement of the colour management Grok's CLI does through lcms2 for a JP2 file's ICC
profile (color_apply_icc_profile) and for CIELab (color_cielab_to_rgb), on v / (2^p - 1):

    tone curve -> profile colorants (s15Fixed16) -> inverse of lcms2's sRGB colorants -> clip to
    [0, 1] -> sRGB encoding -> * (2^p - 1), rounded half up.

Every function returns the UNROUNDED level and the rounded one, so that a comparison can tell a
sample that sits on a rounding tie.  tests/test_icc.py pins it against lcms2.  Test infrastructure
only; it reads profiles on its own (no engine code)."""
import struct

import numpy as np

SRGB_COLORANTS = np.array([[0.43604125, 0.38511291, 0.14304584],
                           [0.22248454, 0.71690508, 0.06061038],
                           [0.01392019, 0.09706724, 0.71391257]])
D50 = np.array([0.9642, 1.0, 0.8249])


def srgb_encode(v):
    v = np.clip(v, 0.0, 1.0)
    return np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(v, 1 / 2.4) - 0.055)


def _tags(b):
    n = struct.unpack_from(">I", b, 128)[0]
    out = {}
    for i in range(n):
        sg, off, size = struct.unpack_from(">4sII", b, 132 + 12 * i)
        out.setdefault(sg, b[off:off + size])
    return out


def _s15(b, off):
    return struct.unpack_from(">i", b, off)[0] / 65536.0


def _curve(t):
    """tag data -> a function on float64 arrays over [0, 1]; a table curve (on_samples) takes the
    integer samples and their largest value instead"""
    if t[:4] == b"curv":
        n = struct.unpack_from(">I", t, 8)[0]
        if n == 0:
            return lambda x: x
        if n == 1:
            g = struct.unpack_from(">H", t, 12)[0] / 256.0
            return lambda x: np.power(x, g)
        tab = np.array(struct.unpack_from(">%dH" % n, t, 12), np.uint32)

        def interp(v, vmax):
            # lcms2 reads a 16-bit table in fixed point (cmsEvalToneCurveFloat -> LinLerp1D,
            # cmsintrp.c): the input as a 16-bit word rounded half up, _cmsToFixedDomain, LinearInterp
            # in unsigned 32-bit arithmetic, a 16-bit result
            inp = ((2 * v.astype(np.uint64) * 65535 + vmax) // (2 * vmax)).astype(np.uint32)
            v3 = (np.uint32(n - 1) * inp).astype(np.uint32)
            v3 = (v3 + (v3 + np.uint32(0x7fff)) // np.uint32(0xffff)).astype(np.uint32)
            cell, rest = np.minimum(v3 >> 16, n - 2), v3 & np.uint32(0xffff)
            y0, y1 = tab[cell], tab[cell + 1]
            out = ((((y1 - y0) * rest + np.uint32(0x8000)) >> 16) + y0) & np.uint32(0xffff)
            out = np.where(inp == 0xffff, tab[n - 1], out)
            return out.astype(np.float64) / 65535.0
        interp.on_samples = True
        return interp
    assert t[:4] == b"para"
    ft = struct.unpack_from(">H", t, 8)[0]
    v = [_s15(t, 12 + 4 * i) for i in range((1, 3, 4, 5, 7)[ft])] + [0.0] * 7
    g, a, b, c, d, e, f = v[0], 1.0, 0.0, 0.0, 0.0, 0.0, 0.0
    if ft in (1, 2):
        a, b = v[1], v[2]
        d = -b / a
        if ft == 2:
            e = f = v[3]
    elif ft >= 3:
        a, b, c, d = v[1:5]
        if ft == 4:
            e, f = v[5], v[6]

    def fn(x):
        with np.errstate(invalid="ignore"):
            return np.where(x >= d, np.power(np.maximum(a * x + b, 0.0), g) + e, c * x + f)
    return fn


def read_profile(b):
    """-> (is grey, [curve functions], matrix into linear sRGB or None)"""
    t = _tags(b)
    if b[16:20] == b"GRAY":
        return True, [_curve(t[b"kTRC"])], None
    col = np.array([[_s15(t[ch + b"XYZ"], 8 + 4 * i) for ch in (b"r", b"g", b"b")] for i in range(3)])
    return False, [_curve(t[ch + b"TRC"]) for ch in (b"r", b"g", b"b")], np.linalg.inv(SRGB_COLORANTS) @ col


def _levels(enc, bits):
    x = enc * float((1 << bits) - 1)
    return x, np.floor(x + 0.5).astype(np.int64)


def apply_profile(profile, samples, bits):
    """samples: integer array, (..., 3) for an RGB profile or (...) for a grey one, at `bits` bits ->
    (unrounded float64, rounded int64) sRGB levels at the same precision; a grey profile gives one
    value per sample (its R = G = B)."""
    grey, curves, m = read_profile(profile)
    vmax = (1 << bits) - 1
    v = np.asarray(samples, np.int64)
    x = v.astype(np.float64) / float(vmax)

    def run(fn, k):
        if getattr(fn, "on_samples", False):
            return fn(v[k], vmax)
        return fn(x[k])
    if grey:
        return _levels(srgb_encode(run(curves[0], Ellipsis)), bits)
    lin = np.stack([run(curves[k], (Ellipsis, k)) for k in range(3)], axis=-1)
    return _levels(srgb_encode(lin @ m.T), bits)


def lab_ranges(bits, words):
    """(lo, range) per channel from Grok's words: value = lo + v * range / (2^bits - 1)
    (color_cielab_to_rgb :833-851, :920-927)."""
    p = float(bits)
    r = [100.0, 170.0, 200.0]
    o = [0.0, 2.0 ** (p - 1), 3 * 2.0 ** (p - 3)]
    if len(words) >= 9 and words[1] == 0:
        r = [float(words[2]), float(words[4]), float(words[6])]
        o = [float(words[3]), float(words[5]), float(words[7])]
    vmax = 2.0 ** p - 1
    lo = [-(r[k] * o[k]) / vmax for k in range(3)]
    return lo, [(lo[k] + r[k]) - lo[k] for k in range(3)]


def lab_values(samples, bits, words):
    """integer L*a*b* samples (..., 3) -> CIELab values, as Grok hands them to lcms2"""
    lo, rng = lab_ranges(bits, words)
    v = np.asarray(samples, np.float64)
    return np.stack([lo[k] + v[..., k] * rng[k] / (2.0 ** bits - 1) for k in range(3)], axis=-1)


def lab_to_rgb(lab):
    """CIELab (..., 3) under D50 -> (unrounded, rounded) sRGB at 16 bits"""
    lab = np.asarray(lab, np.float64)
    fy = (lab[..., 0] + 16.0) / 116.0
    f = np.stack([fy + 0.002 * lab[..., 1], fy, fy - 0.005 * lab[..., 2]], axis=-1)
    xyz = np.where(f <= 24.0 / 116.0, (108.0 / 841.0) * (f - 16.0 / 116.0), f ** 3) * D50
    return _levels(srgb_encode(xyz @ np.linalg.inv(SRGB_COLORANTS).T), 16)


def tie_band(bits):
    """tau(p) = 2^(p - 19) LSB"""
    return 2.0 ** (bits - 19)


def check(got, unrounded, rounded, bits):
    """The comparison rule: equal to the rounded reference, or one off where the unrounded value
    lies within tau of a rounding tie.  Returns the number of samples that break it."""
    got = np.asarray(got, np.int64)
    diff = np.abs(got - rounded)
    frac = unrounded - np.floor(unrounded)
    near_tie = np.abs(frac - 0.5) <= tie_band(bits)
    return int(np.count_nonzero((diff > 1) | ((diff == 1) & ~near_tie)))
