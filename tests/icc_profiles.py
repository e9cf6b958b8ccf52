"""ICC profiles written as bytes, and CIELab colr boxes: what a JP2 colr box may carry (Part 1:
Monochrome Input and Three-Component Matrix-Based Input profiles), plus the malformed and
unsupported ones the engine refuses under GK_DISPLAY_ICC.  Test infrastructure only."""
import functools
import struct

import numpy as np

D50 = (0.9642, 1.0, 0.8249)
# D50-adapted colorants (rows r, g, b; X, Y, Z each)
COLORANTS = {
    "adobe": ((0.60974, 0.31111, 0.01947), (0.20528, 0.62567, 0.06087), (0.14919, 0.06322, 0.74457)),
    "p3": ((0.51512, 0.24120, -0.00105), (0.29198, 0.69225, 0.04189), (0.15710, 0.06657, 0.78407)),
    "prophoto": ((0.79767, 0.28804, 0.0), (0.13519, 0.71188, 0.0), (0.03134, 0.00009, 0.82521)),
}


def s15(v):
    return struct.pack(">i", int(round(v * 65536)))


def xyz_tag(x, y, z):
    return b"XYZ " + b"\0" * 4 + s15(x) + s15(y) + s15(z)


def curv_identity():
    return b"curv" + b"\0" * 4 + struct.pack(">I", 0)


def curv_gamma(u8f8):
    """count 1: a u8Fixed8 gamma (563 is 2.19921875)."""
    return b"curv" + b"\0" * 4 + struct.pack(">IH", 1, u8f8)


def curv_table(values, count=None):
    values = [int(v) for v in values]
    return b"curv" + b"\0" * 4 + struct.pack(">I", len(values) if count is None else count) + \
        b"".join(struct.pack(">H", v) for v in values)


def para(ftype, params):
    return b"para" + b"\0" * 4 + struct.pack(">HH", ftype, 0) + b"".join(s15(v) for v in params)


def srgb_decode(x):
    x = np.asarray(x, np.float64)
    return np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)


def table_curve(n, power=None):
    """n uint16 entries over [0, 1]: the sRGB decoding, or x ** power."""
    x = np.arange(n) / (n - 1.0)
    y = srgb_decode(x) if power is None else x ** power
    return np.floor(y * 65535 + 0.5).astype(np.int64)


_S = 0.95 ** (1 / 2.4)
CURVES = {
    "g22": curv_gamma(563),
    "g18": curv_gamma(461),
    "table1024": curv_table(table_curve(1024)),
    "para0": para(0, [2.2]),
    # (every curve maps 0 to 0: with a black above zero lcms2 compensates the black point for these
    #  v4 profiles under the perceptual intent, which the engine does not do)
    "para1": para(1, [2.0, 1.1, -0.1]),
    "para2": para(2, [2.0, 0.9, 0.1, -0.01]),
    "para3": para(3, [2.4, 1 / 1.055, 0.055 / 1.055, 1 / 12.92, 0.04045]),
    "para4": para(4, [2.4, _S / 1.055, _S * 0.055 / 1.055, 0.95 / 12.92, 0.04045, 0.02, 0.0]),
}


def profile(tags, space=b"RGB ", pcs=b"XYZ ", intent=0, size=None, ntags=None, signature=b"acsp", move=None):
    """tags: [(signature, data)].  size / ntags / signature override the header fields; move = (tag
    signature, offset) rewrites one tag's offset in the table."""
    n = len(tags)
    off = 128 + 4 + 12 * n
    table, body = b"", b""
    for sg, data in tags:
        data = data + b"\0" * (-len(data) % 4)
        o = off + len(body)
        if move and move[0] == sg:
            o = move[1]
        table += sg + struct.pack(">II", o, len(data))
        body += data
    total = off + len(body)
    hdr = struct.pack(">I", total if size is None else size) + b"\0" * 4 + struct.pack(">I", 0x04300000) + b"mntr" + space + pcs
    hdr += b"\0" * 12 + signature + b"\0" * 24 + struct.pack(">I", intent) + s15(D50[0]) + s15(D50[1]) + s15(D50[2])
    hdr += b"\0" * (128 - len(hdr))
    return hdr + struct.pack(">I", n if ntags is None else ntags) + table + body


def rgb_profile(colorants, curves, intent=0, drop=(), extra=(), **kw):
    """colorants: a COLORANTS name; curves: one CURVES name / tag data, or three."""
    c = COLORANTS[colorants]
    if isinstance(curves, (str, bytes)):
        curves = [curves] * 3
    curves = [CURVES[v] if isinstance(v, str) else v for v in curves]
    tags = [(b"wtpt", xyz_tag(*D50))]
    for k, ch in enumerate("rgb"):
        tags.append((ch.encode() + b"XYZ", xyz_tag(*c[k])))
        tags.append((ch.encode() + b"TRC", curves[k]))
    tags = [t for t in tags if t[0] not in drop] + list(extra)
    return profile(tags, intent=intent, **kw)


def grey_profile(curve, **kw):
    curve = CURVES[curve] if isinstance(curve, str) else curve
    return profile([(b"wtpt", xyz_tag(*D50)), (b"kTRC", curve)], space=b"GRAY", **kw)


@functools.lru_cache(maxsize=None)
def accepted():
    """name -> (profile bytes, is grey)"""
    out = {}
    for c in COLORANTS:
        for v in CURVES:
            out["%s_%s" % (c, v)] = (rgb_profile(c, v), False)
    out["adobe_three_curves"] = (rgb_profile("adobe", ["g22", "table1024", "para3"]), False)
    out["p3_identity_intent3"] = (rgb_profile("p3", curv_identity(), intent=3), False)
    out["grey_g22"] = (grey_profile("g22"), True)
    out["grey_table"] = (grey_profile(curv_table(table_curve(256, 1.8))), True)
    return out


RANDOM_200 = bytes(np.random.RandomState(7).randint(0, 256, 200).astype(np.uint8))   # (tests/jp2_boxes.py c7_icc)


@functools.lru_cache(maxsize=None)
def refused():
    """name -> (profile bytes, words the refusal must contain)"""
    good = rgb_profile("adobe", "g22")
    out = {}
    out["random_bytes"] = (RANDOM_200, "acsp")
    out["no_acsp"] = (rgb_profile("adobe", "g22", signature=b"xxxx"), "acsp")
    out["size_past_box"] = (rgb_profile("adobe", "g22", size=len(good) + 100), "size field")
    out["tag_table_outside"] = (rgb_profile("adobe", "g22", ntags=100000), "tag table")
    out["tag_outside"] = (rgb_profile("adobe", "g22", move=(b"gXYZ", len(good) - 8)), "outside the profile")
    out["curve_overrun"] = (rgb_profile("adobe", ["g22", curv_table([0, 65535], count=5000), "g22"]), "overruns")
    out["a2b0"] = (rgb_profile("adobe", "g22", extra=[(b"A2B0", b"mft2" + b"\0" * 48)]), "A2B0")
    out["a2b1"] = (rgb_profile("adobe", "g22", extra=[(b"A2B1", b"mft2" + b"\0" * 48)]), "A2B1")
    out["ycbcr"] = (rgb_profile("adobe", "g22", space=b"YCbr"), "YCbr")
    out["cmyk"] = (rgb_profile("adobe", "g22", space=b"CMYK"), "CMYK")
    out["pcs_lab"] = (rgb_profile("adobe", "g22", pcs=b"Lab "), "Lab")
    out["missing_colorant"] = (rgb_profile("adobe", "g22", drop=(b"gXYZ",)), "gXYZ")
    out["missing_curve"] = (rgb_profile("adobe", "g22", drop=(b"bTRC",)), "bTRC")
    out["grey_missing_curve"] = (profile([(b"wtpt", xyz_tag(*D50))], space=b"GRAY"), "kTRC")
    out["unknown_curve"] = (rgb_profile("adobe", ["g22", b"mft2" + b"\0" * 48, "g22"]), "mft2")
    out["para_type_5"] = (rgb_profile("adobe", para(5, [1.0] * 7)), "parametric")
    return out


# ---------------------------------------------------------------------------- CIELab colr boxes
GRK_DEFAULT_CIELAB_SPACE, GRK_CUSTOM_CIELAB_SPACE = 0x44454600, 0
CIE_D50, CIE_D65 = 0x00443530, 0x00443635


def colr_lab(custom=None):
    """The colr box of EnumCS 14: 7 bytes, or 35 with custom = (rl, ol, ra, oa, rb, ob, il)."""
    payload = struct.pack(">BBBI", 1, 0, 0, 14)
    if custom is not None:
        payload += struct.pack(">7I", *custom)
    return struct.pack(">I4s", 8 + len(payload), b"colr") + payload


def lab_words(custom=None):
    """What Grok keeps in icc_profile_buf for that box."""
    if custom is None:
        return [14, GRK_DEFAULT_CIELAB_SPACE]
    return [14, GRK_CUSTOM_CIELAB_SPACE] + [int(v) for v in custom]


# ---------------------------------------------------------------------------- JP2 files
def jp2(cs, h, w, nc, prec, colr, cdef=None, extra=(), signed=False):
    """A JP2 file around codestream cs: ihdr, the colr box given as bytes (colr_profile / colr_lab /
    an enumerated one), an optional cdef [(Cn, Typ, Asoc)] and further jp2h boxes."""
    import jp2_boxes as J
    sub = [J.ihdr(h, w, nc, prec, signed), colr]
    if cdef is not None:
        sub.append(J.cdef(cdef))
    return J.jp2_file(cs, sub + list(extra))


def colr_profile(profile):
    return struct.pack(">I4sBBB", 8 + 3 + len(profile), b"colr", 2, 0, 0) + bytes(profile)


RGBA_CDEF = [(0, 0, 1), (1, 0, 2), (2, 0, 3), (3, 1, 0)]
GREYA_CDEF = [(0, 0, 1), (1, 1, 0)]
