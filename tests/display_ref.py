"""NumPy restatement of what Grok's CLI does to a decoded image (GrkDecompress::postProcess,
bin/jp2/grk_decompress.cpp:1300-1506): color_sycc_to_rgb / color_esycc_to_rgb / color_cmyk_to_rgb
(bin/common/color.cpp:86-418, 970-1086) and upsample_image_components (bin/common/convert.cpp:209-360).
The checker of tests/test_display.py (known answers, CPU) and tests/test_gpu_display.py (the HIP
display stage against this file applied to the engine's own flag-0 decode).

Arithmetic: float64 (sYCC, e-sYCC) and float32 (CMYK) element by element, every product and sum
rounded on its own as NumPy does, astype(int32) truncating toward zero like the C cast.  Which
chroma sample a pixel takes is decided by the reference's loops, transcribed with the same
pointers; the arithmetic is then applied to the selected samples at once.

sycc420_to_rgb as written keys its first-ROW branch on oddFirstX (:300) and its first-COLUMN branch
on oddFirstY (:316).  With equal parities that is consistent and the transcription below is the C,
pointer for pointer (it asserts that every pixel is written exactly once).  With different parities
the C loops leave the planes (one row too many, or rows one sample short whose pointers drift), so
there is nothing to transcribe; `sycc420_select` then follows the rule the loops are meant to
implement: row 0 alone when the origin's row is odd, column 0 alone when its column is odd, pairs
from there, and (as :316-320) column 0 of the first row of each pair alone when the row is odd."""
import numpy as np

CS_UNKNOWN, CS_SRGB, CS_GRAY, CS_SYCC, CS_EYCC, CS_CMYK = 0, 2, 3, 4, 5, 6   # GRK_COLOR_SPACE


def sycc_to_rgb(offset, upb, y, cb, cr):
    """sycc_to_rgb (:86-113) on arrays (or scalars) of samples."""
    y = np.asarray(y, np.int64)
    cb = np.asarray(cb, np.int64) - offset
    cr = np.asarray(cr, np.int64) - offset
    r = y + (np.float64(1.402) * cr.astype(np.float64)).astype(np.int32)
    g = y - (np.float64(0.344) * cb.astype(np.float64) + np.float64(0.714) * cr.astype(np.float64)).astype(np.int32)
    b = y + (np.float64(1.772) * cb.astype(np.float64)).astype(np.int32)
    return [np.clip(v, 0, upb).astype(np.int32) for v in (r, g, b)]


def sycc422_select(w, h, cb, cr, ofx):
    """sycc422_to_rgb's loops (:210-234): the (Cb, Cr) every pixel is converted with."""
    sb, sr = np.full((h, w), -1, np.int64), np.full((h, w), -1, np.int64)
    loopmaxw = w - (1 if ofx else 0)
    for i in range(h):
        x = 0
        c = 0
        if ofx:
            sb[i, x], sr[i, x] = 0, 0
            x += 1
        j = 0
        while j < (loopmaxw & ~1):
            sb[i, x], sr[i, x] = cb[i, c], cr[i, c]
            x += 1
            sb[i, x], sr[i, x] = cb[i, c], cr[i, c]
            x += 1
            c += 1
            j += 2
        if j < loopmaxw:
            sb[i, x], sr[i, x] = cb[i, c], cr[i, c]
            x += 1
            c += 1
        assert x == w and c == cb.shape[1]
    return sb, sr


def _sycc420_unequal(w, h, cb, cr, ofx, ofy):
    sb, sr = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    paired = (h - ofy) & ~1
    for y in range(ofy, h):
        ry = y - ofy
        for x in range(ofx, w):
            sb[y, x], sr[y, x] = cb[ry // 2, (x - ofx) // 2], cr[ry // 2, (x - ofx) // 2]
        if ofy and ry < paired and not ry & 1:
            sb[y, 0], sr[y, 0] = 0, 0
    return sb, sr


def sycc420_select(w, h, cb, cr, ofx, ofy):
    """sycc420_to_rgb's loops (:290-357) with flat pointers: d / n walk the luma and destination
    rows (one stride: w), c the chroma planes."""
    ofx, ofy = int(bool(ofx)), int(bool(ofy))
    if ofx != ofy:
        return _sycc420_unequal(w, h, cb, cr, ofx, ofy)
    cbf, crf = np.asarray(cb).ravel(), np.asarray(cr).ravel()
    sb, sr = np.full(w * h, -1, np.int64), np.full(w * h, -1, np.int64)

    def put(p, vb, vr):
        assert sb[p] == -1
        sb[p], sr[p] = vb, vr

    loopmaxw, loopmaxh = w - ofx, h - ofy
    d = c = 0
    if ofx:                                   # (:300, as written)
        for _ in range(w):
            put(d, 0, 0)
            d += 1
    i = 0
    while i < (loopmaxh & ~1):
        n = d + w
        if ofy:                               # (:316, as written)
            put(d, 0, 0)
            d += 1
            put(n, cbf[c], crf[c])
            n += 1
        j = 0
        while j < (loopmaxw & ~1):
            put(d, cbf[c], crf[c])
            d += 1
            put(d, cbf[c], crf[c])
            d += 1
            put(n, cbf[c], crf[c])
            n += 1
            put(n, cbf[c], crf[c])
            n += 1
            c += 1
            j += 2
        if j < loopmaxw:
            put(d, cbf[c], crf[c])
            d += 1
            put(n, cbf[c], crf[c])
            n += 1
            c += 1
        d += w
        i += 2
    if i < loopmaxh:                          # last row has no sub-sampling
        j = 0
        while j < (w & ~1):
            put(d, cbf[c], crf[c])
            d += 1
            put(d, cbf[c], crf[c])
            d += 1
            c += 1
            j += 2
        if j < w:
            put(d, cbf[c], crf[c])
    assert (sb >= 0).all()
    return sb.reshape(h, w), sr.reshape(h, w)


def color_sycc_to_rgb(planes, comps, ofx, ofy):
    """color_sycc_to_rgb (:379-418): (planes, comps) converted, or None for another pattern."""
    (dx0, dy0, prec, _), (dx1, dy1, _, _), (dx2, dy2, _, _) = comps[:3]
    offset, upb = 1 << (prec - 1), (1 << prec) - 1
    y, cb, cr = planes
    h, w = y.shape
    pat = (dx0, dx1, dx2, dy0, dy1, dy2)
    if pat == (1, 2, 2, 1, 2, 2):
        sb, sr = sycc420_select(w, h, cb, cr, ofx, ofy)
    elif pat == (1, 2, 2, 1, 1, 1):
        sb, sr = sycc422_select(w, h, cb, cr, ofx)
    elif pat == (1, 1, 1, 1, 1, 1):
        sb, sr = cb, cr
    else:
        return None
    out = sycc_to_rgb(offset, upb, y, sb, sr)
    return out, [(dx0, dy0, p, s) for (_, _, p, s) in comps]


def sanity(comps):
    """all_components_sanity_check(image, true) (common.cpp:333-375)."""
    if comps[0][2] == 0 or comps[0][2] > 16:
        return False
    return all(c[2] == comps[0][2] and c[3] == comps[0][3] for c in comps[1:])


def color_esycc_to_rgb(planes, comps):
    """color_esycc_to_rgb (:1027-1086)."""
    prec = comps[0][2]
    flip, mx = 1 << (prec - 1), (1 << prec) - 1
    y = planes[0].astype(np.float64)
    cb = (planes[1].astype(np.int64) - (0 if comps[1][3] else flip)).astype(np.float64)
    cr = (planes[2].astype(np.int64) - (0 if comps[2][3] else flip)).astype(np.float64)
    f = np.float64
    r = (y - f(0.0000368) * cb + f(1.40199) * cr + f(0.5)).astype(np.int32)
    g = (f(1.0003) * y - f(0.344125) * cb - f(0.7141128) * cr + f(0.5)).astype(np.int32)
    b = (f(0.999823) * y + f(1.77204) * cb - f(0.000008) * cr + f(0.5)).astype(np.int32)
    return [np.clip(v, 0, mx).astype(np.int32) for v in (r, g, b)]


def color_cmyk_to_rgb(planes, comps):
    """color_cmyk_to_rgb (:970-1024): single precision, one rounding per operation."""
    f = np.float32
    s = [f(1.0) / f((1 << c[2]) - 1) for c in comps[:4]]
    v = [f(1.0) - planes[k].astype(np.float32) * s[k] for k in range(4)]
    return [(f(255.0) * v[k] * v[3]).astype(np.int32) for k in range(3)]


def upsample_component(src, dx, dy, x0, y0, x1, y1):
    """upsample_image_components' loops for one component with dx > 1 or dy > 1 (:268-351)."""
    cd = lambda a, b: -(-a // b)
    sh, sw = src.shape
    w = x1 - x0 if dx > 1 else sw
    h = y1 - y0 if dy > 1 else sh
    dst = np.full((h, w), -(1 << 30), np.int64)
    xoff, yoff = dx * cd(x0, dx) - x0, dy * cd(y0, dy) - y0
    assert xoff < dx and yoff < dy

    def row(drow, srow):
        x = xorg = 0
        while x < xoff:
            drow[x] = 0
            x += 1
        if w > dx - 1:
            while x < w - (dx - 1):
                for k in range(dx):
                    drow[x + k] = srow[xorg]
                x += dx
                xorg += 1
        while x < w:
            drow[x] = srow[xorg]
            x += 1

    y = sy = 0
    while y < yoff:
        dst[y, :] = 0
        y += 1
    if h > dy - 1:
        while y < h - (dy - 1):
            row(dst[y], src[sy])
            for k in range(1, dy):
                dst[y + k] = dst[y]
            y += dy
            sy += 1
    if y < h:
        row(dst[y], src[sy])
        y0_ = y
        y += 1
        while y < h:
            dst[y] = dst[y0_]
            y += 1
    assert (dst > -(1 << 30)).all()
    return dst.astype(np.int32)


def post_process(planes, comps, colour_space, bounds, rgb=False, upsample=False, odd_first=None):
    """postProcess on a decoded image.  planes: the components (2-D int arrays); comps: [(dx, dy,
    prec, sgnd)]; colour_space: GRK_COLOR_SPACE of the file (0 for a raw codestream); bounds: the
    image's (or the window's) canvas rectangle (x0, y0, x1, y1); odd_first: (oddFirstX, oddFirstY),
    by default the parities of bounds' origin.
    Returns (planes, comps, colour_space, converted, upsampled)."""
    planes = [np.asarray(p) for p in planes]
    comps = [tuple(c) for c in comps]
    x0, y0, x1, y1 = bounds
    ofx, ofy = odd_first if odd_first is not None else (x0 & 1, y0 & 1)
    converted = upsampled = False
    cs = colour_space
    if rgb:
        n = len(planes)
        if cs != CS_SYCC and n == 3 and comps[0][0] == comps[0][1] and comps[1][0] != 1:
            cs = CS_SYCC
        elif n <= 2:
            cs = CS_GRAY
        if cs == CS_SYCC:
            if n != 3:
                raise ValueError("YCC: number of components %d not equal to 3" % n)
            got = color_sycc_to_rgb(planes, comps, ofx, ofy)
            if got is not None:
                (planes, comps), cs, converted = got, CS_SRGB, True
        elif cs == CS_EYCC:
            if n != 3:
                raise ValueError("YCC: number of components %d not equal to 3" % n)
            if sanity(comps):
                planes, cs, converted = color_esycc_to_rgb(planes, comps), CS_SRGB, True
        elif cs == CS_CMYK:
            if n != 4:
                raise ValueError("CMYK: number of components %d not equal to 4" % n)
            if sanity(comps):
                planes = color_cmyk_to_rgb(planes, comps)
                comps = [(c[0], c[1], 8, c[3]) for c in comps[:3]]
                cs, converted = CS_SRGB, True
    if upsample and any(c[0] > 1 or c[1] > 1 for c in comps):
        out = []
        for p, (dx, dy, _, _) in zip(planes, comps):
            out.append(upsample_component(p, dx, dy, x0, y0, x1, y1) if dx > 1 or dy > 1 else p.astype(np.int32))
        planes, comps, upsampled = out, [(1, 1, c[2], c[3]) for c in comps], True
    return planes, comps, cs, converted, upsampled
