"""The region of each band under a shaped region of interest (ISO 15444-1 Annex H.3), in numpy.

Test infrastructure only: the definition the mask kernels (grok_amd/csrc/gk_roi.hip) are held to,
itself checked against the inverse transforms in tests/test_roi_region.py.

One dimension: samples and coefficients of a tile-component at one decomposition level share the
interleaved index k over [lo, hi) in that level's canvas coordinates; even k is low-pass, odd k
high-pass.  A region sample at k needs the coefficients at k + d for |d| <= REACH[transform][k & 1]
(the synthesis cones of the two lifting schemes); an index outside [lo, hi) is reflected
whole-sample symmetrically, again and again for intervals shorter than the cone, and an interval
of one sample needs only itself.  Two dimensions are the product: rows, then columns.  The low/low
positions of the result are the next level's sample mask, the other parities that level's HL, LH
and HH band masks; the last level's low/low is the LL band's mask.
"""
import numpy as np

REACH = {"53": (1, 2), "97": (3, 4)}   # by transform: (k even, k odd)


def reflect(i, lo, hi):
    """Index i reflected whole-sample symmetrically into [lo, hi)."""
    if hi - lo == 1:
        return lo
    while i < lo or i >= hi:
        i = 2 * lo - i if i < lo else 2 * (hi - 1) - i
    return i


def needed_1d(k, lo, hi, transform):
    """The coefficient indices the sample at k of [lo, hi) needs."""
    if hi - lo == 1:
        return {k}
    r = REACH[transform][k & 1]
    return {reflect(k + d, lo, hi) for d in range(-r, r + 1)}


def dilate_1d(mask, lo, transform):
    """mask: booleans over [lo, lo + len(mask)).  The coefficient mask of that interval."""
    out = np.zeros(len(mask), bool)
    for i in np.flatnonzero(mask):
        for j in needed_1d(lo + int(i), lo, lo + len(mask), transform):
            out[j - lo] = True
    return out


def dilate_2d(mask, x0, y0, transform):
    """mask (h, w) at canvas origin (x0, y0): along rows, then along columns."""
    m = np.asarray(mask, bool)
    rows = np.array([dilate_1d(r, x0, transform) for r in m]).reshape(m.shape)
    cols = np.array([dilate_1d(c, y0, transform) for c in rows.T]).reshape(m.T.shape).T
    return cols


def split(cm, x0, y0):
    """The four parities of an interleaved coefficient mask at origin (x0, y0): LL, HL, LH, HH."""
    ex, ey = x0 & 1, y0 & 1      # offset of the first even column / row
    ox, oy = 1 - ex, 1 - ey      # of the first odd ones
    return cm[ey::2, ex::2], cm[ey::2, ox::2], cm[oy::2, ex::2], cm[oy::2, ox::2]


def band_masks(mask, x0, y0, levels, transform):
    """mask: (h, w) booleans of a tile-component whose canvas origin is (x0, y0).  Returns
    {(resolution, band): mask} as the engine numbers them: (0, 0) is the LL band; resolution
    r >= 1 has bands 0 HL, 1 LH, 2 HH (decomposition level levels + 1 - r)."""
    out = {}
    m = np.asarray(mask, bool)
    for lev in range(1, levels + 1):
        cm = dilate_2d(m, x0, y0, transform) if m.size else m
        ll, hl, lh, hh = split(cm, x0, y0)
        r = levels + 1 - lev
        out[(r, 0)], out[(r, 1)], out[(r, 2)] = hl, lh, hh
        m = ll
        x0, y0 = (x0 + 1) >> 1, (y0 + 1) >> 1
    out[(0, 0)] = m
    return out


def image_band_masks(mask, origin, tiles, tile_origin, levels, transform):
    """Every tile's band masks for an image mask (H, W) whose canvas origin is origin = (x0, y0),
    tiled by tiles = (tw, th) (None: one tile) from tile_origin: {(tile, resolution, band): mask}."""
    h, w = mask.shape
    x0, y0 = origin
    gx, gy = tile_origin
    tw, th = tiles if tiles else (x0 + w - gx, y0 + h - gy)
    ntx, nty = -(-(x0 + w - gx) // tw), -(-(y0 + h - gy) // th)
    out = {}
    for j in range(nty):
        for i in range(ntx):
            tx0, ty0 = max(gx + i * tw, x0), max(gy + j * th, y0)
            tx1, ty1 = min(gx + (i + 1) * tw, x0 + w), min(gy + (j + 1) * th, y0 + h)
            sub = mask[ty0 - y0:ty1 - y0, tx0 - x0:tx1 - x0]
            for (r, b), m in band_masks(sub, tx0, ty0, levels, transform).items():
                out[(j * ntx + i, r, b)] = m
    return out
