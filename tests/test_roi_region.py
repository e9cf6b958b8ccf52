"""Shaped region of interest, the parts that need no GPU: the rule of tests/roi_ref.py against the
inverse transforms themselves, gk_probe_encode_roi's refusals and shifts, and the argument checks
of the Python interface."""
import numpy as np
import pytest

import grok_amd as G
import j2k_markers as M
import roi_ref as RR

# ------------------------------------------------------------------ plain inverse lifting (Annex F)
A97, B97, C97, D97, K97 = -1.586134342059924, -0.052980118572961, 0.882911075530934, 0.443506852043971, 1.230174104914001


def _ext(c, lo, i):
    """c[i] under whole-sample symmetric extension (the test's own: roi_ref's is what is checked)."""
    n = len(c)
    m = (i - lo) % (2 * n - 2)
    return c[m if m < n else 2 * n - 2 - m]


def inv53(c, lo):
    """c: interleaved coefficients over [lo, lo + n) (even index low-pass).  F.3.8.2, integers."""
    n = len(c)
    if n == 1:
        return [c[0] if lo % 2 == 0 else c[0] // 2]
    x = {}
    for k in range(lo - 3, lo + n + 3):
        x[k] = _ext(c, lo, k)
    for k in range(lo - 2, lo + n + 2):
        if k % 2 == 0:
            x[k] = x[k] - ((x[k - 1] + x[k + 1] + 2) >> 2)
    for k in range(lo - 1, lo + n + 1):
        if k % 2:
            x[k] = x[k] + ((x[k - 1] + x[k + 1]) >> 1)
    return [x[k] for k in range(lo, lo + n)]


def inv97(c, lo):
    """F.3.8.1 in floats: scale, then the four lifting steps undone."""
    n = len(c)
    if n == 1:
        return [c[0] if lo % 2 == 0 else c[0] / 2]
    x = {}
    for k in range(lo - 8, lo + n + 8):
        v = _ext(c, lo, k)
        x[k] = v * K97 if k % 2 == 0 else v / K97
    for step, (par, coef) in enumerate(((0, D97), (1, C97), (0, B97), (1, A97))):
        m = 7 - step
        for k in range(lo - m, lo + n + m):
            if k % 2 == par:
                x[k] = x[k] - coef * (x[k - 1] + x[k + 1])
    return [x[k] for k in range(lo, lo + n)]


INV = {"53": inv53, "97": inv97}


def _influence_1d(transform, lo, n, rng):
    """dep[j] = the samples that change when coefficient j changes (over several bases and steps)."""
    inv = INV[transform]
    dep = [set() for _ in range(n)]
    for trial in range(3):
        base = [int(v) for v in rng.integers(-40, 40, n)]
        if transform == "97":
            base = [v + 0.37 for v in base]
        ref = inv(base, lo)
        for j in range(n):
            for delta in (1, 2, 3, 4, 8, 17, -5):
                c = list(base)
                c[j] += delta
                out = inv(c, lo)
                dep[j].update(k for k in range(n) if out[k] != ref[k])
    return dep


@pytest.mark.parametrize("transform", ["53", "97"])
@pytest.mark.parametrize("lo", [0, 1, 6, 7])
def test_rule_is_the_inverse_transforms_dependency_1d(transform, lo):
    """For every single region sample the coefficients that change it are exactly the rule's set."""
    rng = np.random.default_rng(5)
    for n in range(1, 25):
        dep = _influence_1d(transform, lo, n, rng)
        for k in range(n):
            changed = {lo + j for j in range(n) if k in dep[j]}
            assert changed == RR.needed_1d(lo + k, lo, lo + n, transform), (transform, lo, n, k)
            m = np.zeros(n, bool)
            m[k] = True
            assert set(lo + np.flatnonzero(RR.dilate_1d(m, lo, transform))) == changed


def _inv2d_levels(bands, x0, y0, w, h, levels, transform):
    """Inverse 2-D transform of a tile-component at origin (x0, y0) from roi_ref-numbered bands."""
    inv = INV[transform]
    geo = [(x0, y0, w, h)]
    for _ in range(levels):
        gx, gy, gw, gh = geo[-1]
        geo.append(((gx + 1) >> 1, (gy + 1) >> 1, ((gx + gw + 1) >> 1) - ((gx + 1) >> 1), ((gy + gh + 1) >> 1) - ((gy + 1) >> 1)))
    ll = bands[(0, 0)]
    for lev in range(levels, 0, -1):
        gx, gy, gw, gh = geo[lev - 1]
        r = levels + 1 - lev
        a = np.zeros((gh, gw), dtype=ll.dtype)
        ex, ey = gx & 1, gy & 1
        a[ey::2, ex::2] = ll
        a[ey::2, 1 - ex::2] = bands[(r, 0)]
        a[1 - ey::2, ex::2] = bands[(r, 1)]
        a[1 - ey::2, 1 - ex::2] = bands[(r, 2)]
        a = np.array([inv(list(col), gy) for col in a.T], dtype=ll.dtype).reshape(gw, gh).T if gw else a
        a = np.array([inv(list(row), gx) for row in a], dtype=ll.dtype).reshape(gh, gw) if gh else a
        ll = a
    return ll


@pytest.mark.parametrize("transform", ["53", "97"])
def test_rule_is_the_inverse_transforms_dependency_2d(transform):
    """A 13 x 10 tile-component at origin (3, 5), two levels: perturb every coefficient of every
    band; the set that changes a sample is the rule's band masks for that one-sample region."""
    x0, y0, w, h, levels = 3, 5, 13, 10, 2
    rng = np.random.default_rng(11)
    shapes = {k: v.shape for k, v in RR.band_masks(np.zeros((h, w), bool), x0, y0, levels, transform).items()}
    dt = np.int64 if transform == "53" else np.float64
    hit = {k: np.zeros(s + (h, w), bool) for k, s in shapes.items()}   # [band][by][bx][y][x]
    for trial in range(2):
        base = {k: rng.integers(-40, 40, s).astype(dt) + (0.37 if transform == "97" else 0) for k, s in shapes.items()}
        ref = _inv2d_levels(base, x0, y0, w, h, levels, transform)
        for k, s in shapes.items():
            for by in range(s[0]):
                for bx in range(s[1]):
                    # (5/3 rounds: a far coefficient weighs 1/256 at the sample, so some steps are large)
                    for delta in (4, 17, -5, 64, 4096, 1 << 14):
                        c = {q: v.copy() for q, v in base.items()}
                        c[k][by, bx] += delta
                        hit[k][by, bx] |= _inv2d_levels(c, x0, y0, w, h, levels, transform) != ref
    for y in range(h):
        for x in range(w):
            m = np.zeros((h, w), bool)
            m[y, x] = True
            want = RR.band_masks(m, x0, y0, levels, transform)
            for k in shapes:
                assert np.array_equal(hit[k][:, :, y, x], want[k]), (transform, x, y, k)


# ------------------------------------------------------------------------------- gk_probe_encode_roi
def _refused(match, shape=(3, 88, 72), prec=8, params=None, **kw):
    with pytest.raises(ValueError, match=match):
        G.probe_encode_roi(shape, prec, params, **kw)


def test_probe_refusals():
    ok = [(8, 8, 24, 40)]
    _refused("together with roi_compno / roi_shift", params=G.default_params(roi=(0, 11)), rects=ok)
    _refused("outside the 72 x 88 image", rects=[(8, 8, 73, 40)])
    _refused("outside the 72 x 88 image", rects=[(8, 8, 24, 89)])
    _refused("empty rectangle", rects=[(8, 8, 8, 40)])
    _refused("empty rectangle", rects=[(30, 8, 24, 40)])
    _refused("the mask is 70 x 88, the image 72 x 88", mask=np.ones((88, 70), np.uint8))
    _refused("the mask is 72 x 80, the image 72 x 88", mask=np.ones((80, 72), np.uint8))
    _refused("component index 3 past the last", rects=ok, components=[0, 3])
    _refused("empty region", mask=np.zeros((88, 72), np.uint8))
    _refused("empty region")
    _refused("shift 10 is below the smallest legal shift 11 of component 0", rects=ok, shift=10)
    _refused("ROI shift must be below 32", rects=ok, shift=32)
    # the same description, accepted
    assert G.probe_encode_roi((3, 88, 72), 8, rects=ok, mask=np.eye(88, 72, dtype=np.uint8)) == [11, 11, 11]
    assert G.probe_encode_roi((3, 88, 72), 8, rects=ok, components=[1], shift=12) == [0, 12, 0]


def _nominal_mb(cs):
    """The largest band bit-plane count of a stream: exponent + guard bits - 1 over the QCD's bands."""
    b = M.body(cs, 0xff5c)
    guard, style = b[0] >> 5, b[0] & 31
    if style == 0:
        expn = [v >> 3 for v in b[1:]]
    else:
        assert style == 2
        expn = [b[k] >> 3 for k in range(1, len(b), 2)]
    return max(expn) + guard - 1


def test_probe_shift_is_the_nominal_bitplane_count():
    """8-bit RGB, 5/3 with RCT and 9/7 (three resolutions: with more the doubled count passes the
    Part-1 coder's 25 planes and the description is refused, see below): the shift of shift=0 is
    the largest band bit-plane count of the plain stream, re-derived from its QCD and guard bits.
    The plain streams are the oracle's (no GPU here)."""
    import oracle as O
    img = np.random.default_rng(3).integers(0, 256, (3, 40, 48)).astype(np.int32)
    for irrev, numres in ((False, 6), (True, 3)):
        cs = O.encode(img, 8, numres=numres, irreversible=irrev)
        p = G.default_params(numresolution=numres, irreversible=irrev)
        assert G.probe_encode_roi(img.shape, 8, p, rects=[(4, 4, 20, 20)]) == [_nominal_mb(cs)] * 3
    # 9/7 at the default six resolutions: the LL band alone has 15 bit-planes
    _refused("ROI shift too large for this precision", shape=img.shape, params=G.default_params(irreversible=True),
             rects=[(4, 4, 20, 20)])


def test_probe_16_bit_part1_is_refused():
    _refused("ROI shift too large for this precision", shape=(1, 64, 64), prec=16, rects=[(4, 4, 20, 20)])


# -------------------------------------------------------------------------- Python argument checks
def test_argument_checks():
    for bad in ([(1, 2, 3)], [(0, 0, -1, 4)], [(0, 0, 1 << 32, 4)]):
        with pytest.raises(ValueError, match="a rectangle is"):
            G.probe_encode_roi((1, 16, 16), 8, rects=bad)
    with pytest.raises(ValueError, match="an \\(H, W\\) array"):
        G.probe_encode_roi((1, 16, 16), 8, mask=np.ones(16, np.uint8))
    with pytest.raises(ValueError, match="component indices"):
        G.probe_encode_roi((1, 16, 16), 8, rects=[(0, 0, 4, 4)], components=[-1])
    with pytest.raises(ValueError, match="shift is"):
        G.probe_encode_roi((1, 16, 16), 8, rects=[(0, 0, 4, 4)], shift=-1)
    for name in ("gk_set_encode_roi", "gk_probe_encode_roi", "gk_roi_band_mask"):
        assert name in G.EXPORTS
    # a mask of any dtype counts its non-zero elements
    assert G.probe_encode_roi((1, 16, 16), 8, mask=np.eye(16) * 0.5) == [11]
