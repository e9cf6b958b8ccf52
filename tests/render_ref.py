"""The render rule in numpy int64: what gk_set_decode_render makes of the int32
pixels of a pixel call, the bin rule of gk_decode_levels and the percentile rule of Levels.window.
It imports nothing from the engine; Python's // and numpy's floor_divide are floor divisions."""
import numpy as np


def level(v, lo, hi):
    """The window (lo, hi), lo != hi, of int32 samples v -> 0 .. 255; lo > hi inverts."""
    lo, hi = int(lo), int(hi)
    if lo == hi:
        raise ValueError("render: lo == hi")
    if lo > hi:
        return 255 - level(v, hi, lo)
    u = np.clip(np.asarray(v).astype(np.int64), lo, hi)
    return (2 * 255 * (u - lo) + (hi - lo)) // (2 * (hi - lo))


def _entry(lst, k):
    return lst[min(k, len(lst) - 1)]


def levels_of(pix, windows, curve=None):
    """t_k of every channel of (H, W, C) pixels: window min(k, n - 1), then the optional curve."""
    pix = np.asarray(pix)
    t = np.stack([level(pix[:, :, k], *_entry(windows, k)) for k in range(pix.shape[2])], axis=2)
    if curve is not None:
        curve = np.asarray(curve)
        assert curve.shape == (256,) and curve.dtype == np.uint8
        t = curve.astype(np.int64)[t]
    return t


def render(pix, mode, windows, tints=None, curve=None, map=None):
    """(H, W, C) int32 pixels -> (H, W, C or 3) uint8 display pixels."""
    pix = np.asarray(pix)
    c = pix.shape[2]
    t = levels_of(pix, windows, curve)
    if mode == "window":
        return t.astype(np.uint8)
    if mode == "map":
        assert c == 1, "map mode takes exactly one channel"
        m = np.asarray(map)
        assert m.shape == (256, 3) and m.dtype == np.uint8
        return m[t[:, :, 0]]
    if mode == "blend":
        assert 1 <= c <= 16
        tint = np.array([_entry(tints, k) for k in range(c)], np.int64)   # (C, 3)
        assert tint.any(), "blend mode with every tint zero"
        s = np.einsum("hwk,kc->hwc", t, tint)
        return np.minimum(255, (2 * s + 255) // 510).astype(np.uint8)
    raise ValueError(mode)


def gamma_curve(g):
    """round(255 (t / 255)^(1 / g)), the table the Python side builds."""
    t = np.arange(256, dtype=np.float64) / 255.0
    return np.floor(255.0 * t ** (1.0 / float(g)) + 0.5).astype(np.uint8)


def bin_of(v, origin, shift, bins):
    """b = clamp(floor((v - origin) / 2^shift), 0, bins - 1)."""
    return np.clip((np.asarray(v).astype(np.int64) - int(origin)) // (1 << int(shift)), 0, bins - 1)


def stats(pix, bins=0, entries=((0, 0),)):
    """min, max, sum, count and hist per channel of (H, W, C) int32 pixels, as gk_decode_levels."""
    pix = np.asarray(pix).astype(np.int64)
    out = []
    for k in range(pix.shape[2]):
        p = pix[:, :, k]
        hist = None
        if bins:
            origin, shift = _entry(list(entries), k)
            hist = np.bincount(bin_of(p, origin, shift, bins).ravel(), minlength=bins).astype(np.uint64)
        out.append(dict(min=int(p.min()), max=int(p.max()), sum=int(p.sum()), count=p.size, hist=hist))
    return out


def auto_bins(mn, mx, bins):
    """The binning Engine.levels chooses: origin = min and the smallest shift that fits max."""
    shift = 0
    while ((mx - mn) >> shift) >= bins:
        shift += 1
    return mn, shift


def percentile_window(hist, origin, shift, low, high, per=1000):
    """With N pixels: lo is the lower edge of the first bin whose cumulative count reaches
    max(1, ceil(N low / per)), hi the last value of the first bin whose cumulative count reaches
    ceil(N high / per); hi = lo + 1 if they meet."""
    h = [int(v) for v in hist]
    n = sum(h)
    cum = np.cumsum(h)
    need_lo, need_hi = max(1, -(-n * low // per)), -(-n * high // per)
    b_lo = int(np.argmax(cum >= need_lo))
    b_hi = int(np.argmax(cum >= need_hi))
    lo, hi = origin + (b_lo << shift), origin + ((b_hi + 1) << shift) - 1
    return (lo, hi) if hi > lo else (lo, lo + 1)
