"""A view restated in numpy: the size and reduce resolution of gk_view, the exact area average of
k_view (gk_view.hip) in int64, and the orientation.  DESIGN.md §3 has the rule in words; this file
shares no code with the engine or with the binding."""
import numpy as np


def cdiv(a, b):
    return -(-a // b)


def scaled(a, num, den):
    """Side `a` scaled by num / den, rounded half up, at least 1."""
    return max(1, (2 * a * num + den) // (2 * den))


def resolve_size(W, H, out_w=0, out_h=0, fit=False):
    """(out_w, out_h) before rotation for a region of W x H; ValueError for what the engine refuses."""
    if not out_w and not out_h:
        raise ValueError("both sizes 0")
    if not out_h:
        out_h = scaled(out_w, H, W)
    elif not out_w:
        out_w = scaled(out_h, W, H)
    elif fit:
        if out_w * H <= out_h * W:
            out_h = scaled(out_w, H, W)
        else:
            out_w = scaled(out_h, W, H)
    if out_w > W or out_h > H:
        raise ValueError("upscaling")
    return out_w, out_h


def reduced(region, r, origin=(0, 0)):
    """The region (image relative) on the canvas reduced r times: every edge ceil(x / 2^r)."""
    x0, y0, x1, y1 = region
    ox, oy = origin
    return cdiv(x0 + ox, 1 << r), cdiv(y0 + oy, 1 << r), cdiv(x1 + ox, 1 << r), cdiv(y1 + oy, 1 << r)


def choose_reduce(region, out_w, out_h, max_reduce, origin=(0, 0)):
    """The largest r <= max_reduce whose reduced region is still at least out_w x out_h."""
    best = 0
    for r in range(max_reduce + 1):
        x0, y0, x1, y1 = reduced(region, r, origin)
        if x1 - x0 >= out_w and y1 - y0 >= out_h:
            best = r
    return best


def weights(rn, on):
    """(on, rn) int64: the overlap of output cell i, [i rn, (i + 1) rn), with source cell s,
    [s on, (s + 1) on), in units of 1 / on of a source sample."""
    i = np.arange(on, dtype=np.int64)[:, None]
    s = np.arange(rn, dtype=np.int64)[None, :]
    return np.clip(np.minimum((i + 1) * rn, (s + 1) * on) - np.maximum(i * rn, s * on), 0, None)


def resample(a, out_w, out_h):
    """a: (rh, rw, C) integers -> (out_h, out_w, C) int64: floor((2 S + rw rh) / (2 rw rh)) with
    S = sum wy wx v; numpy's // is floor division."""
    a = np.asarray(a).astype(np.int64)
    rh, rw = a.shape[:2]
    wy, wx = weights(rh, out_h), weights(rw, out_w)
    s = np.einsum("js,stc->jtc", wy, a)
    s = np.einsum("it,jtc->jic", wx, s)
    return (2 * s + rw * rh) // (2 * rw * rh)


def orient(a, rotate=0, mirror=False):
    """Mirror left-right, then rotate clockwise by `rotate` degrees."""
    if mirror:
        a = np.fliplr(a)
    return np.ascontiguousarray(np.rot90(a, k=-(rotate // 90)))


def view(a, out_w, out_h, rotate=0, mirror=False):
    """The written image of a view whose reduced region decodes to a (rh, rw, C)."""
    return orient(resample(a, out_w, out_h), rotate, mirror)
