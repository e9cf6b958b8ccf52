"""NumPy restatement of the end of Grok's post-processing (GrkDecompress::postProcess,
bin/jp2/grk_decompress.cpp:1444-1494): convert_gray_to_rgb and scale_component
(bin/common/convert.cpp:96-207), the clip rule the engine builds in place of Grok's clip<T>
(DESIGN.md R-BUG-11), and the pack into (H, W, C) pixels.  Layered on display_ref.post_process;
the checker of tests/test_pixels.py (known answers, CPU) and tests/test_gpu_pixels.py.

scale_component up: (int32_t)lrintf((float)v * scale) with scale = (float)newMax / (float)oldMax,
a float32 quotient taken first, then one float32 product per sample, rounded to nearest, ties to
even (np.rint).  Down: C integer division by 2^(old - new), truncating toward zero."""
import numpy as np

import display_ref as R


def parse(spec):
    """[(prec, "C" | "S")] of a -p string or such a list (None / "" / []: no list)."""
    if not spec:
        return []
    if isinstance(spec, str):
        out = []
        for item in spec.split(","):
            mode = "C"
            if item[-1] in "CS":
                item, mode = item[:-1], item[-1]
            out.append((int(item), mode))
        return out
    return [(int(p), m) for p, m in spec]


def scale_component(v, old, new, sgnd):
    """scale_component (:117-146) on an int array of precision `old`."""
    v = np.asarray(v).astype(np.int32)
    if new == old:
        return v
    if new > old:
        new_max = np.float32(1 << (new - 1) if sgnd else (1 << new) - 1)
        old_max = np.float32(1 << (old - 1) if sgnd else (1 << old) - 1)
        scale = np.float32(new_max / old_max)
        assert scale.dtype == np.float32
        prod = v.astype(np.float32) * scale
        assert prod.dtype == np.float32
        return np.rint(prod).astype(np.int32)
    d = 1 << (old - new)
    q = np.abs(v.astype(np.int64)) // d          # C division truncates toward zero
    return (np.sign(v) * q).astype(np.int32)


def clip_component(v, new, sgnd):
    """The clamp to the forced precision's range with the channel's sign."""
    lo, hi = (-(1 << (new - 1)), (1 << (new - 1)) - 1) if sgnd else (0, (1 << new) - 1)
    return np.clip(np.asarray(v).astype(np.int32), lo, hi).astype(np.int32)


def gray_to_rgb(planes, comps, colour_space):
    """postProcess :1444-1468 / convert_gray_to_rgb: (planes, comps, colour_space, replicated)."""
    if colour_space == R.CS_SRGB:
        return planes, comps, colour_space, False
    if colour_space != R.CS_GRAY:
        raise ValueError("don't know how to convert image to RGB colorspace (%d)" % colour_space)
    return [planes[0]] * 3 + list(planes[1:]), [comps[0]] * 3 + list(comps[1:]), R.CS_SRGB, True


def force_precision(planes, comps, spec):
    """postProcess :1469-1494: channel k takes entry min(k, n - 1); 0 keeps its precision."""
    lst = parse(spec)
    if not lst:
        return planes, comps
    out_p, out_c = [], []
    for k, (p, (dx, dy, prec, sgnd)) in enumerate(zip(planes, comps)):
        new, mode = lst[min(k, len(lst) - 1)]
        new = new or prec
        out_p.append(scale_component(p, prec, new, sgnd) if mode == "S" else clip_component(p, new, sgnd))
        out_c.append((dx, dy, new, sgnd))
    return out_p, out_c


def post_process(planes, comps, colour_space, bounds, rgb=False, upsample=False, force_rgb=False, precision=None,
                 odd_first=None):
    """display_ref.post_process, then grey to RGB and the precision list.  Returns (planes, comps,
    colour_space)."""
    planes, comps, cs, _, _ = R.post_process(planes, comps, colour_space, bounds, rgb, upsample, odd_first)
    return finish(planes, comps, cs, force_rgb, precision)


def finish(planes, comps, colour_space, force_rgb=False, precision=None):
    """Grey to RGB and the precision list on an image that display_ref.post_process (or a decode
    under the rgb / upsample flags) has produced.  Returns (planes, comps, colour_space)."""
    planes, comps, cs = list(planes), [tuple(c) for c in comps], colour_space
    if force_rgb:   # (the colour-space rule of :1335-1341 applies under either flag)
        n = len(planes)
        if cs != R.CS_SYCC and n == 3 and comps[0][0] == comps[0][1] and comps[1][0] != 1:
            cs = R.CS_SYCC
        elif n <= 2:
            cs = R.CS_GRAY
        planes, comps, cs, _ = gray_to_rgb(planes, comps, cs)
    planes, comps = force_precision(planes, comps, precision)
    return planes, comps, cs


def pack(planes):
    """(H, W, C) pixels of equally sized planes."""
    return np.stack([np.asarray(p) for p in planes], -1)
