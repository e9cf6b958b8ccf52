"""grok_amd — MI355X-native JPEG 2000 tile pipeline (host-side Python mirror).

The product is the C-ABI library ``libgrok_amd.so`` (include/grok_amd.h):
HIP kernels for gfx950 plus the native host engine (T2, codestream).  This
module binds it with ctypes and mirrors the reference's compress/decompress
call shape (grk_compress_* / grk_decompress_*, grok.h:1261-1451) for tests
and the benchmark.  There is no CPU fallback: if the extension cannot be
loaded, or no GPU is present, calls raise.
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# GROK_AMD_LIB: another in-tree build of the library (A/B measurements of kernel variants)
LIB_PATH = os.environ.get("GROK_AMD_LIB") or os.path.join(HERE, "libgrok_amd.so")

GK_MAXRLVLS = 33
GK_MAX_LAYERS = 100

# Exported symbols declared in include/grok_amd.h (checked by tests/test_capi.py).
EXPORTS = ("gk_create", "gk_destroy", "gk_set_default_params", "gk_encode", "gk_encode_tiles", "gk_main_header",
           "gk_jp2_header", "gk_decode_header", "gk_probe_header", "gk_decode", "gk_decode_window", "gk_get_timings",
           "gk_last_error", "gk_version", "gk_set_decode_layers", "gk_set_decode_reduce",
           "gk_set_window_rule", "gk_set_subsampling", "gk_probe_components", "gk_header_components",
           "gk_probe_colour", "gk_header_colour", "gk_header_icc", "gk_set_decode_colour", "gk_probe_icc",
           "gk_probe_stream_components", "gk_set_decode_display", "gk_probe_display", "gk_set_decode_precision",
           "gk_probe_output", "gk_decode_pixels", "gk_decode_window_pixels", "gk_encode_pixels",
           "gk_set_encode_colour", "gk_jp2_boxes", "gk_header_cielab", "gk_probe_cielab",
           "gk_set_encode_convert", "gk_probe_encode_convert", "gk_set_default_transcode", "gk_transcode",
           "gk_probe_transcode", "gk_set_encode_roi", "gk_probe_encode_roi", "gk_roi_band_mask",
           "gk_set_encode_quant", "gk_probe_encode_quant", "gk_get_encode_quant", "gk_probe_view",
           "gk_decode_view_pixels", "gk_set_decode_render", "gk_probe_render", "gk_decode_levels",
           "gk_probe_tensor", "gk_decode_view_tensor")
GK_TENSOR_F32, GK_TENSOR_F16, GK_TENSOR_BF16 = 1, 2, 3   # gk_tensor::dtype
GK_RENDER_WINDOW, GK_RENDER_MAP, GK_RENDER_BLEND = 1, 2, 3   # gk_render::mode
GK_RENDER_MAX_CHANNELS, GK_LEVELS_MAX_BINS = 16, 4096
GK_QUANT_STEP, GK_QUANT_BYTES, GK_QUANT_PSNR = 1, 2, 3   # gk_encode_quant::mode
GK_QUANT_FOR_TILES, GK_QUANT_FOR_BLOCKS = 0x100, 0x200   # gk_probe_encode_quant: the call asked about
GK_TRANSCODE_HT, GK_TRANSCODE_PART1 = 1, 2   # gk_transcode_params::target
GK_MAX_CHANNELS = 256
GK_DISPLAY_RGB, GK_DISPLAY_UPSAMPLE, GK_DISPLAY_FORCE_RGB, GK_DISPLAY_ICC = 1, 2, 4, 8   # gk_set_decode_display flags
GK_PREC_CLIP, GK_PREC_SCALE = 0, 1   # gk_precision::mode (grk_precision_mode)


class Precision(ctypes.Structure):
    """gk_precision (include/grok_amd.h): one entry of a forced-precision list."""
    _fields_ = [("prec", ctypes.c_uint8), ("mode", ctypes.c_uint8)]


def parse_precision(spec):
    """A forced-precision list as [(prec, "C" | "S")]: `spec` is None / [] (no list), such a list, or
    grk_decompress's -p string (parsePrecision, grk_decompress.cpp:212-330): comma-separated
    entries of a precision 1..32 and an optional mode letter C (clip, the default) or S (scale).
    (0 keeps a channel's precision and is accepted in a list given as tuples, and here.)"""
    if spec is None:
        return []
    if isinstance(spec, str):
        out = []
        for item in spec.split(","):
            item = item.strip()
            mode = "C"
            if item and item[-1] in "CS":
                item, mode = item[:-1], item[-1]
            if not item.isdigit() or int(item) > 32:
                raise ValueError("precision %r: expected {prec}[C|S] with a precision of 1..32" % item)
            out.append((int(item), mode))
        return out
    out = []
    for prec, mode in spec:
        mode = {GK_PREC_CLIP: "C", GK_PREC_SCALE: "S"}.get(mode, mode)
        if mode not in ("C", "S") or not 0 <= int(prec) <= 255:
            raise ValueError("precision entry (%r, %r): expected (prec, 'C' | 'S')" % (prec, mode))
        out.append((int(prec), mode))
    return out


class View(ctypes.Structure):
    """gk_view (include/grok_amd.h): a region, its output size and its orientation."""
    _fields_ = [("x0", ctypes.c_uint32), ("y0", ctypes.c_uint32), ("x1", ctypes.c_uint32), ("y1", ctypes.c_uint32),
                ("out_w", ctypes.c_uint32), ("out_h", ctypes.c_uint32), ("fit", ctypes.c_uint32),
                ("rotate", ctypes.c_uint32), ("mirror", ctypes.c_uint32)]


class ViewResult(ctypes.Structure):
    """gk_view_result: what a view resolved to."""
    _fields_ = [("reduce", ctypes.c_uint32), ("rx0", ctypes.c_uint32), ("ry0", ctypes.c_uint32),
                ("rx1", ctypes.c_uint32), ("ry1", ctypes.c_uint32), ("out_w", ctypes.c_uint32),
                ("out_h", ctypes.c_uint32), ("pix_w", ctypes.c_uint32), ("pix_h", ctypes.c_uint32),
                ("channels", ctypes.c_uint32), ("prec", ctypes.c_uint32), ("sgnd", ctypes.c_uint32)]

    def __repr__(self):
        return "ViewResult(%s)" % ", ".join("%s=%d" % (f, getattr(self, f)) for f, _ in self._fields_)


def _view(region, size, width, height, fit, rotate, mirror):
    """The gk_view of decode_view's / probe_view's keyword arguments."""
    if size is not None:
        if width is not None or height is not None:
            raise ValueError("view: give size=(w, h) or width= / height=, not both")
        width, height = size
    x0, y0, x1, y1 = region if region is not None else (0, 0, 0, 0)
    vals = [x0, y0, x1, y1, width or 0, height or 0, int(fit), rotate, int(mirror)]
    if any(int(v) != v or not 0 <= v < 2 ** 32 for v in vals):
        raise ValueError("view: every field is an integer in 0 .. 2^32 - 1")
    return View(*[int(v) for v in vals])


def _view_size(w, h, width=None, height=None, fit=False):
    """gk_view's size rule for a region of w x h: (out_w, out_h) before rotation.  Both given: as
    they are; one of them: the other keeps the aspect, max(1, (2 a h + w) // (2 w)); fit: the
    largest size of the region's aspect inside width x height.  The engine's own resolution,
    which also refuses upscaling, is gk_probe_view's, and Engine.decode_view sizes its array from
    that; this restatement serves only a codestream in device memory, which cannot be probed."""
    ow, oh = int(width or 0), int(height or 0)
    if not ow and not oh:
        raise ValueError("view: out_w and out_h are both 0")
    if not oh:
        oh = max(1, (2 * ow * h + w) // (2 * w))
    elif not ow:
        ow = max(1, (2 * oh * w + h) // (2 * h))
    elif fit:
        if ow * h <= oh * w:
            oh = max(1, (2 * ow * h + w) // (2 * w))
        else:
            ow = max(1, (2 * oh * w + h) // (2 * h))
    return ow, oh


def parse_iiif(w, h, region="full", size="max", rotation="0"):
    """IIIF Image API 3.0 region / size / rotation strings for an image of w x h, as the keyword
    arguments of Engine.decode_view / probe_view (region, width, height, fit, rotate, mirror).
    region: full | square (centred) | x,y,w,h | pct:x,y,w,h (cut at the image's edges, as the API
    asks); size: max | w, | ,h | pct:n | w,h | !w,h (!w,h is held to the region's size, as the API
    asks; every other form above the region's size is upscaling); rotation: 0 | 90 | 180 | 270
    with an optional leading ! (mirror).  Upscaling (^) and other angles raise ValueError."""
    from fractions import Fraction

    def numbers(text, n, what, whole):
        parts = text.split(",")
        if len(parts) != n:
            raise ValueError("iiif %s %r: expected %d comma-separated numbers" % (what, text, n))
        try:
            vals = [Fraction(p) for p in parts]
        except (ValueError, ZeroDivisionError):
            raise ValueError("iiif %s %r: not a number" % (what, text)) from None
        if any(v < 0 for v in vals) or (whole and any(v.denominator != 1 for v in vals)):
            raise ValueError("iiif %s %r: expected %s" % (what, text, "whole numbers" if whole else "numbers >= 0"))
        return vals

    half_up = lambda q: int((2 * q + 1) // 2)
    w, h = int(w), int(h)
    if w <= 0 or h <= 0:
        raise ValueError("iiif: an image of %d x %d" % (w, h))
    if region == "full":
        box = None
    elif region == "square":
        side = min(w, h)
        box = ((w - side) // 2, (h - side) // 2, (w - side) // 2 + side, (h - side) // 2 + side)
    else:
        pct = region.startswith("pct:")
        x, y, rw, rh = numbers(region[4:] if pct else region, 4, "region", not pct)
        if pct:
            x, y, rw, rh = x * w / 100, y * h / 100, rw * w / 100, rh * h / 100
        box = (half_up(x), half_up(y), min(w, half_up(x + rw)), min(h, half_up(y + rh)))
        if rw == 0 or rh == 0 or box[0] >= box[2] or box[1] >= box[3]:
            raise ValueError("iiif region %r: empty, or outside the image of %d x %d" % (region, w, h))
    bw, bh = (box[2] - box[0], box[3] - box[1]) if box else (w, h)
    if box == (0, 0, w, h):
        box = None
    if "^" in size:
        raise ValueError("iiif size %r: upscaling (^) is out of scope" % size)
    fit = False
    if size == "max":
        width, height = bw, bh
    elif size.startswith("pct:"):
        n, = numbers(size[4:], 1, "size", False)
        if n > 100:
            raise ValueError("iiif size %r: upscaling is out of scope" % size)
        width, height = max(1, half_up(bw * n / 100)), max(1, half_up(bh * n / 100))
    elif size.startswith("!"):
        width, height = (int(v) for v in numbers(size[1:], 2, "size", True))
        width, height, fit = min(width, bw), min(height, bh), True
    elif size.endswith(",") and size.count(",") == 1:
        (width,), height = (int(v) for v in numbers(size[:-1], 1, "size", True)), None
    elif size.startswith(",") and size.count(",") == 1:
        width, (height,) = None, (int(v) for v in numbers(size[1:], 1, "size", True))
    else:
        width, height = (int(v) for v in numbers(size, 2, "size", True))
    if width == 0 or height == 0:
        raise ValueError("iiif size %r: a size of 0" % size)
    if (width or 0) > bw or (height or 0) > bh:
        raise ValueError("iiif size %r: upscaling of a region of %d x %d is out of scope" % (size, bw, bh))
    mirror = rotation.startswith("!")
    try:
        angle = Fraction(rotation[1:] if mirror else rotation)
    except (ValueError, ZeroDivisionError):
        raise ValueError("iiif rotation %r: not a number" % rotation) from None
    if angle not in (0, 90, 180, 270):
        raise ValueError("iiif rotation %r: only 0, 90, 180 and 270 are supported" % rotation)
    return dict(region=box, width=width, height=height, fit=fit, rotate=int(angle), mirror=mirror)


class RenderChannel(ctypes.Structure):
    """gk_render_channel: one channel's window and its BLEND tint."""
    _fields_ = [("lo", ctypes.c_int32), ("hi", ctypes.c_int32), ("tint", ctypes.c_uint8 * 3)]


class Render(ctypes.Structure):
    """gk_render (include/grok_amd.h): how the pixel calls' int32 samples become 8-bit display pixels."""
    _fields_ = [("mode", ctypes.c_uint32), ("n", ctypes.c_uint32), ("ch", ctypes.POINTER(RenderChannel)),
                ("curve", ctypes.POINTER(ctypes.c_uint8)), ("map", ctypes.POINTER(ctypes.c_uint8))]


class RenderResult(ctypes.Structure):
    """gk_render_result: the rendered output's channels, precision, sign and colour space."""
    _fields_ = [("channels", ctypes.c_uint32), ("prec", ctypes.c_uint32), ("sgnd", ctypes.c_uint32),
                ("colour_space", ctypes.c_uint32)]

    def __repr__(self):
        return "RenderResult(%s)" % ", ".join("%s=%d" % (f, getattr(self, f)) for f, _ in self._fields_)


class LevelsBins(ctypes.Structure):
    """gk_levels_bins: bin b of a channel holds origin + b * 2^shift .. origin + (b + 1) * 2^shift - 1."""
    _fields_ = [("origin", ctypes.c_int32), ("shift", ctypes.c_uint32)]


class ChannelLevels(ctypes.Structure):
    """gk_channel_levels: one channel's statistics."""
    _fields_ = [("min", ctypes.c_int32), ("max", ctypes.c_int32), ("sum", ctypes.c_int64), ("count", ctypes.c_uint64)]


class Tensor(ctypes.Structure):
    """gk_tensor (include/grok_amd.h): where and how a view is written as floats."""
    _fields_ = [("data", ctypes.c_void_p), ("on_device", ctypes.c_int32), ("dtype", ctypes.c_uint32),
                ("stride_c", ctypes.c_int64), ("stride_y", ctypes.c_int64), ("stride_x", ctypes.c_int64),
                ("n", ctypes.c_uint32), ("scale", ctypes.POINTER(ctypes.c_float)), ("bias", ctypes.POINTER(ctypes.c_float))]


_TENSOR_DTYPES = {"float32": GK_TENSOR_F32, "float16": GK_TENSOR_F16, "bfloat16": GK_TENSOR_BF16}


def _tensor_dtype(dtype):
    """gk_tensor::dtype of a name, a numpy dtype or a torch dtype."""
    name = str(dtype).replace("torch.", "")
    if name not in _TENSOR_DTYPES:
        name = getattr(dtype, "__name__", name)   # (np.float32 and its like)
    if name not in _TENSOR_DTYPES:
        raise ValueError("tensor: dtype %r (float32, float16 or bfloat16)" % (dtype,))
    return _TENSOR_DTYPES[name]


def _tensor_affine(mean=None, std=None, unit=None, prec=None, sgnd=False):
    """(scale, bias) as float32 arrays for x = (v / unit - mean_k) / std_k: scale_k = 1 / (unit std_k)
    and bias_k = -mean_k / std_k, computed in float64 and rounded once to float32.  mean / std: a
    number or one per channel (the shorter list's last entry repeats; None: 0 / 1).  unit: None is
    2^prec - 1 of an unsigned view; a signed view has no such default."""
    if unit is None:
        if sgnd:
            raise ValueError("tensor: a signed view has no default unit: give unit=")
        if not prec:
            raise ValueError("tensor: give unit= (the view's precision is not known)")
        unit = 2 ** int(prec) - 1
    as_list = lambda x, d: [float(e) for e in x] if isinstance(x, (list, tuple, np.ndarray)) else [float(d if x is None else x)]
    m, s = as_list(mean, 0.0), as_list(std, 1.0)
    if not m or not s:
        raise ValueError("tensor: an empty mean or std")
    n = max(len(m), len(s))
    m = np.array([m[min(k, len(m) - 1)] for k in range(n)], np.float64)
    s = np.array([s[min(k, len(s) - 1)] for k in range(n)], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):   # (the engine names a result that is not finite)
        return (1.0 / (np.float64(unit) * s)).astype(np.float32), (-m / s).astype(np.float32)


def _tensor_description(dtype, strides, scale=None, bias=None, data=None, on_device=True):
    """The gk_tensor of a dtype, (stride_c, stride_y, stride_x) in elements and scale / bias (a
    number or one per channel; None: 1 / 0), and the arrays it points into."""
    as_f32 = lambda x, d: np.ascontiguousarray(np.atleast_1d(np.asarray(d if x is None else x, np.float64)).astype(np.float32).reshape(-1))
    if scale is None and bias is None:
        n, sc, bi = 0, None, None
    else:
        sc, bi = as_f32(scale, 1.0), as_f32(bias, 0.0)
        n = max(len(sc), len(bi))
        if not len(sc) or not len(bi):
            raise ValueError("tensor: an empty scale or bias")
        sc, bi = (np.concatenate([a, np.repeat(a[-1:], n - len(a))]) for a in (sc, bi))
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if a is not None else None
    t = Tensor(data, int(bool(on_device)), _tensor_dtype(dtype), int(strides[0]), int(strides[1]), int(strides[2]), n, fp(sc), fp(bi))
    return t, (sc, bi)


def probe_tensor(view_result, dtype, strides, scale=None, bias=None, on_device=True):
    """gk_probe_tensor: the extent in elements of a tensor of `dtype` ("float32", "float16",
    "bfloat16", or a numpy / torch dtype) with strides = (stride_c, stride_y, stride_x) in
    elements for a resolved view (probe_view's ViewResult), as Engine.decode_tensor would judge
    it; no engine or GPU needed.  on_device=False asks about a host tensor, which must be dense.
    Raises ValueError with the engine's refusal."""
    lib = load_library()
    t, keep = _tensor_description(dtype, strides, scale, bias, None, on_device)
    extent, msg = ctypes.c_uint64(0), ctypes.create_string_buffer(512)
    if lib.gk_probe_tensor(ctypes.byref(view_result), ctypes.byref(t), ctypes.byref(extent), msg, 512) != 0:
        raise ValueError(msg.value.decode())
    del keep
    return extent.value


def gamma_curve(g):
    """The 256-byte curve round(255 (t / 255)^(1 / g)), built on the host: the kernel never sees a float."""
    g = float(g)
    if not g > 0:
        raise ValueError("render: gamma must be positive")
    t = np.arange(256, dtype=np.float64) / 255.0
    return np.floor(255.0 * t ** (1.0 / g) + 0.5).astype(np.uint8)


def _render(mode, windows, tints, curve, map, gamma):
    """(gk_render or None, the arrays it points into) of set_decode_render's / probe_render's arguments."""
    if mode is None:
        return None, ()
    modes = {"window": GK_RENDER_WINDOW, "map": GK_RENDER_MAP, "blend": GK_RENDER_BLEND}
    if mode not in modes and mode not in modes.values():
        raise ValueError("render: mode %r (None, 'window', 'map' or 'blend')" % (mode,))
    windows = [tuple(int(v) for v in w) for w in (windows or [])]
    if any(len(w) != 2 or not all(-2 ** 31 <= v < 2 ** 31 for v in w) for w in windows):
        raise ValueError("render: windows are (lo, hi) pairs of int32 values")
    tints = [tuple(int(v) for v in t) for t in (tints or [])]
    if any(len(t) != 3 or not all(0 <= v <= 255 for v in t) for t in tints):
        raise ValueError("render: tints are (r, g, b) in 0 .. 255")
    if windows and tints and len(tints) != len(windows) and 1 not in (len(tints), len(windows)):
        raise ValueError("render: %d windows for %d tints" % (len(windows), len(tints)))
    n = max(len(windows), len(tints))
    ch = (RenderChannel * max(n, 1))()
    for k in range(n):
        lo, hi = windows[min(k, len(windows) - 1)] if windows else (0, 0)
        tint = tints[min(k, len(tints) - 1)] if tints else (0, 0, 0)
        ch[k] = RenderChannel(lo, hi, (ctypes.c_uint8 * 3)(*tint))
    if curve is not None and gamma is not None:
        raise ValueError("render: give curve= or gamma=, not both")
    if gamma is not None:
        curve = gamma_curve(gamma)
    keep = [ch]
    r = Render(modes.get(mode, mode), n, ch, None, None)
    if curve is not None:
        c = np.ascontiguousarray(curve)
        if c.dtype != np.uint8 or c.shape != (256,):
            raise ValueError("render: curve must be 256 uint8 values")
        keep.append(c)
        r.curve = c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    if map is not None:
        m = np.ascontiguousarray(map)
        if m.dtype != np.uint8 or m.shape != (256, 3):
            raise ValueError("render: map must be a (256, 3) uint8 array")
        keep.append(m)
        r.map = m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    return r, keep


class Levels:
    """What Engine.levels reports of a view's int32 pixels, per output channel: min, max, sum (exact), mean
    (sum / count as a float), count, and with bins the histogram hist[k] (uint64,
    bin b of channel k holding origin[k] + b * 2^shift[k] and the 2^shift[k] - 1 values after it;
    values outside the binned range are counted in the end bins)."""

    def __init__(self, stats, hist, origin, shift, view):
        self.min = [int(s.min) for s in stats]
        self.max = [int(s.max) for s in stats]
        self.sum = [int(s.sum) for s in stats]
        self.count = [int(s.count) for s in stats]
        self.mean = [s / c for s, c in zip(self.sum, self.count)]
        self.hist, self.origin, self.shift, self.view = hist, list(origin), list(shift), view

    def window(self, low, high, per=1000):
        """[(lo, hi)] per channel from the histogram, in integers: with N pixels, lo is the lower edge
        of the first bin whose cumulative count reaches max(1, ceil(N low / per)), hi the last value
        of the first bin whose cumulative count reaches ceil(N high / per); hi = lo + 1 if they meet."""
        if self.hist is None:
            raise ValueError("levels: no histogram (bins=0)")
        low, high, per = int(low), int(high), int(per)
        if not 0 <= low <= high <= per or per <= 0:
            raise ValueError("levels: 0 <= low <= high <= per")
        return [_percentile_window(self.hist[k], self.origin[k], self.shift[k], low, high, per) for k in range(len(self.min))]


def _percentile_window(hist, origin, shift, low, high, per):
    cum, n = 0, int(sum(int(v) for v in hist))
    need_lo, need_hi = max(1, -(-n * low // per)), -(-n * high // per)
    lo = hi = None
    for b, c in enumerate(hist):
        cum += int(c)
        if lo is None and cum >= need_lo:
            lo = origin + (b << shift)
        if hi is None and cum >= need_hi:
            hi = origin + ((b + 1) << shift) - 1
        if lo is not None and hi is not None:
            break
    if lo is None or hi is None:
        raise ValueError("levels: an empty histogram")
    if hi <= lo:
        hi = lo + 1
    return lo, hi


def _precision_array(spec):
    lst = parse_precision(spec)
    arr = (Precision * max(len(lst), 1))()
    for i, (prec, mode) in enumerate(lst):
        arr[i] = Precision(prec, GK_PREC_SCALE if mode == "S" else GK_PREC_CLIP)
    return arr, len(lst)


class Poc(ctypes.Structure):
    """gk_poc (include/grok_amd.h): one progression order change."""
    _fields_ = [("resS", ctypes.c_uint32), ("compS", ctypes.c_uint32), ("layE", ctypes.c_uint32),
                ("resE", ctypes.c_uint32), ("compE", ctypes.c_uint32), ("prog", ctypes.c_int32)]


class CParameters(ctypes.Structure):
    """gk_cparameters (include/grok_amd.h) — subset of grk_cparameters (grok.h:466-590)."""
    _fields_ = [
        ("numlayers", ctypes.c_uint16),
        ("layer_rate", ctypes.c_double * GK_MAX_LAYERS),
        ("numresolution", ctypes.c_uint8),
        ("cblockw_init", ctypes.c_uint32), ("cblockh_init", ctypes.c_uint32),
        ("cblk_sty", ctypes.c_uint8), ("irreversible", ctypes.c_uint8), ("mct", ctypes.c_uint8),
        ("numgbits", ctypes.c_uint8), ("csty", ctypes.c_uint8),
        ("res_spec", ctypes.c_uint32),
        ("prcw_init", ctypes.c_uint32 * GK_MAXRLVLS), ("prch_init", ctypes.c_uint32 * GK_MAXRLVLS),
        ("write_comment", ctypes.c_uint8),
        ("tile_size_on", ctypes.c_uint8),
        ("t_width", ctypes.c_uint32), ("t_height", ctypes.c_uint32),
        ("writeTLM", ctypes.c_uint8), ("writePLT", ctypes.c_uint8),
        ("cod_format", ctypes.c_int32), ("prog_order", ctypes.c_int32),
        ("enableTilePartGeneration", ctypes.c_uint8), ("newTilePartProgressionDivider", ctypes.c_char),
        ("roi_compno", ctypes.c_int32), ("roi_shift", ctypes.c_uint32),
        ("numpocs", ctypes.c_uint32), ("pocs", Poc * 32),
        ("allocationByQuality", ctypes.c_uint8), ("layer_distortion", ctypes.c_double * GK_MAX_LAYERS),
        ("tx0", ctypes.c_uint32), ("ty0", ctypes.c_uint32),
        ("num_comments", ctypes.c_uint32), ("comment", ctypes.c_char_p * 256), ("comment_len", ctypes.c_uint16 * 256),
        ("is_binary_comment", ctypes.c_uint8 * 256),
    ]


class TranscodeParams(ctypes.Structure):
    """gk_transcode_params (include/grok_amd.h)."""
    _fields_ = [(n, ctypes.c_uint32) for n in ("target", "tlm", "plt", "com")]


def _transcode_params(target, tlm=False, plt=False, com=True):
    """target: "ht" | "part1" (or GK_TRANSCODE_HT / GK_TRANSCODE_PART1)."""
    t = {"ht": GK_TRANSCODE_HT, "part1": GK_TRANSCODE_PART1}.get(target, target)
    if t not in (GK_TRANSCODE_HT, GK_TRANSCODE_PART1):
        raise ValueError("transcode target %r: expected 'ht' or 'part1'" % (target,))
    return TranscodeParams(t, int(bool(tlm)), int(bool(plt)), int(bool(com)))


class ImageInfo(ctypes.Structure):
    """gk_image_info; sample_bytes: 0/4 = int32 planes, 1/2 = planar 8/16-bit samples."""
    _fields_ = [(n, ctypes.c_uint32) for n in ("w", "h", "numcomps", "prec", "sgnd", "sample_bytes", "x0", "y0")]


class Timings(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in ("mct_ms", "dwt_ms", "t1_ms", "t2_ms", "assemble_ms", "total_ms",
                                              "t1_cm_ms", "t1_coder_ms")] + \
               [("dwt_launches", ctypes.c_uint32), ("t1_blocks", ctypes.c_uint32)] + \
               [(n, ctypes.c_uint64) for n in ("dwt_bytes", "cs_bytes", "t1_bytes", "t1_steps_max", "t1_steps_total",
                                               "t1_symbols", "t1_solo_blocks", "t1_solo_decisions",
                                               "t1_solo_decisions_max", "t1_shared")] + \
               [("roi_ms", ctypes.c_float)]


class ColourInfo(ctypes.Structure):
    """gk_colour_info (include/grok_amd.h): colour description of a JP2 file / codestream."""
    _fields_ = [(n, ctypes.c_uint32) for n in ("colour_space", "enumcs", "meth", "icc_len", "has_palette",
                                               "palette_entries", "palette_columns", "has_cdef", "num_comps",
                                               "num_channels")] + \
               [("typ", ctypes.c_uint16 * GK_MAX_CHANNELS), ("asoc", ctypes.c_uint16 * GK_MAX_CHANNELS),
                ("display_applied", ctypes.c_uint32)]

    def channels(self):
        """[(typ, asoc)] per output channel (cdef Typ / Asoc, or Grok's defaults)."""
        return [(self.typ[k], self.asoc[k]) for k in range(min(self.num_channels, GK_MAX_CHANNELS))]


_lib = None


class CmapEntry(ctypes.Structure):
    """gk_cmap_entry"""
    _fields_ = [("component", ctypes.c_uint16), ("mapping_type", ctypes.c_uint8), ("palette_column", ctypes.c_uint8)]


class EncodeColour(ctypes.Structure):
    """gk_encode_colour"""
    _fields_ = [("colour_space", ctypes.c_uint32), ("icc", ctypes.c_void_p), ("icc_len", ctypes.c_uint32),
                ("num_channels", ctypes.c_uint32), ("typ", ctypes.POINTER(ctypes.c_uint16)),
                ("asoc", ctypes.POINTER(ctypes.c_uint16)), ("palette_entries", ctypes.c_uint32),
                ("palette_columns", ctypes.c_uint32), ("channel_prec", ctypes.POINTER(ctypes.c_uint8)),
                ("lut", ctypes.POINTER(ctypes.c_int32)), ("cmap", ctypes.POINTER(CmapEntry))]


class EncodeConvert(ctypes.Structure):
    """gk_encode_convert"""
    _fields_ = [("space", ctypes.c_uint32), ("chroma_dx", ctypes.c_uint32), ("chroma_dy", ctypes.c_uint32)]


class Rect(ctypes.Structure):
    """gk_rect: half-open, in samples from the image's top-left sample"""
    _fields_ = [(n, ctypes.c_uint32) for n in ("x0", "y0", "x1", "y1")]


class EncodeRoi(ctypes.Structure):
    """gk_encode_roi"""
    _fields_ = [("shift", ctypes.c_uint32), ("num_comps", ctypes.c_uint32), ("comps", ctypes.POINTER(ctypes.c_uint32)),
                ("num_rects", ctypes.c_uint32), ("rects", ctypes.POINTER(Rect)), ("mask", ctypes.c_void_p),
                ("mask_w", ctypes.c_uint32), ("mask_h", ctypes.c_uint32), ("mask_row_bytes", ctypes.c_size_t),
                ("mask_on_device", ctypes.c_int)]


def _encode_roi(rects, mask, shift, components):
    """gk_encode_roi of the Python arguments: rects [(x0, y0, x1, y1)] half-open in image samples, mask
    an (H, W) array of 8-bit elements (numpy, or a torch cuda tensor: non-zero = region), shift 0..31
    (0: the smallest legal shift), components a list of indices (None: all).  None when there is
    neither a rectangle nor a mask."""
    if not rects and mask is None:
        return None
    if not 0 <= int(shift) < 1 << 32:
        raise ValueError("roi: shift is an unsigned 32-bit value")
    r = EncodeRoi()
    r.shift = int(shift)
    keep = []
    if components is not None and len(components):
        if any(not 0 <= int(c) < 1 << 32 for c in components):
            raise ValueError("roi: component indices are unsigned 32-bit values")
        ca = (ctypes.c_uint32 * len(components))(*[int(c) for c in components])
        keep.append(ca)
        r.num_comps, r.comps = len(components), ca
    if rects:
        for q in rects:
            if len(q) != 4 or any(not 0 <= int(v) < 1 << 32 for v in q):
                raise ValueError("roi: a rectangle is (x0, y0, x1, y1), unsigned 32-bit values")
        ra = (Rect * len(rects))(*[Rect(*[int(v) for v in q]) for q in rects])
        keep.append(ra)
        r.num_rects, r.rects = len(rects), ra
    if mask is not None:
        if _is_torch_cuda(mask):
            if mask.dim() != 2 or mask.element_size() != 1 or (mask.shape[1] > 1 and mask.stride(1) != 1):
                raise ValueError("roi: the mask is an (H, W) tensor of 8-bit elements with unit column stride")
            r.mask, r.mask_on_device = mask.data_ptr(), 1
            r.mask_h, r.mask_w = int(mask.shape[0]), int(mask.shape[1])
            r.mask_row_bytes = int(mask.stride(0)) if mask.shape[0] > 1 else r.mask_w
        else:
            m = np.asarray(mask)
            if m.ndim != 2:
                raise ValueError("roi: the mask is an (H, W) array")
            m = np.ascontiguousarray(m != 0, dtype=np.uint8)
            r.mask, r.mask_on_device = m.ctypes.data, 0
            r.mask_h, r.mask_w = m.shape
            r.mask_row_bytes = m.shape[1]
            mask = m
        keep.append(mask)
    r._keep = keep
    return r


def probe_encode_roi(shape, prec, params=None, rects=None, mask=None, shift=0, components=None, signed=False,
                     origin=None):
    """gk_probe_encode_roi: what an encode of a (C, H, W) image of `prec` bits under `params` and
    Engine.set_encode_roi(rects, mask, shift, components) would answer, no engine or GPU needed: the
    shift of each component (0: it does not carry the region).  A refusal raises ValueError with
    the engine's message."""
    lib = load_library()
    c, h, w = shape
    info = ImageInfo(w, h, c, prec, int(signed), 0)
    if params is None:
        params = default_params()
    if origin is not None:
        info.x0, info.y0 = int(origin[0]), int(origin[1])
    else:   # as Engine.encode: without an origin the image sits at the tile grid's
        info.x0, info.y0 = params.tx0, params.ty0
    r = _encode_roi(rects, mask, shift, components)
    if r is None:
        raise ValueError("gk_probe_encode_roi: roi: empty region (no rectangle and no non-zero mask byte)")
    out = (ctypes.c_uint32 * max(c, 1))()
    msg = ctypes.create_string_buffer(512)
    if lib.gk_probe_encode_roi(ctypes.byref(info), ctypes.byref(params), ctypes.byref(r), out, msg, len(msg)) != 0:
        raise ValueError("gk_probe_encode_roi: " + msg.value.decode())
    return [out[k] for k in range(c)]


class EncodeQuant(ctypes.Structure):
    """gk_encode_quant"""
    _fields_ = [("mode", ctypes.c_uint32), ("value", ctypes.c_double)]


class QuantResult(ctypes.Structure):
    """gk_quant_result"""
    _fields_ = [("mode", ctypes.c_uint32), ("notch", ctypes.c_uint32), ("t1_passes", ctypes.c_uint32),
                ("stats_passes", ctypes.c_uint32), ("base_step", ctypes.c_double), ("est_mse", ctypes.c_double),
                ("est_psnr", ctypes.c_double), ("est_psnr_next", ctypes.c_double), ("bytes", ctypes.c_uint64)]


def _encode_quant(step=None, max_bytes=None, psnr=None):
    """gk_encode_quant of the Python arguments: exactly one of step (base step, nominal-range units),
    max_bytes and psnr (dB); None when all are None."""
    given = [(m, v) for m, v in ((GK_QUANT_STEP, step), (GK_QUANT_BYTES, max_bytes), (GK_QUANT_PSNR, psnr)) if v is not None]
    if not given:
        return None
    if len(given) > 1:
        raise ValueError("quant: give exactly one of step, max_bytes and psnr")
    return EncodeQuant(given[0][0], float(given[0][1]))


def probe_encode_quant(shape, prec, params=None, step=None, max_bytes=None, psnr=None, signed=False, call="encode"):
    """gk_probe_encode_quant: what an encode of a (C, H, W) image of `prec` bits under `params` and
    Engine.set_encode_quant(step, max_bytes, psnr) would answer, no engine or GPU needed: the
    ladder's (step_min, step_max, notches).  call: "encode" (Engine.encode / encode_pixels),
    "encode_tiles" or "encode_blocks".  A refusal raises ValueError with the engine's message."""
    lib = load_library()
    c, h, w = shape
    info = ImageInfo(w, h, c, prec, int(signed), 0)
    if params is None:
        params = default_params()
    info.x0, info.y0 = params.tx0, params.ty0
    flags = {"encode": 0, "encode_tiles": GK_QUANT_FOR_TILES, "encode_blocks": GK_QUANT_FOR_BLOCKS}
    if call not in flags:
        raise ValueError("quant: call is 'encode', 'encode_tiles' or 'encode_blocks'")
    q = _encode_quant(step, max_bytes, psnr)
    if q is not None:
        q.mode |= flags[call]
    lo, hi, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_uint32()
    msg = ctypes.create_string_buffer(512)
    if lib.gk_probe_encode_quant(ctypes.byref(info), ctypes.byref(params), ctypes.byref(q) if q is not None else None,
                                 ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(n), msg, len(msg)) != 0:
        raise ValueError("gk_probe_encode_quant: " + msg.value.decode())
    return lo.value, hi.value, n.value


# GRK_COLOR_SPACE by name (gk_encode_colour::colour_space)
COLOUR_SPACES = {"srgb": 2, "grey": 3, "gray": 3, "sycc": 4, "esycc": 5, "eycc": 5, "cmyk": 6, "cie": 7, "icc": 9}


def _encode_colour(space=None, icc=None, channels=None, palette=None):
    """gk_encode_colour of the Python arguments (set_encode_colour / jp2_boxes), or None when all are
    None.  space: a GRK_COLOR_SPACE value or a name of COLOUR_SPACES (default: "icc" with a profile);
    channels: [(typ, asoc)] per component; palette: (lut (NE, NPC), column precisions,
    [(component, mapping type, palette column)])."""
    if space is None and icc is None and channels is None and palette is None:
        return None
    e = EncodeColour()
    if space is None:
        space = "icc" if icc is not None else 0
    if isinstance(space, str):
        if space.lower() not in COLOUR_SPACES:
            raise ValueError("colour_space: unknown colour space name %r" % space)
        space = COLOUR_SPACES[space.lower()]
    e.colour_space = int(space)
    keep = []
    if icc is not None:
        b = (ctypes.c_uint8 * max(len(icc), 1)).from_buffer_copy(bytes(icc) or b"\0")
        keep.append(b)
        e.icc, e.icc_len = ctypes.cast(b, ctypes.c_void_p), len(icc)
    if channels is not None:
        n = len(channels)
        t = (ctypes.c_uint16 * max(n, 1))(*[int(c[0]) for c in channels])
        a = (ctypes.c_uint16 * max(n, 1))(*[int(c[1]) for c in channels])
        keep += [t, a]
        e.num_channels, e.typ, e.asoc = n, t, a
    if palette is not None:
        lut, precs, cm = palette
        lut = np.asarray(lut)
        if lut.ndim != 2 or lut.shape[1] != len(precs) or len(cm) != len(precs):
            raise ValueError("pclr / cmap: the LUT is (NE, NPC), with NPC column precisions and NPC cmap entries")
        if lut.size and (lut.min() < -(1 << 31) or lut.max() >= (1 << 31)):
            raise ValueError("pclr box: a LUT value does not fit 32 bits")
        if any(not 0 <= int(p) <= 255 for p in precs) or any(not (0 <= c <= 65535 and 0 <= m <= 255 and 0 <= k <= 255) for c, m, k in cm):
            raise ValueError("pclr / cmap: column precisions, MTYP and PCOL are bytes, CMP 16 bits")
        l32 = np.ascontiguousarray(lut, dtype=np.int32)
        pr = (ctypes.c_uint8 * max(len(precs), 1))(*[int(x) for x in precs])
        ce = (CmapEntry * max(len(cm), 1))(*[CmapEntry(int(c), int(m), int(k)) for c, m, k in cm])
        keep += [l32, pr, ce]
        e.palette_entries, e.palette_columns = lut.shape
        e.channel_prec, e.lut, e.cmap = pr, l32.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ce
    e._keep = keep
    return e


def _encode_convert(space, chroma):
    """gk_encode_convert of the Python arguments: space a GRK_COLOR_SPACE value or a name of
    COLOUR_SPACES ("sycc", "esycc"), chroma = (dx, dy)."""
    if isinstance(space, str):
        if space.lower() not in COLOUR_SPACES:
            raise ValueError("convert: unknown colour space name %r" % space)
        space = COLOUR_SPACES[space.lower()]
    dx, dy = chroma
    if not (0 <= int(space) < 1 << 32 and 0 <= int(dx) < 1 << 32 and 0 <= int(dy) < 1 << 32):
        raise ValueError("convert: colour space and chroma factors are unsigned 32-bit values")
    return EncodeConvert(int(space), int(dx), int(dy))


def probe_encode_convert(shape, prec, space, chroma=(1, 1), origin=None, signed=False, sample_bytes=0):
    """gk_probe_encode_convert: what an encode of an (H, W, C) image of `prec` bits codes under
    Engine.set_encode_convert(space, chroma), no engine or GPU needed: [(dx, dy)] and [(rows, cols)]
    per component.  A refusal raises ValueError with the engine's message."""
    lib = load_library()
    h, w, c = shape
    info = ImageInfo(w, h, c, prec, int(signed), sample_bytes)
    if origin is not None:
        info.x0, info.y0 = int(origin[0]), int(origin[1])
    spec = _encode_convert(space, chroma)
    dx, dy, cw, ch = [(ctypes.c_uint32 * 3)() for _ in range(4)]
    msg = ctypes.create_string_buffer(512)
    if lib.gk_probe_encode_convert(ctypes.byref(info), ctypes.byref(spec), dx, dy, cw, ch, msg, len(msg)) != 0:
        raise ValueError("gk_probe_encode_convert: " + msg.value.decode())
    return [(dx[k], dy[k]) for k in range(3)], [(ch[k], cw[k]) for k in range(3)]


def jp2_boxes(shape, prec, cs_len, signed=False, space=None, icc=None, channels=None, palette=None):
    """gk_jp2_boxes: the JP2 boxes in front of a codestream of cs_len bytes for an image of
    shape = (C, H, W), no device needed; file = these bytes + the codestream.  The colour
    arguments are Engine.set_encode_colour's; without them ihdr and the default colr
    (Engine.jp2_header's bytes).  A refusal raises ValueError with the engine's message."""
    lib = load_library()
    c, h, w = shape
    info = ImageInfo(w, h, c, prec, int(signed), 0)
    e = _encode_colour(space, icc, channels, palette)
    msg = ctypes.create_string_buffer(512)
    n = ctypes.c_size_t()
    buf = np.empty(4096, np.uint8)
    for _ in range(2):
        rc = lib.gk_jp2_boxes(ctypes.byref(info), ctypes.byref(e) if e is not None else None, cs_len, buf.ctypes.data, buf.size,
                              ctypes.byref(n), msg, len(msg))
        if rc != -2:
            break
        buf = np.empty(n.value, np.uint8)
    if rc != 0:
        raise ValueError("gk_jp2_boxes: " + msg.value.decode())
    return buf[:n.value].tobytes()


def load_library(build_if_missing=True):
    """Load the in-tree HIP extension (built by grok_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        if not build_if_missing:
            raise RuntimeError("libgrok_amd.so is missing: run __graft_entry__.build()")
        from . import build as _b
        _b.build()
    lib = ctypes.CDLL(LIB_PATH)
    P = ctypes.POINTER
    lib.gk_create.restype = ctypes.c_void_p
    lib.gk_create.argtypes = [ctypes.c_int]
    lib.gk_destroy.argtypes = [ctypes.c_void_p]
    lib.gk_set_default_params.argtypes = [P(CParameters)]
    lib.gk_encode.restype = ctypes.c_int
    lib.gk_encode.argtypes = [ctypes.c_void_p, P(ImageInfo), P(ctypes.c_void_p), P(ctypes.c_uint32), ctypes.c_int,
                              P(CParameters), ctypes.c_void_p, ctypes.c_size_t, P(ctypes.c_size_t), ctypes.c_int]
    lib.gk_encode_tiles.restype = ctypes.c_int
    lib.gk_encode_tiles.argtypes = [ctypes.c_void_p, P(ImageInfo), P(ctypes.c_void_p), P(ctypes.c_uint32), ctypes.c_int,
                                    P(CParameters), ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t,
                                    P(ctypes.c_size_t), P(ctypes.c_uint32), ctypes.c_int]
    lib.gk_main_header.restype = ctypes.c_int
    lib.gk_main_header.argtypes = [ctypes.c_void_p, P(ImageInfo), P(CParameters), ctypes.c_void_p, ctypes.c_size_t,
                                   P(ctypes.c_size_t), P(ctypes.c_size_t), P(ctypes.c_uint32)]
    lib.gk_jp2_header.restype = ctypes.c_int
    lib.gk_jp2_header.argtypes = [ctypes.c_void_p, P(ImageInfo), ctypes.c_uint64, ctypes.c_void_p, ctypes.c_size_t,
                                  P(ctypes.c_size_t)]
    lib.gk_probe_header.restype = ctypes.c_int
    lib.gk_probe_header.argtypes = [ctypes.c_void_p, ctypes.c_size_t, P(ImageInfo), P(CParameters), ctypes.c_char_p,
                                    ctypes.c_size_t]
    lib.gk_decode_window.restype = ctypes.c_int
    lib.gk_decode_window.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int] + \
        [ctypes.c_uint32] * 4 + [P(ctypes.c_void_p), P(ctypes.c_uint32), ctypes.c_uint32, ctypes.c_int]
    lib.gk_decode_header.restype = ctypes.c_int
    lib.gk_decode_header.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, P(ImageInfo)]
    lib.gk_set_decode_reduce.restype = ctypes.c_int
    lib.gk_set_decode_reduce.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    lib.gk_set_window_rule.restype = ctypes.c_int
    lib.gk_set_window_rule.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.gk_set_subsampling.restype = ctypes.c_int
    lib.gk_set_subsampling.argtypes = [ctypes.c_void_p, ctypes.c_uint32, P(ctypes.c_uint32), P(ctypes.c_uint32)]
    lib.gk_probe_components.restype = ctypes.c_int
    lib.gk_probe_components.argtypes = [ctypes.c_void_p, ctypes.c_size_t] + [P(ctypes.c_uint32)] * 4 + [ctypes.c_uint32]
    lib.gk_header_components.restype = ctypes.c_int
    lib.gk_header_components.argtypes = [ctypes.c_void_p] + [P(ctypes.c_uint32)] * 4 + [ctypes.c_uint32]
    lib.gk_probe_colour.restype = ctypes.c_int
    lib.gk_probe_colour.argtypes = [ctypes.c_void_p, ctypes.c_size_t, P(ColourInfo), ctypes.c_char_p, ctypes.c_size_t]
    lib.gk_probe_icc.restype = ctypes.c_int
    lib.gk_probe_icc.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, P(ctypes.c_size_t)]
    lib.gk_probe_stream_components.restype = ctypes.c_int
    lib.gk_probe_stream_components.argtypes = [ctypes.c_void_p, ctypes.c_size_t] + [P(ctypes.c_uint32)] * 4 + \
        [ctypes.c_uint32]
    lib.gk_header_colour.restype = ctypes.c_int
    lib.gk_header_colour.argtypes = [ctypes.c_void_p, P(ColourInfo)]
    lib.gk_header_icc.restype = ctypes.c_int
    lib.gk_header_icc.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, P(ctypes.c_size_t)]
    lib.gk_header_cielab.restype = ctypes.c_int
    lib.gk_header_cielab.argtypes = [ctypes.c_void_p, P(ctypes.c_uint32), P(ctypes.c_uint32)]
    lib.gk_probe_cielab.restype = ctypes.c_int
    lib.gk_probe_cielab.argtypes = [ctypes.c_void_p, ctypes.c_size_t, P(ctypes.c_uint32), P(ctypes.c_uint32)]
    lib.gk_set_decode_colour.restype = ctypes.c_int
    lib.gk_set_decode_colour.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.gk_set_decode_display.restype = ctypes.c_int
    lib.gk_set_decode_display.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    lib.gk_probe_display.restype = ctypes.c_int
    lib.gk_probe_display.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, P(ImageInfo),
                                     P(ColourInfo)] + [P(ctypes.c_uint32)] * 4 + [ctypes.c_uint32, ctypes.c_char_p,
                                                                                  ctypes.c_size_t]
    lib.gk_set_decode_precision.restype = ctypes.c_int
    lib.gk_set_decode_precision.argtypes = [ctypes.c_void_p, P(Precision), ctypes.c_uint32]
    lib.gk_probe_output.restype = ctypes.c_int
    lib.gk_probe_output.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, P(Precision),
                                    ctypes.c_uint32, P(ImageInfo), P(ColourInfo)] + [P(ctypes.c_uint32)] * 4 + \
        [ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t]
    lib.gk_decode_pixels.restype = ctypes.c_int
    lib.gk_decode_pixels.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p,
                                     ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int]
    lib.gk_decode_window_pixels.restype = ctypes.c_int
    lib.gk_decode_window_pixels.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int] + \
        [ctypes.c_uint32] * 4 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int]
    lib.gk_encode_pixels.restype = ctypes.c_int
    lib.gk_encode_pixels.argtypes = [ctypes.c_void_p, P(ImageInfo), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                     P(CParameters), ctypes.c_void_p, ctypes.c_size_t, P(ctypes.c_size_t), ctypes.c_int]
    lib.gk_set_encode_colour.restype = ctypes.c_int
    lib.gk_set_encode_colour.argtypes = [ctypes.c_void_p, P(EncodeColour)]
    lib.gk_jp2_boxes.restype = ctypes.c_int
    lib.gk_jp2_boxes.argtypes = [P(ImageInfo), P(EncodeColour), ctypes.c_uint64, ctypes.c_void_p, ctypes.c_size_t,
                                 P(ctypes.c_size_t), ctypes.c_char_p, ctypes.c_size_t]
    lib.gk_set_encode_convert.restype = ctypes.c_int
    lib.gk_set_encode_convert.argtypes = [ctypes.c_void_p, P(EncodeConvert)]
    lib.gk_probe_encode_convert.restype = ctypes.c_int
    lib.gk_probe_encode_convert.argtypes = [P(ImageInfo), P(EncodeConvert)] + [P(ctypes.c_uint32)] * 4 + \
        [ctypes.c_char_p, ctypes.c_size_t]
    lib.gk_set_encode_roi.restype = ctypes.c_int
    lib.gk_set_encode_roi.argtypes = [ctypes.c_void_p, P(EncodeRoi)]
    lib.gk_probe_encode_roi.restype = ctypes.c_int
    lib.gk_probe_encode_roi.argtypes = [P(ImageInfo), P(CParameters), P(EncodeRoi), P(ctypes.c_uint32), ctypes.c_char_p,
                                        ctypes.c_size_t]
    # (another build named by GROK_AMD_LIB, the A side of a measurement, may predate these three: its
    # plain calls still run and set_encode_quant fails on the missing symbol; the tree's own must have them)
    if hasattr(lib, "gk_set_encode_quant") or not os.environ.get("GROK_AMD_LIB"):
        lib.gk_set_encode_quant.restype = ctypes.c_int
        lib.gk_set_encode_quant.argtypes = [ctypes.c_void_p, P(EncodeQuant)]
        lib.gk_probe_encode_quant.restype = ctypes.c_int
        lib.gk_probe_encode_quant.argtypes = [P(ImageInfo), P(CParameters), P(EncodeQuant), P(ctypes.c_double),
                                              P(ctypes.c_double), P(ctypes.c_uint32), ctypes.c_char_p, ctypes.c_size_t]
        lib.gk_get_encode_quant.restype = ctypes.c_int
        lib.gk_get_encode_quant.argtypes = [ctypes.c_void_p, P(QuantResult)]
    lib.gk_roi_band_mask.restype = ctypes.c_int
    lib.gk_roi_band_mask.argtypes = [ctypes.c_void_p, P(ImageInfo), P(CParameters)] + [ctypes.c_uint32] * 4 + \
        [ctypes.c_void_p, ctypes.c_size_t, P(ctypes.c_uint32), P(ctypes.c_uint32), ctypes.c_int]
    lib.gk_set_default_transcode.argtypes = [P(TranscodeParams)]
    lib.gk_transcode.restype = ctypes.c_int
    lib.gk_transcode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, P(TranscodeParams),
                                 ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, P(ctypes.c_size_t)]
    lib.gk_probe_transcode.restype = ctypes.c_int
    lib.gk_probe_transcode.argtypes = [ctypes.c_void_p, ctypes.c_size_t, P(TranscodeParams), ctypes.c_char_p,
                                       ctypes.c_size_t]
    if hasattr(lib, "gk_probe_view") or not os.environ.get("GROK_AMD_LIB"):   # (as above: an older A side)
        lib.gk_probe_view.restype = ctypes.c_int
        lib.gk_probe_view.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, P(Precision), ctypes.c_uint32,
                                      P(View), P(ViewResult), ctypes.c_char_p, ctypes.c_size_t]
        lib.gk_decode_view_pixels.restype = ctypes.c_int
        lib.gk_decode_view_pixels.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, P(View),
                                              ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int, P(ViewResult)]
    if hasattr(lib, "gk_set_decode_render") or not os.environ.get("GROK_AMD_LIB"):   # (as above: an older A side)
        lib.gk_set_decode_render.restype = ctypes.c_int
        lib.gk_set_decode_render.argtypes = [ctypes.c_void_p, P(Render)]
        lib.gk_probe_render.restype = ctypes.c_int
        lib.gk_probe_render.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, P(Precision), ctypes.c_uint32,
                                        P(Render), P(RenderResult), ctypes.c_char_p, ctypes.c_size_t]
        lib.gk_decode_levels.restype = ctypes.c_int
        lib.gk_decode_levels.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, P(View),
                                         P(LevelsBins), ctypes.c_uint32, ctypes.c_uint32, P(ChannelLevels),
                                         ctypes.c_void_p, ctypes.c_size_t, P(ViewResult)]
    if hasattr(lib, "gk_probe_tensor") or not os.environ.get("GROK_AMD_LIB"):   # (as above: an older A side)
        lib.gk_probe_tensor.restype = ctypes.c_int
        lib.gk_probe_tensor.argtypes = [P(ViewResult), P(Tensor), P(ctypes.c_uint64), ctypes.c_char_p, ctypes.c_size_t]
        lib.gk_decode_view_tensor.restype = ctypes.c_int
        lib.gk_decode_view_tensor.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, P(View),
                                              P(Tensor), P(ViewResult)]
    lib.gk_set_decode_layers.restype = ctypes.c_int
    lib.gk_set_decode_layers.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    lib.gk_decode.restype = ctypes.c_int
    lib.gk_decode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, P(ctypes.c_void_p),
                              P(ctypes.c_uint32), ctypes.c_uint32, ctypes.c_int]
    lib.gk_get_timings.restype = ctypes.c_int
    lib.gk_get_timings.argtypes = [ctypes.c_void_p, P(Timings)]
    lib.gk_last_error.restype = ctypes.c_char_p
    lib.gk_last_error.argtypes = [ctypes.c_void_p]
    lib.gk_version.restype = ctypes.c_char_p
    _lib = lib
    return lib


PROG_ORDERS = ["LRCP", "RLCP", "RPCL", "PCRL", "CPRL"]   # GRK_PROG_ORDER (grok.h)


def default_params(numresolution=6, cblk=(64, 64), irreversible=False, mct=True, numlayers=1, layer_rate=None,
                   precincts=None, write_comment=True, cblk_sty=0, tiles=None, tlm=False, plt=False, jp2=False,
                   prog_order="LRCP", tile_parts=None, pocs=None, roi=None, sop=False, eph=False, quality=None,
                   tile_origin=None, comments=None):
    """grk_compress_set_default_params + the CLI options used by the benchmark configs.

    prog_order: "LRCP", "RLCP", "RPCL", "PCRL", "CPRL" or 0..4 (grk_compress -p).
    cblk_sty=0x40 selects the HTJ2K block coder; like grk_compress -M 64
    (grk_compress.cpp:1120-1125) it also sets one guard bit."""
    lib = load_library()
    p = CParameters()
    lib.gk_set_default_params(ctypes.byref(p))
    p.numresolution = numresolution
    if tile_origin:   # grk_compress -T: the tile grid's canvas origin (the image origin is Engine.encode's `origin`)
        p.tx0, p.ty0 = int(tile_origin[0]), int(tile_origin[1])
    p.cblockw_init, p.cblockh_init = cblk
    p.irreversible = int(irreversible)
    p.mct = int(mct)
    p.numlayers = len(layer_rate) if layer_rate else numlayers
    if layer_rate:
        for i, r in enumerate(layer_rate):
            p.layer_rate[i] = r
    if precincts:
        p.csty |= 1
        p.res_spec = len(precincts)
        for i, (w, h) in enumerate(precincts):
            p.prcw_init[i], p.prch_init[i] = w, h
    p.write_comment = int(write_comment)
    p.cblk_sty = int(cblk_sty)
    if cblk_sty & 0x40:
        p.numgbits = 1
    if tiles:   # grk_compress -t W,H
        p.tile_size_on = 1
        p.t_width, p.t_height = int(tiles[0]), int(tiles[1])
    p.writeTLM, p.writePLT = int(bool(tlm)), int(bool(plt))
    p.cod_format = 2 if jp2 else 0   # GRK_CODEC_JP2 / GRK_CODEC_J2K
    p.prog_order = PROG_ORDERS.index(prog_order) if isinstance(prog_order, str) else int(prog_order)
    p.roi_compno, p.roi_shift = (int(roi[0]), int(roi[1])) if roi else (-1, 0)   # grk_compress -ROI c=..,U=..
    if pocs:   # [(resS, compS, layE, resE, compE, "PROG"), ...] (grk_compress -P)
        p.numpocs = len(pocs)
        for i, (rs, cs, le, re_, ce, pr) in enumerate(pocs):
            p.pocs[i] = Poc(rs, cs, le, re_, ce, PROG_ORDERS.index(pr) if isinstance(pr, str) else int(pr))
    if tile_parts:   # grk_compress -u L|R|C: a new tile part whenever that index changes
        p.enableTilePartGeneration = 1
        p.newTilePartProgressionDivider = tile_parts.encode()
    p.csty |= (2 if sop else 0) | (4 if eph else 0)   # grk_compress -S / -E
    if comments:   # grk_compress -C: [bytes or str, ...] (bytes = binary, Rcom 0); the buffers stay with p
        p._comment_bufs = [c if isinstance(c, bytes) else c.encode() for c in comments]
        p.num_comments = len(comments)
        for i, c in enumerate(comments):
            p.comment[i] = p._comment_bufs[i]
            p.comment_len[i] = len(p._comment_bufs[i])
            p.is_binary_comment[i] = 1 if isinstance(c, bytes) else 0
    if quality:   # grk_compress -q PSNR,PSNR,...: fixed-quality layers
        p.allocationByQuality = 1
        p.numlayers = len(quality)
        for i, q in enumerate(quality):
            p.layer_distortion[i] = q
    return p


def probe_header(cs):
    """gk_probe_header: image info of host codestream / JP2 bytes, no engine or GPU needed."""
    lib = load_library()
    b = np.frombuffer(bytes(cs), np.uint8)
    info = ImageInfo()
    msg = ctypes.create_string_buffer(256)
    if lib.gk_probe_header(b.ctypes.data, len(b), ctypes.byref(info), None, msg, 256) != 0:
        raise ValueError(msg.value.decode())
    return info


def probe_transcode(cs, target="ht", tlm=False, plt=False, com=True):
    """gk_probe_transcode: whether host codestream / JP2 bytes would transcode to `target` ("ht" |
    "part1"); no engine or GPU needed (headers and packet headers are parsed on the host).  Returns
    None, or raises ValueError with the refusal Engine.transcode would give."""
    lib = load_library()
    b = np.frombuffer(bytes(cs), np.uint8)
    tp = _transcode_params(target, tlm, plt, com)
    msg = ctypes.create_string_buffer(512)
    if lib.gk_probe_transcode(b.ctypes.data, len(b), ctypes.byref(tp), msg, 512) != 0:
        raise ValueError(msg.value.decode())


def probe_colour(cs):
    """gk_probe_colour: ColourInfo of host codestream / JP2 bytes (colour space, ICC length, palette,
    output channels with their cdef types), no engine or GPU needed.  Malformed colour boxes raise
    ValueError with a message naming the box."""
    lib = load_library()
    b = np.frombuffer(bytes(cs), np.uint8)
    info = ColourInfo()
    msg = ctypes.create_string_buffer(512)
    if lib.gk_probe_colour(b.ctypes.data, len(b), ctypes.byref(info), msg, 512) != 0:
        raise ValueError(msg.value.decode())
    return info


def probe_icc(cs):
    """gk_probe_icc: the ICC profile bytes (colr METH 2) of host JP2 bytes, b"" without one."""
    lib = load_library()
    b = np.frombuffer(bytes(cs), np.uint8)
    n = ctypes.c_size_t()
    if lib.gk_probe_icc(b.ctypes.data, len(b), None, 0, ctypes.byref(n)) == -1:
        probe_colour(cs)   # (raises with the reason)
    buf = np.empty(max(n.value, 1), np.uint8)
    if n.value and lib.gk_probe_icc(b.ctypes.data, len(b), buf.ctypes.data, buf.size, ctypes.byref(n)) != 0:
        raise ValueError("gk_probe_icc failed")
    return buf[:n.value].tobytes()


def probe_cielab(cs):
    """gk_probe_cielab: the CIELab words of host JP2 bytes (colr EnumCS 14) as Grok keeps them: [14,
    default / custom tag] or [14, 0, rl, ol, ra, oa, rb, ob, il]; [] for any other file."""
    lib = load_library()
    b = np.frombuffer(bytes(cs), np.uint8)
    words, n = (ctypes.c_uint32 * 9)(), ctypes.c_uint32()
    if lib.gk_probe_cielab(b.ctypes.data, len(b), words, ctypes.byref(n)) != 0:
        probe_colour(cs)   # (raises with the reason)
        raise ValueError("gk_probe_cielab failed")
    return [int(words[i]) for i in range(n.value)]


class DisplayInfo:
    """What probe_display reports: the output of a decode under the display flags."""

    def __init__(self, info, colour, chans, reduce):
        self.info, self.colour = info, colour
        self.channels = [(dx, dy) for dx, dy, _, _ in chans]          # (dx, dy) per output channel
        self.precisions = [pr for _, _, pr, _ in chans]
        self.signed = [bool(sg) for _, _, _, sg in chans]
        self.shapes = [comp_shape(info.w, info.h, dx, dy, (info.x0, info.y0), reduce) for dx, dy, _, _ in chans]
        self.colour_space = colour.colour_space
        self.converted = bool(colour.display_applied & GK_DISPLAY_RGB)
        self.upsampled = bool(colour.display_applied & GK_DISPLAY_UPSAMPLE)
        self.replicated = bool(colour.display_applied & GK_DISPLAY_FORCE_RGB)   # grey to RGB
        self.managed = bool(colour.display_applied & GK_DISPLAY_ICC)   # ICC profile / CIELab to sRGB


def probe_display(cs, rgb=False, upsample=False, reduce=0, icc=False):
    """gk_probe_display: what a decode of host codestream / JP2 bytes returns under
    Engine.set_decode_display(rgb, upsample, icc=icc) and set_decode_reduce(reduce), no engine or GPU
    needed: a DisplayInfo with the channel shapes (rows, cols), precisions, signs, colour space
    (GRK_COLOR_SPACE) and the converted / upsampled flags.  Raises ValueError with the refusal."""
    lib = load_library()
    b = np.frombuffer(bytes(cs), np.uint8)
    info, colour = ImageInfo(), ColourInfo()
    dx, dy, pr, sg = [(ctypes.c_uint32 * 16384)() for _ in range(4)]
    msg = ctypes.create_string_buffer(512)
    flags = (GK_DISPLAY_RGB if rgb else 0) | (GK_DISPLAY_UPSAMPLE if upsample else 0) | (GK_DISPLAY_ICC if icc else 0)
    n = lib.gk_probe_display(b.ctypes.data, len(b), flags, int(reduce), ctypes.byref(info), ctypes.byref(colour),
                             dx, dy, pr, sg, 16384, msg, 512)
    if n < 0:
        raise ValueError(msg.value.decode())
    return DisplayInfo(info, colour, [(dx[c], dy[c], pr[c], sg[c]) for c in range(n)], int(reduce))


def probe_output(cs, rgb=False, upsample=False, force_rgb=False, precision=None, reduce=0, icc=False):
    """gk_probe_output: probe_display with the grey-to-RGB flag and a forced-precision list
    (parse_precision): what Engine.decode / decode_pixels return under set_decode_display(rgb,
    upsample, force_rgb, icc) and set_decode_precision(precision), no engine or GPU needed."""
    lib = load_library()
    b = np.frombuffer(bytes(cs), np.uint8)
    info, colour = ImageInfo(), ColourInfo()
    dx, dy, pr, sg = [(ctypes.c_uint32 * 16384)() for _ in range(4)]
    msg = ctypes.create_string_buffer(512)
    flags = (GK_DISPLAY_RGB if rgb else 0) | (GK_DISPLAY_UPSAMPLE if upsample else 0) | \
        (GK_DISPLAY_FORCE_RGB if force_rgb else 0) | (GK_DISPLAY_ICC if icc else 0)
    arr, n = _precision_array(precision)
    n = lib.gk_probe_output(b.ctypes.data, len(b), flags, int(reduce), arr, n, ctypes.byref(info), ctypes.byref(colour),
                            dx, dy, pr, sg, 16384, msg, 512)
    if n < 0:
        raise ValueError(msg.value.decode())
    return DisplayInfo(info, colour, [(dx[c], dy[c], pr[c], sg[c]) for c in range(n)], int(reduce))


def probe_view(cs, region=None, size=None, width=None, height=None, fit=False, rotate=0, mirror=False, rgb=False,
               upsample=False, force_rgb=False, icc=False, precision=None):
    """gk_probe_view: what Engine.decode_view would resolve for host codestream / JP2 bytes under
    set_decode_display(rgb, upsample, force_rgb, icc) and set_decode_precision(precision), no engine
    or GPU needed: a ViewResult (reduce, the region on the reduced canvas, out_w x out_h, the written
    pix_w x pix_h, channels, prec, sgnd).  Raises ValueError with the engine's refusal."""
    lib = load_library()
    b = np.frombuffer(bytes(cs), np.uint8)
    flags = (GK_DISPLAY_RGB if rgb else 0) | (GK_DISPLAY_UPSAMPLE if upsample else 0) | \
        (GK_DISPLAY_FORCE_RGB if force_rgb else 0) | (GK_DISPLAY_ICC if icc else 0)
    arr, n = _precision_array(precision)
    v, res = _view(region, size, width, height, fit, rotate, mirror), ViewResult()
    msg = ctypes.create_string_buffer(512)
    if lib.gk_probe_view(b.ctypes.data, len(b), flags, arr, n, ctypes.byref(v), ctypes.byref(res), msg, 512) != 0:
        raise ValueError(msg.value.decode())
    return res


def probe_render(cs, mode=None, windows=None, tints=None, curve=None, map=None, gamma=None, rgb=False, upsample=False,
                 force_rgb=False, icc=False, precision=None):
    """gk_probe_render: what the pixel calls return for host codestream / JP2 bytes under
    set_decode_display(rgb, upsample, force_rgb, icc), set_decode_precision(precision) and
    set_decode_render(mode, windows, ...), no engine or GPU needed: a RenderResult (channels, prec,
    sgnd, colour_space).  Raises ValueError with the engine's refusal."""
    lib = load_library()
    b = np.frombuffer(bytes(cs), np.uint8)
    flags = (GK_DISPLAY_RGB if rgb else 0) | (GK_DISPLAY_UPSAMPLE if upsample else 0) | \
        (GK_DISPLAY_FORCE_RGB if force_rgb else 0) | (GK_DISPLAY_ICC if icc else 0)
    arr, n = _precision_array(precision)
    r, keep = _render(mode, windows, tints, curve, map, gamma)
    res = RenderResult()
    msg = ctypes.create_string_buffer(512)
    if lib.gk_probe_render(b.ctypes.data, len(b), flags, arr, n, ctypes.byref(r) if r is not None else None,
                           ctypes.byref(res), msg, 512) != 0:
        raise ValueError(msg.value.decode())
    del keep
    return res


def probe_components(cs, precision=False):
    """gk_probe_components: [(dx, dy)] per output channel of host codestream / JP2 bytes (SIZ XRsiz /
    YRsiz; the channels a JP2 palette / channel definition makes of the components); with
    precision=True [(dx, dy, prec, signed)]."""
    lib = load_library()
    b = np.frombuffer(bytes(cs), np.uint8)
    dx, dy, pr, sg = [(ctypes.c_uint32 * 16384)() for _ in range(4)]
    n = lib.gk_probe_components(b.ctypes.data, len(b), dx, dy, pr, sg, 16384)
    if n < 0:
        probe_header(cs)   # (raises with the reason)
        raise ValueError("gk_probe_components failed")
    if precision:
        return [(dx[c], dy[c], pr[c], bool(sg[c])) for c in range(n)]
    return [(dx[c], dy[c]) for c in range(n)]


def comp_shape(w, h, dx, dy, origin=(0, 0), reduce=0):
    """(rows, cols) of a component sampled every (dx, dy) canvas positions over the image area
    [x0, x0 + w) x [y0, y0 + h) (grk_image_comp h / w), reduced by `reduce` resolutions."""
    x0, y0 = origin
    cd = lambda a, b: -(-a // b)
    cx0, cy0, cx1, cy1 = cd(x0, dx), cd(y0, dy), cd(x0 + w, dx), cd(y0 + h, dy)
    r = 1 << reduce
    return cd(cy1, r) - cd(cy0, r), cd(cx1, r) - cd(cx0, r)


def _sample_bytes(x):
    """gk_image_info::sample_bytes of a plane array (numpy or torch): 0 for 32-bit, else its item size."""
    n = x.element_size() if hasattr(x, "element_size") else x.dtype.itemsize
    return 0 if n == 4 else n


def _host_planes(a, prec):
    """Host planes as passed when their 8/16-bit type fits the precision ((prec + 7) // 8 bytes,
    grk_compress_tile's raw buffer), int32 otherwise."""
    if a.dtype.kind in "ui" and a.dtype.itemsize in (1, 2) and a.dtype.itemsize == (prec + 7) // 8:
        return np.ascontiguousarray(a)
    return np.ascontiguousarray(a, dtype=np.int32)


def _np_sample_dtype(sample_bytes, info):
    if sample_bytes in (0, 4):
        return np.int32
    return {(1, 0): np.uint8, (1, 1): np.int8, (2, 0): np.uint16, (2, 1): np.int16}[(sample_bytes, int(info.sgnd))]


def _is_torch_cuda(x):
    return hasattr(x, "is_cuda") and x.is_cuda


class Engine:
    """One MI355X, one HIP stream (grk_codec analogue)."""

    def __init__(self, device=0):
        # PyTorch-ROCm bundles its own HIP/HSA runtime.  When both live in one
        # process, torch's must initialise first or it later reports "No HIP
        # GPUs"; device tensors are only exchanged with torch, so initialise it
        # here when it is present.  The C ABI itself does not depend on torch.
        if "torch" in sys.modules:
            try:
                sys.modules["torch"].cuda.init()
            except Exception:
                pass
        self.lib = load_library()
        self.ctx = self.lib.gk_create(device)
        if not self.ctx:
            raise RuntimeError("gk_create failed: no HIP device %d" % device)
        self._display_flags, self._precision = 0, None   # as set_decode_display / set_decode_precision left them

    def close(self):
        if self.ctx:
            self.lib.gk_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, what):
        raise RuntimeError("%s failed: %s" % (what, self.lib.gk_last_error(self.ctx).decode()))

    def timings(self):
        t = Timings()
        self.lib.gk_get_timings(self.ctx, ctypes.byref(t))
        return t

    # ------------------------------------------------------------------ encode
    def encode(self, planes, prec, signed=False, params=None, out=None, origin=None, subsampling=None, size=None):
        """planes: (C, H, W) int32 numpy array (host) or torch cuda tensor (device).
        Returns bytes (host) or, when ``out`` (a torch cuda uint8 tensor) is given,
        the codestream length written into it on the device.  origin: the image area's
        canvas origin (grk_image::x0 / y0, grk_compress -d); without it the image sits at
        the tile grid origin (-T alone moves the image there, grk_compress.cpp:1547-1551).
        subsampling=[(dx, dy), ...] (grk_image_comp::dx / dy): planes is then a list of 2-D
        planes of comp_shape(W, H, dx, dy, origin) each and size=(W, H) the image area."""
        if params is None:
            params = default_params()
        if subsampling:
            return self._encode_subsampled(planes, prec, signed, params, out, origin, subsampling, size)
        c, h, w = planes.shape
        on_dev = _is_torch_cuda(planes)
        if on_dev:
            assert planes.is_contiguous() and planes.element_size() in (1, 2, 4)
            base = planes.data_ptr()
        else:
            planes = _host_planes(planes, prec)
            base = planes.ctypes.data
        sb = _sample_bytes(planes)
        es = sb or 4
        info = ImageInfo(w, h, c, prec, int(signed), sb)
        if origin is not None:
            info.x0, info.y0 = int(origin[0]), int(origin[1])
        else:
            info.x0, info.y0 = params.tx0, params.ty0
        ptrs = (ctypes.c_void_p * c)(*[base + k * h * w * es for k in range(c)])
        strides = (ctypes.c_uint32 * c)(*([w] * c))
        n = ctypes.c_size_t()
        if out is not None:
            rc = self.lib.gk_encode(self.ctx, ctypes.byref(info), ptrs, strides, int(on_dev), ctypes.byref(params),
                                    ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.byref(n), 1)
            if rc != 0:
                self._err("gk_encode")
            return n.value
        cap = c * h * w * 4 + (1 << 20)
        buf = np.empty(cap, np.uint8)
        rc = self.lib.gk_encode(self.ctx, ctypes.byref(info), ptrs, strides, int(on_dev), ctypes.byref(params),
                                buf.ctypes.data, cap, ctypes.byref(n), 0)
        if rc == -2:
            buf = np.empty(n.value, np.uint8)
            rc = self.lib.gk_encode(self.ctx, ctypes.byref(info), ptrs, strides, int(on_dev), ctypes.byref(params),
                                    buf.ctypes.data, n.value, ctypes.byref(n), 0)
        if rc != 0:
            self._err("gk_encode")
        return buf[:n.value].tobytes()

    def transcode(self, cs, target="ht", out=None, tlm=False, plt=False, com=True, length=None):
        """gk_transcode: the codestream or JP2 file `cs` (bytes, or a torch cuda uint8 tensor with
        `length`) re-coded with the other block coder, target "ht" | "part1", coefficient for
        coefficient (no DWT, no second lossy generation).  Returns bytes, or with ``out`` (a torch
        cuda uint8 tensor) the length written into it on the device, as encode does.  A refusal
        (include/grok_amd.h lists them) raises RuntimeError with its message."""
        tp = _transcode_params(target, tlm, plt, com)
        on_dev = _is_torch_cuda(cs)
        if on_dev:
            assert cs.is_contiguous() and cs.element_size() == 1
            src, n_in = cs.data_ptr(), int(length if length is not None else cs.numel())
        else:
            keep = np.frombuffer(bytes(cs), np.uint8)
            src, n_in = keep.ctypes.data, len(keep)
        n = ctypes.c_size_t()
        if out is not None:
            rc = self.lib.gk_transcode(self.ctx, src, n_in, int(on_dev), ctypes.byref(tp), ctypes.c_void_p(out.data_ptr()),
                                       out.numel(), 1, ctypes.byref(n))
            if rc != 0:
                self._err("gk_transcode")
            return n.value
        cap = 2 * n_in + (1 << 16)
        buf = np.empty(cap, np.uint8)
        rc = self.lib.gk_transcode(self.ctx, src, n_in, int(on_dev), ctypes.byref(tp), buf.ctypes.data, cap, 0, ctypes.byref(n))
        if rc == -2:
            buf = np.empty(n.value, np.uint8)
            rc = self.lib.gk_transcode(self.ctx, src, n_in, int(on_dev), ctypes.byref(tp), buf.ctypes.data, n.value, 0,
                                       ctypes.byref(n))
        if rc != 0:
            self._err("gk_transcode")
        return buf[:n.value].tobytes()

    def set_encode_colour(self, space=None, icc=None, channels=None, palette=None):
        """gk_set_encode_colour (sticky): the colour description later JP2 encodes and jp2_header write
        (colr, cdef, pclr + cmap), as _encode_colour reads the arguments; no argument clears it.  sYCC
        and e-sYCC also clear the MCT of later encodes, raw codestreams included.  A refusal raises
        ValueError and leaves the engine with no description."""
        e = _encode_colour(space, icc, channels, palette)
        if self.lib.gk_set_encode_colour(self.ctx, ctypes.byref(e) if e is not None else None) != 0:
            raise ValueError("gk_set_encode_colour: " + self.lib.gk_last_error(self.ctx).decode())

    def set_encode_convert(self, space=None, chroma=(1, 1)):
        """gk_set_encode_convert (sticky): later encode_pixels calls with 3 channels and encode calls with
        a (3, H, W) array take R, G, B, convert them to sYCC ("sycc") or e-sYCC ("esycc") on the
        device with the chroma planes every chroma = (dx, dy) positions ((1, 1), (2, 1), (2, 2): 4:4:4,
        4:2:2, 4:2:0) and encode those planes as encode(..., subsampling=[(1, 1), chroma, chroma])
        does under set_encode_colour(space).  space=None clears it.  A refusal raises ValueError and
        leaves the engine with none."""
        spec = None if space is None else _encode_convert(space, chroma)
        if self.lib.gk_set_encode_convert(self.ctx, ctypes.byref(spec) if spec is not None else None) != 0:
            raise ValueError("gk_set_encode_convert: " + self.lib.gk_last_error(self.ctx).decode())

    def set_encode_roi(self, rects=None, mask=None, shift=0, components=None):
        """gk_set_encode_roi (sticky): later encode / encode_pixels calls code the region, the union of
        rects [(x0, y0, x1, y1)] (half-open, image samples) and the non-zero elements of mask (an
        (H, W) numpy array or torch cuda tensor of 8-bit elements), ahead of the background
        (maxshift): components (None: all) get an RGN marker with `shift` (0: the smallest legal one).
        No rectangle and no mask clears it.  A refusal raises ValueError and leaves the engine with
        none; what depends on the image is refused by the encode (RuntimeError)."""
        r = _encode_roi(rects, mask, shift, components)
        if self.lib.gk_set_encode_roi(self.ctx, ctypes.byref(r) if r is not None else None) != 0:
            raise ValueError("gk_set_encode_roi: " + self.lib.gk_last_error(self.ctx).decode())

    def set_encode_quant(self, step=None, max_bytes=None, psnr=None):
        """gk_set_encode_quant (sticky): later HTJ2K 9/7 encodes quantise with the base step `step`
        (nominal-range units; the default is 2^-(prec + signed)), or with the finest ladder notch
        whose output is at most `max_bytes` long, or with the coarsest one whose estimated PSNR
        reaches `psnr` dB.  Exactly one argument; none clears the setting.  encode_quant() reports
        what an encode did."""
        q = _encode_quant(step, max_bytes, psnr)
        if self.lib.gk_set_encode_quant(self.ctx, ctypes.byref(q) if q is not None else None) != 0:
            raise ValueError("gk_set_encode_quant: " + self.lib.gk_last_error(self.ctx).decode())

    def encode_quant(self):
        """gk_get_encode_quant: the gk_quant_result of the last encode as a dict."""
        r = QuantResult()
        if self.lib.gk_get_encode_quant(self.ctx, ctypes.byref(r)) != 0:
            self._err("gk_get_encode_quant")
        return {k: getattr(r, k) for k, _ in QuantResult._fields_}

    def roi_band_mask(self, shape, prec, params=None, comp=0, tile=0, resolution=0, band=0, signed=False, origin=None,
                      out=None):
        """gk_roi_band_mask: the coefficient mask (uint8, 1 = region) of one band of a (C, H, W) image
        of `prec` bits under `params` and the engine's current region, computed by the kernels the
        encode runs.  band: 0 (LL) at resolution 0; above it 0 HL, 1 LH, 2 HH.  Returns an (h, w)
        numpy array, or with ``out`` (a torch cuda uint8 tensor) fills it on the device and returns
        (h, w)."""
        c, h, w = shape
        info = ImageInfo(w, h, c, prec, int(signed), 0)
        if params is None:
            params = default_params()
        if origin is not None:
            info.x0, info.y0 = int(origin[0]), int(origin[1])
        else:
            info.x0, info.y0 = params.tx0, params.ty0
        bw, bh = ctypes.c_uint32(), ctypes.c_uint32()
        args = (self.ctx, ctypes.byref(info), ctypes.byref(params), comp, tile, resolution, band)
        if out is not None:
            if self.lib.gk_roi_band_mask(*args, ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.byref(bw),
                                         ctypes.byref(bh), 1) != 0:
                self._err("gk_roi_band_mask")
            return bh.value, bw.value
        buf = np.zeros(max(w * h, 1), np.uint8)
        if self.lib.gk_roi_band_mask(*args, buf.ctypes.data, buf.size, ctypes.byref(bw), ctypes.byref(bh), 0) != 0:
            self._err("gk_roi_band_mask")
        return buf[:bw.value * bh.value].reshape(bh.value, bw.value).copy()

    def encode_pixels(self, pixels, prec, signed=False, params=None, out=None, origin=None):
        """gk_encode_pixels: encode packed pixels.  pixels: an (H, W, C) or (H, W) numpy array (host)
        or torch cuda tensor (device) with stride(2) == 1, stride(1) == C and any row stride; its
        element size selects the sample type (4 bytes: int32; 1 / 2 bytes must be (prec + 7) // 8; a
        host array of another type is converted to int32 by value, as ``encode`` converts planes; a
        device tensor of a non-integer type is refused).  The result is the codestream
        ``encode`` writes for the same samples in (C, H, W) planes; params, out and origin as there."""
        if params is None:
            params = default_params()
        on_dev = _is_torch_cuda(pixels)
        if on_dev:   # (a device tensor is read as it lies: its bits must be integer samples)
            if pixels.dtype.is_floating_point or pixels.dtype.is_complex or str(pixels.dtype) == "torch.bool" or \
                    pixels.element_size() not in (1, 2, 4):
                raise ValueError("encode_pixels needs a device tensor of 8-, 16- or 32-bit integers, not %s" % pixels.dtype)
        else:
            pixels = np.asarray(pixels)
            if not (pixels.dtype.kind in "ui" and pixels.dtype.itemsize in (1, 2, 4)) or \
                    (pixels.dtype.itemsize < 4 and pixels.dtype.itemsize != (prec + 7) // 8):
                pixels = np.ascontiguousarray(pixels, dtype=np.int32)
        if pixels.ndim == 2:
            pixels = pixels[:, :, None]
        h, w, c = pixels.shape
        es = pixels.element_size() if on_dev else pixels.dtype.itemsize
        if on_dev:
            st = [pixels.stride(i) for i in range(3)]
            base = pixels.data_ptr()
        else:
            if any(s % es for s in pixels.strides):
                pixels = np.ascontiguousarray(pixels)
            st = [s // es for s in pixels.strides]
            base = pixels.ctypes.data
        if (c > 1 and st[2] != 1) or (w > 1 and st[1] != c) or (h > 1 and st[0] < w * c):
            if on_dev:
                raise ValueError("encode_pixels needs stride(2) == 1, stride(1) == C and a row stride of at least W * C")
            pixels = np.ascontiguousarray(pixels)
            st, base = [w * c, c, 1], pixels.ctypes.data
        row_bytes = (st[0] if h > 1 else w * c) * es
        info = ImageInfo(w, h, c, prec, int(signed), 0 if es == 4 else es)
        if origin is not None:
            info.x0, info.y0 = int(origin[0]), int(origin[1])
        else:
            info.x0, info.y0 = params.tx0, params.ty0
        n = ctypes.c_size_t()
        src = ctypes.c_void_p(base)
        if out is not None:
            rc = self.lib.gk_encode_pixels(self.ctx, ctypes.byref(info), src, row_bytes, int(on_dev), ctypes.byref(params),
                                           ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.byref(n), 1)
            if rc != 0:
                self._err("gk_encode_pixels")
            return n.value
        cap = c * h * w * 4 + (1 << 20)
        buf = np.empty(cap, np.uint8)
        rc = self.lib.gk_encode_pixels(self.ctx, ctypes.byref(info), src, row_bytes, int(on_dev), ctypes.byref(params),
                                       buf.ctypes.data, cap, ctypes.byref(n), 0)
        if rc == -2:
            buf = np.empty(n.value, np.uint8)
            rc = self.lib.gk_encode_pixels(self.ctx, ctypes.byref(info), src, row_bytes, int(on_dev), ctypes.byref(params),
                                           buf.ctypes.data, n.value, ctypes.byref(n), 0)
        if rc != 0:
            self._err("gk_encode_pixels")
        return buf[:n.value].tobytes()

    def _encode_subsampled(self, planes, prec, signed, params, out, origin, subsampling, size):
        c = len(planes)
        w, h = size
        on_dev = _is_torch_cuda(planes[0])
        keep = [p if on_dev else _host_planes(p, prec) for p in planes]
        sb = _sample_bytes(keep[0])
        info = ImageInfo(w, h, c, prec, int(signed), sb)
        if origin is not None:
            info.x0, info.y0 = int(origin[0]), int(origin[1])
        else:
            info.x0, info.y0 = params.tx0, params.ty0
        for k, (dx, dy) in enumerate(subsampling):
            assert tuple(keep[k].shape) == comp_shape(w, h, dx, dy, (info.x0, info.y0)), (k, tuple(keep[k].shape))
        ptrs = (ctypes.c_void_p * c)(*[p.data_ptr() if on_dev else p.ctypes.data for p in keep])
        strides = (ctypes.c_uint32 * c)(*[p.shape[1] for p in keep])
        dxs = (ctypes.c_uint32 * c)(*[int(d[0]) for d in subsampling])
        dys = (ctypes.c_uint32 * c)(*[int(d[1]) for d in subsampling])
        if self.lib.gk_set_subsampling(self.ctx, c, dxs, dys) != 0:
            self._err("gk_set_subsampling")
        try:
            n = ctypes.c_size_t()
            if out is not None:
                rc = self.lib.gk_encode(self.ctx, ctypes.byref(info), ptrs, strides, int(on_dev), ctypes.byref(params),
                                        ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.byref(n), 1)
                if rc != 0:
                    self._err("gk_encode")
                return n.value
            cap = c * h * w * 4 + (1 << 20)
            buf = np.empty(cap, np.uint8)
            rc = self.lib.gk_encode(self.ctx, ctypes.byref(info), ptrs, strides, int(on_dev), ctypes.byref(params),
                                    buf.ctypes.data, cap, ctypes.byref(n), 0)
            if rc != 0:
                self._err("gk_encode")
            return buf[:n.value].tobytes()
        finally:
            self.lib.gk_set_subsampling(self.ctx, 0, None, None)

    def encode_tiles_subsampled(self, planes, prec, tile_begin, tile_end, subsampling, size, signed=False, params=None,
                                origin=None):
        """gk_encode_tiles for an image with subsampled components: planes = whole component
        planes (comp_shape each); only the rows of the selected tiles are read.  Returns
        (bytes, part_lens); with main_header_subsampled and EOC the parts assemble the stream."""
        if params is None:
            params = default_params()
        c = len(planes)
        w, h = size
        keep = [_host_planes(p, prec) for p in planes]
        info = ImageInfo(w, h, c, prec, int(signed), _sample_bytes(keep[0]))
        info.x0, info.y0 = (int(origin[0]), int(origin[1])) if origin is not None else (params.tx0, params.ty0)
        ptrs = (ctypes.c_void_p * c)(*[p.ctypes.data for p in keep])
        strides = (ctypes.c_uint32 * c)(*[p.shape[1] for p in keep])
        dxs = (ctypes.c_uint32 * c)(*[int(d[0]) for d in subsampling])
        dys = (ctypes.c_uint32 * c)(*[int(d[1]) for d in subsampling])
        if self.lib.gk_set_subsampling(self.ctx, c, dxs, dys) != 0:
            self._err("gk_set_subsampling")
        try:
            lens = (ctypes.c_uint32 * (tile_end - tile_begin))()
            n = ctypes.c_size_t()
            cap = sum(p.size for p in keep) * 4 + (1 << 20)
            buf = np.empty(cap, np.uint8)
            rc = self.lib.gk_encode_tiles(self.ctx, ctypes.byref(info), ptrs, strides, 0, ctypes.byref(params),
                                          tile_begin, tile_end, buf.ctypes.data, cap, ctypes.byref(n), lens, 0)
            if rc != 0:
                self._err("gk_encode_tiles")
            hdr = np.empty(1 << 20, np.uint8)
            hn, tlm, nt = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint32()
            if self.lib.gk_main_header(self.ctx, ctypes.byref(info), ctypes.byref(params), hdr.ctypes.data, hdr.size,
                                       ctypes.byref(hn), ctypes.byref(tlm), ctypes.byref(nt)) != 0:
                self._err("gk_main_header")
            return hdr[:hn.value].tobytes(), buf[:n.value].tobytes(), list(lens)
        finally:
            self.lib.gk_set_subsampling(self.ctx, 0, None, None)

    def subsampling(self):
        """[(dx, dy)] per component of the stream the last read_header / decode read."""
        dx, dy = (ctypes.c_uint32 * 16384)(), (ctypes.c_uint32 * 16384)()
        n = self.lib.gk_header_components(self.ctx, dx, dy, None, None, 16384)
        return [(dx[c], dy[c]) for c in range(max(n, 0))]

    def _planes_ptrs(self, planes, row0=0, prec=32):
        """Component base pointers addressing image row 0 for a (C, rows, W) slab whose
        first row is image row ``row0`` (only the slab's rows are ever read)."""
        c, h, w = planes.shape
        if _is_torch_cuda(planes):
            assert planes.is_contiguous() and planes.element_size() in (1, 2, 4)
            base, keep = planes.data_ptr(), planes
        else:
            keep = _host_planes(planes, prec)
            base = keep.ctypes.data
        es = _sample_bytes(keep) or 4
        ptrs = (ctypes.c_void_p * c)(*[base + k * h * w * es - row0 * w * es for k in range(c)])
        return ptrs, keep

    def encode_tiles(self, planes, prec, tile_begin, tile_end, image_hw=None, row0=0, signed=False, params=None,
                     out=None):
        """gk_encode_tiles: tile parts of tiles [tile_begin, tile_end) only (tile sharding).
        planes: (C, rows, W) slab starting at image row ``row0`` (the whole image by
        default); image_hw = (H, W) of the full image.  Returns (bytes or length, part_lens)."""
        if params is None:
            params = default_params()
        c, h, w = planes.shape
        H, W = image_hw if image_hw else (h, w)
        assert W == w
        ptrs, keep = self._planes_ptrs(planes, row0, prec)
        info = ImageInfo(W, H, c, prec, int(signed), _sample_bytes(keep))
        info.x0, info.y0 = params.tx0, params.ty0
        on_dev = _is_torch_cuda(planes)
        strides = (ctypes.c_uint32 * c)(*([w] * c))
        lens = (ctypes.c_uint32 * (tile_end - tile_begin))()
        n = ctypes.c_size_t()
        if out is not None:
            rc = self.lib.gk_encode_tiles(self.ctx, ctypes.byref(info), ptrs, strides, int(on_dev), ctypes.byref(params),
                                          tile_begin, tile_end, ctypes.c_void_p(out.data_ptr()), out.numel(),
                                          ctypes.byref(n), lens, 1)
            if rc != 0:
                self._err("gk_encode_tiles")
            return n.value, list(lens)
        cap = c * h * w * 4 + (1 << 20)
        buf = np.empty(cap, np.uint8)
        rc = self.lib.gk_encode_tiles(self.ctx, ctypes.byref(info), ptrs, strides, int(on_dev), ctypes.byref(params),
                                      tile_begin, tile_end, buf.ctypes.data, cap, ctypes.byref(n), lens, 0)
        if rc != 0:
            self._err("gk_encode_tiles")
        del keep
        return buf[:n.value].tobytes(), list(lens)

    def jp2_header(self, image_shape, prec, cs_len, signed=False):
        """gk_jp2_header: the JP2 boxes in front of a codestream of cs_len bytes."""
        c, h, w = image_shape
        info = ImageInfo(w, h, c, prec, int(signed), 0)
        buf = np.empty(256, np.uint8)
        n = ctypes.c_size_t()
        rc = self.lib.gk_jp2_header(self.ctx, ctypes.byref(info), cs_len, buf.ctypes.data, buf.size, ctypes.byref(n))
        if rc == -2:   # (a colour description set by set_encode_colour: an ICC profile, a palette)
            buf = np.empty(n.value, np.uint8)
            rc = self.lib.gk_jp2_header(self.ctx, ctypes.byref(info), cs_len, buf.ctypes.data, buf.size, ctypes.byref(n))
        if rc != 0:
            self._err("gk_jp2_header")
        return buf[:n.value].tobytes()

    def main_header(self, image_shape, prec, signed=False, params=None):
        """gk_main_header: (header bytes, TLM entry offset or 0, number of tiles)."""
        if params is None:
            params = default_params()
        c, h, w = image_shape
        info = ImageInfo(w, h, c, prec, int(signed), 0)
        info.x0, info.y0 = params.tx0, params.ty0
        buf = np.empty(1 << 20, np.uint8)
        n, tlm, nt = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint32()
        rc = self.lib.gk_main_header(self.ctx, ctypes.byref(info), ctypes.byref(params), buf.ctypes.data, buf.size,
                                     ctypes.byref(n), ctypes.byref(tlm), ctypes.byref(nt))
        if rc != 0:
            self._err("gk_main_header")
        return buf[:n.value].tobytes(), tlm.value, nt.value

    # ------------------------------------------------------------------ decode
    def read_header(self, cs, length=None):
        info = ImageInfo()
        if _is_torch_cuda(cs):
            rc = self.lib.gk_decode_header(self.ctx, ctypes.c_void_p(cs.data_ptr()), length, 1, ctypes.byref(info))
        else:
            b = np.frombuffer(cs, np.uint8)
            rc = self.lib.gk_decode_header(self.ctx, b.ctypes.data, len(cs), 0, ctypes.byref(info))
        if rc != 0:
            self._err("gk_decode_header")
        return info

    def colour_info(self):
        """gk_header_colour: ColourInfo of the stream the last read_header / decode read."""
        info = ColourInfo()
        if self.lib.gk_header_colour(self.ctx, ctypes.byref(info)) != 0:
            self._err("gk_header_colour")
        return info

    def icc_profile(self):
        """gk_header_icc: the ICC profile bytes (colr METH 2) of that stream, b"" without one."""
        n = ctypes.c_size_t()
        self.lib.gk_header_icc(self.ctx, None, 0, ctypes.byref(n))
        if not n.value:
            return b""
        buf = np.empty(n.value, np.uint8)
        if self.lib.gk_header_icc(self.ctx, buf.ctypes.data, buf.size, ctypes.byref(n)) != 0:
            self._err("gk_header_icc")
        return buf.tobytes()

    def cielab(self):
        """gk_header_cielab: the CIELab words (colr EnumCS 14) of that stream as Grok keeps them,
        [14, tag] or [14, 0, rl, ol, ra, oa, rb, ob, il]; [] for any other stream."""
        words, n = (ctypes.c_uint32 * 9)(), ctypes.c_uint32()
        if self.lib.gk_header_cielab(self.ctx, words, ctypes.byref(n)) != 0:
            self._err("gk_header_cielab")
        return [int(words[i]) for i in range(n.value)]

    def set_decode_colour(self, apply):
        """gk_set_decode_colour: apply a JP2 file's palette and channel definition on decode (True,
        the default: planes are the output channels) or return the codestream's components (False)."""
        if self.lib.gk_set_decode_colour(self.ctx, int(bool(apply))) != 0:
            self._err("gk_set_decode_colour")

    def set_decode_display(self, rgb=False, upsample=False, force_rgb=False, icc=False):
        """gk_set_decode_display: what grk_decompress does to the decoded image, on the GPU.  rgb:
        sYCC (4:4:4, 4:2:2, 4:2:0), e-sYCC and CMYK images decode to RGB planes; upsample: subsampled
        components are replicated to the image grid (grk_decompress -u); force_rgb: a grey image's
        channel becomes R, G and B (grk_decompress -f; other channels follow, grey + alpha is RGBA);
        icc: a file's ICC profile (colr METH 2, matrix / tone-curve classes) or CIELab space (EnumCS
        14) is converted to sRGB, as the CLI does for an output that cannot embed a profile.
        Sticky; read_header, subsampling and colour_info then describe the output, so decode returns
        one (C, H, W) array."""
        flags = (GK_DISPLAY_RGB if rgb else 0) | (GK_DISPLAY_UPSAMPLE if upsample else 0) | \
            (GK_DISPLAY_FORCE_RGB if force_rgb else 0) | (GK_DISPLAY_ICC if icc else 0)
        if self.lib.gk_set_decode_display(self.ctx, flags) != 0:
            self._err("gk_set_decode_display")
        self._display_flags = flags

    def set_decode_precision(self, spec):
        """gk_set_decode_precision: force the output channels' precision (grk_decompress -p).
        spec: a list of (prec, "C" | "S") or a -p string such as "8S" or "8S,12C,0S"
        (parse_precision); None or [] clears it.  Channel k takes entry min(k, n - 1); prec 0 keeps
        the channel's precision; S scales as Grok does, C clamps to the forced range.  Sticky;
        read_header reports the forced precisions, and 8 / 16-bit output is sized by them."""
        arr, n = _precision_array(spec)
        if self.lib.gk_set_decode_precision(self.ctx, arr, n) != 0:
            self._err("gk_set_decode_precision")
        self._precision = parse_precision(spec)

    def set_decode_render(self, mode=None, windows=None, tints=None, curve=None, map=None, gamma=None):
        """gk_set_decode_render: the pixel calls (decode_pixels, decode_view) return unsigned 8-bit
        display pixels.  mode: None (clears it), "window" (C channels in, C out), "map" (one channel
        through a (256, 3) uint8 colour map) or "blend" (1..16 tinted channels added into RGB).
        windows: [(lo, hi)] sample values stretched to 0..255, any int32 pair, lo > hi inverts; tints:
        [(r, g, b)] for blend; channel k takes entry min(k, n - 1) of each.  curve: 256 uint8 values
        applied after the window, or gamma=g for round(255 (t / 255)^(1 / g)).  Sticky; read_header
        then reports the rendered channels at 8 bits, and decode / decode_window refuse."""
        r, keep = _render(mode, windows, tints, curve, map, gamma)
        if self.lib.gk_set_decode_render(self.ctx, ctypes.byref(r) if r is not None else None) != 0:
            self._err("gk_set_decode_render")
        del keep
        self._render = r is not None

    def levels(self, cs, region=None, size=None, width=None, height=None, fit=False, bins=4096, length=None,
               origin=None, shift=None):
        """gk_decode_levels: min, max, sum, count and a histogram of exactly the int32 pixels
        decode_view(cs, region, size, ...) returns, per output channel, computed on the GPU without
        writing the pixels (a render that is set is ignored).  region / size / width / height / fit:
        as decode_view (none of the sizes: the region's own).  bins: 1..4096 counters a channel, or 0
        for none.  Without origin= / shift= (one value, or one per channel) the binning is chosen
        from the data: bin 0 starts at the channel's minimum and the shift is the smallest at which
        the maximum fits, which takes a second call when max - min >= bins.  Returns a Levels."""
        bins = int(bins)
        if _is_torch_cuda(cs):
            src, n, on_dev = ctypes.c_void_p(cs.data_ptr()), length, 1
        else:
            b = np.frombuffer(cs, np.uint8)
            src, n, on_dev = ctypes.c_void_p(b.ctypes.data), len(cs), 0
        if size is None and width is None and height is None:
            if region is not None:
                size = (region[2] - region[0], region[3] - region[1])
            else:
                info = self.read_header(cs, length)
                size = (info.w, info.h)
        v = _view(region, size, width, height, fit, 0, False)

        def call(entries):
            q = (LevelsBins * max(len(entries), 1))(*[LevelsBins(int(o), int(s)) for o, s in entries])
            stats, vr = (ChannelLevels * GK_RENDER_MAX_CHANNELS)(), ViewResult()
            hist = np.zeros((GK_RENDER_MAX_CHANNELS, bins), np.uint64) if bins else None
            if self.lib.gk_decode_levels(self.ctx, src, n, on_dev, ctypes.byref(v), q, len(entries), bins, stats,
                                         ctypes.c_void_p(hist.ctypes.data) if bins else None, hist.size if bins else 0,
                                         ctypes.byref(vr)) != 0:
                self._err("gk_decode_levels")
            c = vr.channels
            return [stats[k] for k in range(c)], (hist.reshape(-1)[:c * bins].reshape(c, bins) if bins else None), vr

        if origin is not None or shift is not None:
            as_list = lambda x: list(x) if isinstance(x, (list, tuple)) else [x or 0]
            o, sh = as_list(origin), as_list(shift)
            m = max(len(o), len(sh))
            entries = [(o[min(k, len(o) - 1)], sh[min(k, len(sh) - 1)]) for k in range(m)]
            stats, hist, vr = call(entries)
            c = len(stats)
            ent = [entries[min(k, m - 1)] for k in range(c)]
            return Levels(stats, hist, [e[0] for e in ent], [e[1] for e in ent], vr)
        stats, hist, vr = call([(0, 0)])
        if not bins:
            return Levels(stats, None, [0] * len(stats), [0] * len(stats), vr)
        entries = []
        for st in stats:
            sh = 0
            while ((st.max - st.min) >> sh) >= bins:
                sh += 1
            entries.append((st.min, sh))
        if any(e != (0, 0) for e in entries):
            stats, hist, vr = call(entries)
        return Levels(stats, hist, [e[0] for e in entries], [e[1] for e in entries], vr)

    def precisions(self):
        """[(prec, signed)] per output channel of the stream the last read_header / decode read."""
        pr, sg = (ctypes.c_uint32 * 16384)(), (ctypes.c_uint32 * 16384)()
        n = self.lib.gk_header_components(self.ctx, None, None, pr, sg, 16384)
        return [(pr[c], bool(sg[c])) for c in range(max(n, 0))]

    def decode_pixels(self, cs, length=None, out=None, sample_bytes=0, window=None):
        """gk_decode_pixels / gk_decode_window_pixels: the decoded image as packed pixels.  Returns
        an (H, W, C) numpy array (int32, or 8 / 16-bit with sample_bytes 1 / 2), or fills ``out``: a
        torch cuda tensor of that shape with stride(2) == 1, stride(1) == C and any row stride (its
        element size selects the sample type).  C, H and W are what read_header reports under the
        sticky settings (display flags, precision list, reduce); window = (x0, y0, x1, y1) decodes
        that rectangle only.  Channels of different sizes (subsampled components) need
        set_decode_display(upsample=True)."""
        info = self.read_header(cs, length)
        c = info.numcomps
        red = getattr(self, "_reduce", 0)
        sub = self.subsampling()
        dx, dy = sub[0] if sub else (1, 1)
        cd = lambda a, b: -(-a // b)
        x0, y0, x1, y1 = window if window is not None else (0, 0, info.w, info.h)
        gx = lambda v: cd(cd(v + info.x0, dx), 1 << red)
        gy = lambda v: cd(cd(v + info.y0, dy), 1 << red)
        h, w = gy(y1) - gy(y0), gx(x1) - gx(x0)
        if out is not None:
            assert tuple(out.shape) == (h, w, c) and out.stride(2) == 1 and (w == 1 or out.stride(1) == c)
            sample_bytes = _sample_bytes(out)
            es = sample_bytes or 4
            dst, row_bytes, res, out_dev = ctypes.c_void_p(out.data_ptr()), (out.stride(0) if h > 1 else w * c) * es, out, 1
        else:
            es = sample_bytes or 4
            if getattr(self, "_render", False):   # rendered: unsigned 8-bit whatever was asked
                sample_bytes = es = 1
            res = np.empty((h, w, c), _np_sample_dtype(sample_bytes, info))
            dst, row_bytes, out_dev = ctypes.c_void_p(res.ctypes.data), w * c * es, 0
        if _is_torch_cuda(cs):
            src, n, on_dev = ctypes.c_void_p(cs.data_ptr()), length, 1
        else:
            b = np.frombuffer(cs, np.uint8)
            src, n, on_dev = ctypes.c_void_p(b.ctypes.data), len(cs), 0
        if window is None:
            rc = self.lib.gk_decode_pixels(self.ctx, src, n, on_dev, dst, row_bytes, sample_bytes, out_dev)
        else:
            rc = self.lib.gk_decode_window_pixels(self.ctx, src, n, on_dev, x0, y0, x1, y1, dst, row_bytes, sample_bytes,
                                                  out_dev)
        if rc != 0:
            self._err("gk_decode_pixels")
        return res

    def _view_pix_size(self, src, n, on_dev, v, fit, info):
        """(pix_w, pix_h, None) of the image a view writes, or (0, 0, why).  Host bytes: the engine's
        own answer (gk_probe_view under this engine's display flags and precision list).  Device
        bytes cannot be probed: the size rule restated (_view_size; an all-0 region is the image, as
        in the C ABI)."""
        if not on_dev:
            arr, np_ = _precision_array(self._precision)
            msg = ctypes.create_string_buffer(512)
            pr = ViewResult()
            if self.lib.gk_probe_view(src, n, self._display_flags, arr, np_, ctypes.byref(v), ctypes.byref(pr), msg, 512) == 0:
                return pr.pix_w, pr.pix_h, None
            return 0, 0, msg.value.decode()
        whole = not (v.x0 or v.y0 or v.x1 or v.y1)
        bw, bh = (info.w, info.h) if whole else (v.x1 - v.x0, v.y1 - v.y0)
        try:
            ow, oh = _view_size(bw, bh, v.out_w, v.out_h, fit) if bw > 0 and bh > 0 else (0, 0)
        except ValueError:
            ow = oh = 0
        if 0 < ow <= bw and 0 < oh <= bh:
            return (oh, ow, None) if v.rotate in (90, 270) else (ow, oh, None)
        return 0, 0, "the view has no size here"

    def decode_tensor(self, cs, region=None, size=None, width=None, height=None, fit=False, rotate=0, mirror=False,
                      dtype="float32", layout="chw", scale=None, bias=None, mean=None, std=None, unit=None,
                      out=None, length=None):
        """gk_decode_view_tensor: the view decode_view(cs, region, size, ...) returns as int32, written
        by the GPU as normalised floats, x = float32(v) * scale_k + bias_k in two float32 roundings
        and then rounded to the tensor's type (include/grok_amd.h has the exact rule).  region /
        size / width / height / fit / rotate / mirror: as decode_view (none of the sizes: the
        region's own).  scale / bias: a number or one per channel (None: 1 / 0); or mean / std (a
        number or one per channel) with unit: scale_k = 1 / (unit std_k), bias_k = -mean_k / std_k
        (_tensor_affine), unit defaulting to 2^prec - 1 of an unsigned view.  Without ``out`` it
        returns a dense numpy array of dtype "float32" or "float16" and layout "chw" (C, H, W) or "hwc"
        (H, W, C).  ``out``: a 3-d torch cuda tensor in float32 / float16 / bfloat16 of that shape
        in `layout`; its dtype decides and its stride() values go to the engine as they are, so a
        slice batch[i] of a batch tensor and a channels_last tensor both work.  Every sticky decode
        setting is honoured, except that set_decode_reduce must be 0 and a render must be cleared.
        The resolved view is kept as self.view_result."""
        if layout not in ("chw", "hwc"):
            raise ValueError("tensor: layout %r (chw or hwc)" % (layout,))
        if (scale is not None or bias is not None) and (mean is not None or std is not None or unit is not None):
            raise ValueError("tensor: give scale= / bias= or mean= / std= / unit=, not both")
        if _is_torch_cuda(cs):
            src, n, on_dev = ctypes.c_void_p(cs.data_ptr()), length, 1
        else:
            b = np.frombuffer(cs, np.uint8)
            src, n, on_dev = ctypes.c_void_p(b.ctypes.data), len(cs), 0
        info = self.read_header(cs, length)
        if size is None and width is None and height is None:
            size = (region[2] - region[0], region[3] - region[1]) if region is not None else (info.w, info.h)
        v, vr = _view(region, size, width, height, fit, rotate, mirror), ViewResult()
        w, h, why = self._view_pix_size(src, n, on_dev, v, fit, info)
        if why is not None or getattr(self, "_render", False):
            # The engine names its refusal itself.  It is asked with a host tensor of overlapping strides,
            # which is refused after the refusals that concern the settings and the view.
            one = np.zeros(1, np.int64)
            t, keep = _tensor_description("float32", (1, 1, 1), None, None, one.ctypes.data, False)
            self.lib.gk_decode_view_tensor(self.ctx, src, n, on_dev, ctypes.byref(v), ctypes.byref(t), ctypes.byref(vr))
            err = self.lib.gk_last_error(self.ctx).decode()
            raise RuntimeError("gk_decode_view_tensor failed: %s" % (why if why and "tensor: " in err else err))
        if mean is not None or std is not None or unit is not None:
            scale, bias = _tensor_affine(mean, std, unit, info.prec, info.sgnd)
        c = info.numcomps
        shape = (c, h, w) if layout == "chw" else (h, w, c)
        if out is not None:
            if not _is_torch_cuda(out) or out.dim() != 3 or tuple(out.shape) != shape:
                raise ValueError("tensor: out must be a torch cuda tensor of shape %r (%s)" % (shape, layout))
            st = out.stride()
            strides = st if layout == "chw" else (st[2], st[0], st[1])
            t, keep = _tensor_description(out.dtype, strides, scale, bias, out.data_ptr(), True)
            res = out
        else:
            if _tensor_dtype(dtype) == GK_TENSOR_BF16:
                raise ValueError("tensor: numpy has no bfloat16: give out= (a torch cuda tensor)")
            res = np.empty(shape, np.float32 if _tensor_dtype(dtype) == GK_TENSOR_F32 else np.float16)
            strides = (h * w, w, 1) if layout == "chw" else (1, w * c, c)
            t, keep = _tensor_description(dtype, strides, scale, bias, res.ctypes.data, False)
        if self.lib.gk_decode_view_tensor(self.ctx, src, n, on_dev, ctypes.byref(v), ctypes.byref(t), ctypes.byref(vr)) != 0:
            self._err("gk_decode_view_tensor")
        del keep
        if (vr.pix_h, vr.pix_w, vr.channels) != (h, w, c):
            raise RuntimeError("gk_decode_view_tensor wrote %d x %d x %d pixels into a tensor of %d x %d x %d"
                               % (vr.pix_h, vr.pix_w, vr.channels, h, w, c))
        self.view_result = vr
        return res

    def decode_view(self, cs, region=None, size=None, width=None, height=None, fit=False, rotate=0, mirror=False,
                    out=None, sample_bytes=0, length=None):
        """gk_decode_view_pixels: region = (x0, y0, x1, y1) of the image (None: all of it) at exactly
        size = (w, h) pixels, or width= / height= alone (the other keeps the aspect), or both with
        fit=True (the largest size of the region's aspect inside them); then mirrored left-right
        and rotated clockwise by rotate = 0 / 90 / 180 / 270 (parse_iiif makes these arguments of
        IIIF strings).  The engine picks the reduce level, decodes the region there and area-averages
        it on the GPU (include/grok_amd.h has the exact rule).  Returns a (pix_h, pix_w, C) numpy
        array (int32, or 8 / 16-bit with sample_bytes 1 / 2), or fills ``out``: a torch cuda tensor of
        that shape under decode_pixels' stride rules.  Every sticky decode setting is honoured,
        except that set_decode_reduce must be 0.  The resolved view is kept as self.view_result."""
        v = _view(region, size, width, height, fit, rotate, mirror)
        info = self.read_header(cs, length)
        c = info.numcomps
        if _is_torch_cuda(cs):
            src, n, on_dev = ctypes.c_void_p(cs.data_ptr()), length, 1
        else:
            b = np.frombuffer(cs, np.uint8)
            src, n, on_dev = ctypes.c_void_p(b.ctypes.data), len(cs), 0
        vr = ViewResult()
        w, h, why = self._view_pix_size(src, n, on_dev, v, fit, info)
        if why is not None:
            # The engine names its refusal itself.  It is asked with row_bytes 0, which is below any row
            # and so is refused, after the refusals that concern the view, before a byte is written.
            one = np.zeros(1, np.int64)
            self.lib.gk_decode_view_pixels(self.ctx, src, n, on_dev, ctypes.byref(v), ctypes.c_void_p(one.ctypes.data), 0,
                                           sample_bytes if out is None else _sample_bytes(out), 0, ctypes.byref(vr))
            err = self.lib.gk_last_error(self.ctx).decode()
            raise RuntimeError("gk_decode_view_pixels failed: %s" % (why if "row_bytes 0 " in err else err))
        if out is not None:
            assert tuple(out.shape) == (h, w, c) and out.stride(2) == 1 and (w == 1 or out.stride(1) == c)
            sample_bytes = _sample_bytes(out)
            es = sample_bytes or 4
            dst, row_bytes, res, out_dev = ctypes.c_void_p(out.data_ptr()), (out.stride(0) if h > 1 else w * c) * es, out, 1
        else:
            es = sample_bytes or 4
            if getattr(self, "_render", False):   # rendered: unsigned 8-bit whatever was asked
                sample_bytes = es = 1
            res = np.empty((h, w, c), _np_sample_dtype(sample_bytes, info))
            dst, row_bytes, out_dev = ctypes.c_void_p(res.ctypes.data), w * c * es, 0
        if self.lib.gk_decode_view_pixels(self.ctx, src, n, on_dev, ctypes.byref(v), dst, row_bytes, sample_bytes,
                                          out_dev, ctypes.byref(vr)) != 0:
            self._err("gk_decode_view_pixels")
        if (vr.pix_h, vr.pix_w, vr.channels) != (h, w, c):
            raise RuntimeError("gk_decode_view_pixels wrote %d x %d x %d pixels into an array of %d x %d x %d"
                               % (vr.pix_h, vr.pix_w, vr.channels, h, w, c))
        self.view_result = vr
        return res

    def decode_window(self, cs, window, length=None, out=None, sample_bytes=0):
        """gk_decode_window: window = (x0, y0, x1, y1).  Returns a (C, y1-y0, x1-x0) numpy
        array (int32, or 8/16-bit with sample_bytes 1/2), or fills ``out`` (a torch cuda
        tensor of that shape; its element size selects the sample type) in place.  With
        set_decode_reduce(r) the window (full-resolution coordinates) is returned at the
        reduced resolution: its canvas rectangle with every edge ceil(x / 2^r)."""
        on_dev = _is_torch_cuda(cs)
        info = self.read_header(cs, length)
        x0, y0, x1, y1 = window
        c, h, w = info.numcomps, y1 - y0, x1 - x0
        sub = self.subsampling()
        if any(d != (1, 1) for d in sub):
            return self._window_subsampled(cs, length, window, out, sample_bytes, info, sub)
        red = getattr(self, "_reduce", 0)
        if red:   # the window's canvas rectangle reduced: ceil(x / 2^reduce) (set_decode_reduce)
            cd = lambda v: -(-v >> red)
            w = cd(x1 + info.x0) - cd(x0 + info.x0)
            h = cd(y1 + info.y0) - cd(y0 + info.y0)
        if out is not None:
            # any (C, h, w) view with unit column stride (e.g. a row band of a larger window)
            assert tuple(out.shape) == (c, h, w) and out.stride(2) == 1
            base, res, out_dev = out.data_ptr(), out, 1
            sample_bytes = _sample_bytes(out)
            es = sample_bytes or 4
            cstride, rstride = out.stride(0), out.stride(1)
        else:
            res = np.empty((c, h, w), _np_sample_dtype(sample_bytes, info))
            base, out_dev = res.ctypes.data, 0
            es = sample_bytes or 4
            cstride, rstride = h * w, w
        strides = (ctypes.c_uint32 * c)(*([rstride] * c))
        ptrs = (ctypes.c_void_p * c)(*[base + k * cstride * es for k in range(c)])
        if on_dev:
            rc = self.lib.gk_decode_window(self.ctx, ctypes.c_void_p(cs.data_ptr()), length, 1, x0, y0, x1, y1, ptrs,
                                           strides, sample_bytes, out_dev)
        else:
            b = np.frombuffer(cs, np.uint8)
            rc = self.lib.gk_decode_window(self.ctx, b.ctypes.data, len(cs), 0, x0, y0, x1, y1, ptrs, strides,
                                           sample_bytes, out_dev)
        if rc != 0:
            self._err("gk_decode_window")
        return res

    def set_decode_layers(self, max_layers):
        """gk_set_decode_layers: decode only the first max_layers quality layers (0 = all),
        as grk_decompress -l (grk_dparameters::cp_layer)."""
        if self.lib.gk_set_decode_layers(self.ctx, int(max_layers)) != 0:
            self._err("gk_set_decode_layers")

    def set_decode_reduce(self, reduce):
        """gk_set_decode_reduce: discard the `reduce` highest resolutions (grk_decompress -r,
        grk_dparameters::cp_reduce); decode() then returns ceil(H / 2^reduce) x ceil(W / 2^reduce)."""
        if self.lib.gk_set_decode_reduce(self.ctx, int(reduce)) != 0:
            self._err("gk_set_decode_reduce")
        self._reduce = int(reduce)

    def set_window_rule(self, whole_tile):
        """gk_set_window_rule: later windows use Grok's whole-tile inverse 5/3 rule (True, as
        decompressTile without a window) or its partial-tile rule (False, the default)."""
        if self.lib.gk_set_window_rule(self.ctx, int(bool(whole_tile))) != 0:
            self._err("gk_set_window_rule")

    def decode(self, cs, length=None, out=None, row0=0, sample_bytes=0):
        """cs: bytes (host) or torch cuda uint8 tensor (+length).  C counts the output channels
        (a JP2 palette / channel definition applied, see set_decode_colour).  Returns a (C, H, W)
        numpy array (int32, or 8/16-bit with sample_bytes 1/2), or fills ``out`` (torch
        cuda tensor; its element size selects the sample type) in place.  ``out`` may be
        a (C, rows, W) slab holding image rows [row0, row0+rows) when cs carries only the
        tile parts of those rows (sharded decode)."""
        on_dev = _is_torch_cuda(cs)
        info = self.read_header(cs, length)
        c, h, w = info.numcomps, info.h, info.w
        red = getattr(self, "_reduce", 0)
        sub = self.subsampling()
        if any(d != (1, 1) for d in sub):
            return self._decode_subsampled(cs, length, out, sample_bytes, info, sub, red)
        if red:   # reduced-resolution output: the image area on the reduced canvas (ceil(x / 2^reduce))
            cd = lambda v: -(-v // (1 << red))
            h, w = cd(info.y0 + h) - cd(info.y0), cd(info.x0 + w) - cd(info.x0)
        strides = (ctypes.c_uint32 * c)(*([w] * c))
        if out is not None:
            sample_bytes = _sample_bytes(out)
            es = sample_bytes or 4
            base = out.data_ptr()
            rows = out.shape[1]
            ptrs = (ctypes.c_void_p * c)(*[base + k * rows * w * es - row0 * w * es for k in range(c)])
            res, out_dev = out, 1
        else:
            es = sample_bytes or 4
            res = np.empty((c, h, w), _np_sample_dtype(sample_bytes, info))
            base = res.ctypes.data
            ptrs = (ctypes.c_void_p * c)(*[base + k * h * w * es for k in range(c)])
            out_dev = 0
        if on_dev:
            rc = self.lib.gk_decode(self.ctx, ctypes.c_void_p(cs.data_ptr()), length, 1, ptrs, strides, sample_bytes,
                                    out_dev)
        else:
            b = np.frombuffer(cs, np.uint8)
            rc = self.lib.gk_decode(self.ctx, b.ctypes.data, len(cs), 0, ptrs, strides, sample_bytes, out_dev)
        if rc != 0:
            self._err("gk_decode")
        return res

    def _decode_subsampled(self, cs, length, out, sample_bytes, info, sub, red):
        """Subsampled components: a list of 2-D planes, component c of comp_shape(W, H, dx, dy,
        origin, reduce); ``out`` (torch cuda) is then a list of such tensors filled in place."""
        c = info.numcomps
        shapes = [comp_shape(info.w, info.h, dx, dy, (info.x0, info.y0), red) for dx, dy in sub]
        if out is not None:
            assert len(out) == c and all(tuple(o.shape) == s for o, s in zip(out, shapes))
            sample_bytes = _sample_bytes(out[0])
            res, out_dev = out, 1
            ptrs = (ctypes.c_void_p * c)(*[o.data_ptr() for o in out])
            strides = (ctypes.c_uint32 * c)(*[o.stride(0) for o in out])
        else:
            res = [np.empty(s, _np_sample_dtype(sample_bytes, info)) for s in shapes]
            out_dev = 0
            ptrs = (ctypes.c_void_p * c)(*[r.ctypes.data for r in res])
            strides = (ctypes.c_uint32 * c)(*[s[1] for s in shapes])
        if _is_torch_cuda(cs):
            rc = self.lib.gk_decode(self.ctx, ctypes.c_void_p(cs.data_ptr()), length, 1, ptrs, strides, sample_bytes,
                                    out_dev)
        else:
            b = np.frombuffer(cs, np.uint8)
            rc = self.lib.gk_decode(self.ctx, b.ctypes.data, len(cs), 0, ptrs, strides, sample_bytes, out_dev)
        if rc != 0:
            self._err("gk_decode")
        return res

    def _window_subsampled(self, cs, length, window, out, sample_bytes, info, sub):
        """Window of a stream with subsampled components: component c's plane is the window's
        canvas rectangle on its grid (every edge ceil(x / dx), then reduced), a list of planes."""
        x0, y0, x1, y1 = window
        red = getattr(self, "_reduce", 0)
        cd = lambda a, b: -(-a // b)
        shapes = []
        for dx, dy in sub:
            gx = lambda v: cd(cd(v + info.x0, dx), 1 << red)
            gy = lambda v: cd(cd(v + info.y0, dy), 1 << red)
            shapes.append((gy(y1) - gy(y0), gx(x1) - gx(x0)))
        c = info.numcomps
        if out is not None:
            assert len(out) == c and all(tuple(o.shape) == s for o, s in zip(out, shapes))
            sample_bytes = _sample_bytes(out[0])
            res, out_dev = out, 1
            ptrs = (ctypes.c_void_p * c)(*[o.data_ptr() for o in out])
            strides = (ctypes.c_uint32 * c)(*[o.stride(0) for o in out])
        else:
            res = [np.empty(s, _np_sample_dtype(sample_bytes, info)) for s in shapes]
            out_dev = 0
            ptrs = (ctypes.c_void_p * c)(*[r.ctypes.data for r in res])
            strides = (ctypes.c_uint32 * c)(*[max(s[1], 1) for s in shapes])
        if _is_torch_cuda(cs):
            rc = self.lib.gk_decode_window(self.ctx, ctypes.c_void_p(cs.data_ptr()), length, 1, x0, y0, x1, y1, ptrs,
                                           strides, sample_bytes, out_dev)
        else:
            b = np.frombuffer(cs, np.uint8)
            rc = self.lib.gk_decode_window(self.ctx, b.ctypes.data, len(cs), 0, x0, y0, x1, y1, ptrs, strides,
                                           sample_bytes, out_dev)
        if rc != 0:
            self._err("gk_decode_window")
        return res
