"""The float-tensor rule of gk_decode_view_tensor (include/grok_amd.h) in numpy.

    f = float32(v)     g = f * scale_k     z = g + bias_k        each rounded to nearest even
    out = z, float16(z) or bfloat16(z), rounded to nearest even

numpy rounds every float32 operation on its own (nothing here is fused), `astype(np.float16)`
rounds to nearest even, and bfloat16, which numpy does not have, is rounded on the float32's bits
and returned as uint16 bits.  test_tensor.py holds all three to torch on the CPU."""
import numpy as np

SMALLEST_NORMAL = {"float32": 2.0 ** -126, "float16": 2.0 ** -14, "bfloat16": 2.0 ** -126}


def per_channel(x, c, default):
    """Entry min(k, n - 1) of a number or a list, for k < c, as float32; None: `default`."""
    a = np.atleast_1d(np.asarray(default if x is None else x, np.float64)).astype(np.float32)
    return a[np.minimum(np.arange(c), len(a) - 1)]


def bfloat16_bits(z):
    """float32 -> bfloat16 bits (uint16), round to nearest even; z holds no NaN."""
    u = np.ascontiguousarray(z, np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def apply(pixels, scale=None, bias=None, dtype="float32", layout="chw"):
    """(H, W, C) int32 pixels of a view -> the tensor the engine writes: a float32 or float16 array,
    or uint16 bits for bfloat16, as (C, H, W) or (H, W, C).  Asserts that no result is subnormal (or
    below the smallest normal) in the output type: the rule does not pin those, so such an input is
    a bad test input."""
    pixels = np.asarray(pixels)
    assert pixels.ndim == 3 and pixels.dtype == np.int32
    c = pixels.shape[2]
    f = pixels.astype(np.float32)
    g = f * per_channel(scale, c, 1.0)
    z = g + per_channel(bias, c, 0.0)
    assert z.dtype == np.float32 and np.isfinite(z).all()
    for stage in (g, z):
        tiny = (stage != 0) & (np.abs(stage) < 2.0 ** -126)
        assert not tiny.any(), "a subnormal float32 on the way"
    tiny = (z != 0) & (np.abs(z.astype(np.float64)) < SMALLEST_NORMAL[dtype])
    assert not tiny.any(), "%d results are subnormal in %s (e.g. %r): choose other constants" % (tiny.sum(), dtype, float(z[tiny][0]))
    if dtype == "float16":
        with np.errstate(over="ignore"):
            out = z.astype(np.float16)
    elif dtype == "bfloat16":
        out = bfloat16_bits(z)
    else:
        assert dtype == "float32"
        out = z
    return np.ascontiguousarray(out.transpose(2, 0, 1) if layout == "chw" else out)


def bits(a):
    """The bit patterns of a float32 / float16 array (uint16 bits pass through)."""
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint16 else a.view({4: np.uint32, 2: np.uint16}[a.dtype.itemsize])
