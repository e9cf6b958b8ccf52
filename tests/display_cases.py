"""Inputs of the display tests (tests/test_display.py on the CPU, tests/test_gpu_display.py on the
GPU): component planes on their subsampled grids and the JP2 wrapping that names the colour space.
Streams are lossless 5/3 without MCT, so a decode returns the planes that were encoded."""
import numpy as np

import jp2_boxes as J

SYCC, EYCC, CMYK, SRGB = 18, 24, 12, 16   # colr EnumCS
S444 = [(1, 1), (1, 1), (1, 1)]
S422 = [(1, 1), (2, 1), (2, 1)]
S420 = [(1, 1), (2, 2), (2, 2)]


def comp_shape(w, h, dx, dy, origin=(0, 0)):
    x0, y0 = origin
    return -(-(y0 + h) // dy) - -(-y0 // dy), -(-(x0 + w) // dx) - -(-x0 // dx)


def random_planes(w, h, sub, prec, origin=(0, 0), seed=1, signed=False):
    rng = np.random.RandomState(seed)
    lo, hi = (-(1 << (prec - 1)), 1 << (prec - 1)) if signed else (0, 1 << prec)
    return [rng.randint(lo, hi, comp_shape(w, h, dx, dy, origin)).astype(np.int32) for dx, dy in sub]


def numres_for(w, h, sub):
    """Resolutions that the smallest component still has samples for."""
    m = min(min(comp_shape(w, h, dx, dy)) for dx, dy in sub)
    return max(1, min(3, int(m).bit_length()))


def wrap(cs, w, h, nc, prec, enumcs, signed=False, extra=()):
    """The codestream in a JP2 file whose colr box names `enumcs`."""
    return J.jp2_file(cs, [J.ihdr(h, w, nc, prec, signed), J.colr_enum(enumcs)] + list(extra))


def set_ssiz(cs, comp, prec, signed=False):
    """The raw codestream with component `comp`'s SIZ Ssiz rewritten (header probes only)."""
    b = bytearray(cs)
    assert b[:4] == b"\xff\x4f\xff\x51"
    b[42 + 3 * comp] = (prec - 1) | (0x80 if signed else 0)
    return bytes(b)
