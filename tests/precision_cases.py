"""Sample precisions 1..31, shared by the CPU tests (tests/test_precision.py: the oracle against the
source and OpenJPEG 2.5.4) and the GPU tests (tests/test_gpu_precision.py: the HIP engine against
the oracle).

Every image is 37 x 45 with 32 x 32 code-blocks: both sides odd, the width eleven vectors of four
samples and a tail of one, more than one code-block per band.

TOP is the highest precision the encoders accept per coding (DESIGN.md §7 derives it from the
coders' containers); above it `encode` raises an error that names the precision."""
import numpy as np

W, H = 37, 45
CBLK = (32, 32)
HT = 0x40

# (ht, irreversible, components, numres) -> highest accepted precision.  Part-1 5/3: the largest
# band magnitude (input range x the band's BIBO gain: 4 at the finest HH, 2.5 * 1.625 at the
# second level's HL) in 26 bits, RCT chroma one bit wider; HT 5/3: the band's exponent + 1 guard
# bit within 30 bit-planes; 9/7: float32 samples (25 bits) and the largest quantiser index in
# 26 bits (Part 1) or 30 bit-planes (HT).
TOP = {
    (False, False, 1, 1): 25, (False, False, 1, 3): 24, (False, False, 3, 1): 24, (False, False, 3, 3): 23,
    # one level: the checkerboard's finest HH fills all 26 bits at the top (2^26 - 2, 2^26 - 4 under RCT)
    (False, False, 1, 2): 25, (False, False, 3, 2): 24,
    (True, False, 1, 1): 27, (True, False, 1, 3): 27, (True, False, 3, 1): 27, (True, False, 3, 3): 27,
    (False, True, 1, 1): 25, (False, True, 1, 3): 24, (False, True, 3, 1): 25, (False, True, 3, 3): 24,
    (True, True, 1, 1): 25, (True, True, 1, 3): 25, (True, True, 3, 1): 25, (True, True, 3, 3): 25,
}
CODINGS = sorted(TOP)
# one precision per sample container class (1, 2, 4 bytes): tiled with an image offset, which
# takes the parity-general DWT kernels
TILED_PRECISIONS = (5, 11, 20)
TILED = dict(tiles=(32, 32), origin=(1, 1))
# constant planes: the precisions either side of a container boundary (the coding's top is added)
ENDS_PRECISIONS = (1, 7, 9, 15, 17)
# 9/7 with rate control, decoded samples pushed past both ends of the range: the inverse clamp
CLAMP_PRECISIONS = (4, 5, 7, 8, 9, 12, 15, 16, 20, 24)
CLAMP_RATE = [8.0]
# (precision, components) whose streams at that rate are too short to reach the range ends
CLAMP_RATE_OTHER = {(4, 1): [4.0], (5, 1): [4.0]}


def clamp_rate(p, nc):
    return CLAMP_RATE_OTHER.get((p, nc), CLAMP_RATE)


def top(ht, irreversible, nc, numres):
    return TOP[(bool(ht), bool(irreversible), nc, numres)]


def ident(coding):
    """Test id of a TOP key."""
    ht, irreversible, nc, numres = coding
    return "%s-%s-c%d-r%d" % ("ht" if ht else "p1", "97" if irreversible else "53", nc, numres)


def sample_range(p, signed):
    """(lowest, highest) sample value."""
    return (-(1 << (p - 1)), (1 << (p - 1)) - 1) if signed else (0, (1 << p) - 1)


def rand(p, signed, nc, seed=0):
    """Seeded uniform samples over the full range, both range ends planted in the first row."""
    lo, hi = sample_range(p, signed)
    rng = np.random.default_rng(1000 * p + 10 * nc + int(signed) + 100000 * seed)
    img = rng.integers(lo, hi + 1, size=(nc, H, W), dtype=np.int64)
    img[:, 0, 0] = lo
    img[:, 0, 1] = hi
    return img.astype(np.int32)


def chk(p, signed, nc):
    """Checkerboard of the two range ends (the finest HH band's worst case); the second of three
    planes inverted, so that RCT chroma reaches its full range."""
    lo, hi = sample_range(p, signed)
    y, x = np.mgrid[0:H, 0:W]
    a = np.where((y + x) % 2 == 1, hi, lo).astype(np.int64)
    img = np.stack([a] * nc)
    if nc >= 3:
        img[1] = lo + hi - a
    return img.astype(np.int32)


def ends(p, signed, nc):
    """Two images: every plane constant at the lowest, and at the highest, sample value."""
    lo, hi = sample_range(p, signed)
    return [np.full((nc, H, W), v, np.int32) for v in (lo, hi)]


def worst_hl(p, nc):
    """The range ends laid out along the signs of the second level's high-pass analysis filter
    (low-pass (-1 2 6 2 -1) / 8, then (-1 2 -1) / 2 on every other sample: absolute sum 2.5)
    along both axes, about sample 10: a 5/3 coefficient of the second level near its BIBO
    bound.  With three components the pattern is B - G (RCT Cb)."""
    h2 = np.convolve([-.5, 0, 1, 0, -.5], np.array([-1, 2, 6, 2, -1]) / 8.0)

    def line(n):
        s = np.ones(n)
        for i, v in enumerate(h2):
            if v:
                s[10 - len(h2) // 2 + i] = np.sign(v)
        return s
    hi = (1 << p) - 1
    a = np.where(np.outer(line(H), line(W)) > 0, hi, 0).astype(np.int64)
    img = np.stack([hi - a, hi - a, a]) if nc >= 3 else a[None]
    return img.astype(np.int32)


def oracle_kw(ht, irreversible, numres, tiled=False, layer_rate=None):
    kw = dict(numres=numres, cblk=CBLK, cblk_sty=HT if ht else 0, irreversible=bool(irreversible))
    if tiled:
        kw.update(TILED)
    if layer_rate:
        kw["layer_rate"] = layer_rate
    return kw


def engine_kw(ht, irreversible, numres, tiled=False, layer_rate=None):
    """(grok_amd.default_params keyword arguments, encode origin)."""
    kw = dict(numresolution=numres, cblk=CBLK, cblk_sty=HT if ht else 0, irreversible=bool(irreversible))
    if tiled:
        kw["tiles"] = TILED["tiles"]
    if layer_rate:
        kw.update(layer_rate=layer_rate, numlayers=len(layer_rate))
    return kw, (TILED["origin"] if tiled else None)


def tol97(p):
    """Engine against oracle on a 9/7 decode: 1 LSB up to 16 bits; above, the same divergence in
    float32 units, where the sample LSB loses one bit against the float's ulp per bit of precision."""
    return 1 if p <= 16 else 2 ** (p - 16)
