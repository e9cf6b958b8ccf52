"""The cases on which the oracle and the engine are held to Grok 9.2.0 itself: shared by
tests/test_grok_live.py (the live binaries, tests/grok_ref.py), tests/golden/make_grok_fixtures.py
(the committed recordings under tests/golden/grok/) and tests/test_gpu_grok_live.py.

Every image is grok_amd.synth.synth_image(h, w, c, bits, seed) of at most 100 samples a side, but
"big" (130 x 150) and "sq" (128 x 128) for the cases that need several 64 x 64 tiles.  Signed cases
go to grk_compress as PGX (see image()).
"""
import numpy as np

from conftest import parse_flags
from grok_amd.synth import synth_image

IMAGES = {
    "rgb": (67, 93, 3, 8, 5), "rgb10": (67, 93, 3, 10, 5), "rgb12": (67, 93, 3, 12, 5), "rgb16": (67, 93, 3, 16, 5),
    "m8": (50, 41, 1, 8, 5), "m10": (50, 41, 1, 10, 5), "m12": (50, 41, 1, 12, 5), "m16": (50, 41, 1, 16, 5),
    "thin": (33, 2, 1, 8, 5), "one": (1, 1, 1, 8, 5), "big": (130, 150, 3, 8, 5), "bigm16": (130, 150, 1, 16, 5),
    "sq": (128, 128, 3, 8, 5), "sqm16": (128, 128, 1, 16, 5),
    # the shapes of tests/test_gpu_offsets.py::CASES
    "off8": (90, 110, 3, 8, 51), "off12": (120, 100, 3, 12, 55), "off16": (100, 96, 1, 16, 56), "off8b": (97, 113, 3, 8, 57),
}
_cache = {}


def image(key):
    """(image as Grok is given it, image as the encoder sees it, bits, signed): (C, H, W) int32.

    `p:` before a key: a signed component of non-negative samples (the image halved).  `s:`: the
    image minus 2^(bits-1), 8 or 16 bits.  Grok's PGX reader takes a signed sample as the unsigned
    byte or word it is stored in, so what its encoder sees, and what the
    oracle is given here, is the sample modulo 2^8 or 2^16."""
    if key not in _cache:
        kind, k = (key[0], key[2:]) if key[1:2] == ":" else ("", key)
        bits = IMAGES[k][3]
        a = synth_image(*IMAGES[k]).astype(np.int32)
        if kind == "p":
            a = a >> 1
        elif kind == "s":
            assert bits in (8, 16)
            a = a - (1 << (bits - 1))
        seen = a & ((1 << bits) - 1) if kind == "s" else a
        a.setflags(write=False)
        seen.setflags(write=False)
        _cache[key] = (a, seen, bits, kind != "")
    return _cache[key]


# (image, grk_compress flags): the oracle's bytes equal Grok's.  What Grok gets wrong or refuses in
# these families is named case by case in tests/test_grok_defects.py.
ENCODE = [
    # each option family on its own: depths, mode switches, layers, tile parts, markers, offsets, HT
    ("rgb", ""), ("m8", ""), ("m10", ""), ("m12", ""), ("m16", ""),
    ("rgb", "-M 1"), ("rgb", "-M 2"), ("rgb", "-M 4"), ("rgb", "-M 8"), ("rgb", "-M 16"), ("rgb", "-M 32"),
    ("rgb", "-M 63"), ("rgb", "-M 63 -r 20,5 -n 3"), ("m16", "-M 63"),
    ("rgb", "-q 30,40"), ("rgb", "-I -q 30,40,50"),
    ("big", "-t 64,64 -u R"), ("big", "-t 64,64 -u C -p CPRL"), ("rgb", "-u R"), ("rgb", "-u C"),
    ("rgb", "-p RLCP -r 20,10,1 -c [32,32],[16,16] -S -E"), ("rgb", "-p LRCP -r 30,10 -c [64,64] -S -E"),
    ("rgb", "-t 13,7 -n 3"), ("rgb", "-d 3,5"), ("rgb", "-d 1,1 -t 13,7 -n 3"),
    ("rgb", "-d 100,200 -T 90,150 -t 64,64"), ("rgb", "-d 65,33 -T 64,32 -t 32,32 -X -L -p RPCL"),
    ("rgb12", "-d 33,21 -T 31,20 -t 64,32 -I"),
    ("m16", "-M 64"), ("sq", "-M 64 -t 64,64 -X -L"), ("sqm16", "-M 64 -t 32,32 -X -L"),
    ("rgb16", ""), ("rgb16", "-I"), ("rgb12", "-I"), ("rgb10", "-I -r 20,8"),
    ("rgb", "-b 1024,4"), ("thin", "-n 6"), ("one", ""), ("one", "-n 1"),
    # tests/test_gpu_offsets.py::CASES where Grok is sound (the others: tests/test_grok_defects.py)
    ("off8", "-d 3,5"), ("off8", "-d 1,1 -t 13,7 -n 3"), ("off8", "-d 100,200 -T 90,150 -t 64,64"),
    ("off8", "-T 7,3 -t 40,40"), ("off12", "-d 33,21 -T 31,20 -t 64,32 -I"),
    ("off8b", "-d 65,33 -T 64,32 -t 32,32 -X -L -p RPCL"),
    # tests/test_gpu_odd_tiles.py
    ("big", "-t 100,70 -n 4"), ("big", "-t 13,7 -n 3"), ("big", "-t 66,34 -X -L -b 32,32"), ("rgb12", "-t 50,40 -I"),
    ("bigm16", "-t 96,80 -n 4"),
    # tests/test_gpu_modes.py: combinations, 9/7 with rates, 16-bit two layers
    ("rgb", "-M 5"), ("rgb", "-M 17"), ("rgb", "-M 20"), ("rgb", "-M 38"),
    ("rgb", "-I -M 5 -r 20"), ("rgb", "-I -M 63 -r 20"), ("rgb", "-I -M 38 -r 30,10"), ("m16", "-M 5 -r 10,3"),
    # tests/test_gpu_progression.py::CASES under each progression
    ("big", "-p RLCP -n 4 -b 16,16"), ("big", "-p RPCL -n 5 -b 32,32 -c [64,64],[32,32]"),
    ("big", "-p PCRL -n 4 -b 16,16 -c [32,32] -t 64,96 -X -L"), ("big", "-p CPRL -n 4 -b 32,32 -c [64,64] -r 30,10,3"),
    ("big", "-p PCRL -n 3 -b 16,16 -c [32,32] -I -r 40,20"), ("big", "-p RPCL -n 4 -b 32,32 -c [64,64] -r 40,10,2 -L"),
    ("big", "-n 4 -r 20,10 -P T0=0,0,1,3,3,RLCP/T0=0,0,3,4,3,LRCP"),
    # tests/test_gpu_tileparts.py::GEN
    ("big", "-t 64,64 -u L -r 30,10,1"), ("big", "-t 64,64 -u R -p RLCP"), ("big", "-t 64,64 -u R -p RPCL -X"),
    ("big", "-u C -p LRCP"),
    # tests/test_gpu_rc_tiles.py
    ("sq", "-I -r 40,20,10 -t 64,64"), ("sq", "-I -r 30,8 -t 64,32 -X -L"), ("bigm16", "-r 20,5,1 -t 32,64 -n 4"),
    ("big", "-I -r 12 -t 64,64 -b 32,32 -n 5"), ("rgb12", "-I -r 50,25,12,1 -t 64,16 -n 3"),
    # tests/test_gpu_sop_quality.py
    ("rgb", "-S"), ("rgb", "-E"), ("rgb", "-S -E -r 20,5"), ("rgb12", "-S -E -I -r 40,20,10"),
    ("sq", "-S -E -t 64,64 -X -L -r 10"), ("big", "-S -E -p RPCL -c [64,64]"),
    ("sqm16", "-S -E -M 64 -t 64,64 -X -L"), ("big", "-E -u R -t 64,64"),
    ("rgb", "-q 28,36,0"), ("rgb12", "-I -q 35,42"), ("big", "-q 30,38 -t 64,64 -X"), ("m16", "-q 45,60 -S -E"),
    # signed input through PGX
    ("p:m8", ""), ("p:m12", ""), ("p:m16", "-M 64"), ("p:m12", "-r 10,1"), ("p:m10", "-t 32,32 -n 3"),
    ("s:m8", ""), ("s:m16", ""), ("s:m16", "-M 64"), ("s:m8", "-t 32,32 -n 3"),
]

# (index into ENCODE by (image, flags), grk_decompress flags): the oracle's decode equals Grok's on
# Grok's stream (and on the oracle's own, the same bytes).  Windows are canvas coordinates.
DECODE = [
    (("rgb", ""), ""), (("rgb12", "-I"), ""), (("rgb16", "-I"), ""), (("rgb10", "-I -r 20,8"), ""),
    (("rgb", "-p RLCP -r 20,10,1 -c [32,32],[16,16] -S -E"), "-l 1"),
    (("rgb", "-p RLCP -r 20,10,1 -c [32,32],[16,16] -S -E"), "-l 2"),
    (("rgb", "-I -q 30,40,50"), "-l 2"), (("sq", "-I -r 40,20,10 -t 64,64"), "-l 1"),
    (("rgb", ""), "-r 1"), (("rgb", ""), "-r 2"), (("sq", "-I -r 40,20,10 -t 64,64"), "-r 1"),
    (("sq", "-I -r 40,20,10 -t 64,64"), "-r 2 -l 2"), (("rgb12", "-I"), "-r 2"),
    (("sq", "-M 64 -t 64,64 -X -L"), "-r 1"), (("m16", "-M 64"), "-r 2"), (("rgb", "-M 63"), "-r 1"),
    (("rgb", "-M 63 -r 20,5 -n 3"), "-l 1"), (("rgb", "-I -M 63 -r 20"), "-r 1"),
    (("rgb", ""), "-d 10,20,60,50"), (("big", "-t 64,64 -u R"), "-d 37,51,120,100"),
    (("sq", "-I -r 40,20,10 -t 64,64"), "-d 37,51,120,100"), (("sq", "-I -r 40,20,10 -t 64,64"), "-r 1 -d 37,51,120,100"),
    (("big", "-p PCRL -n 4 -b 16,16 -c [32,32] -t 64,96 -X -L"), "-d 70,60,150,130"),
    (("rgb12", "-I"), "-d 1,1,40,30"), (("sq", "-M 64 -t 64,64 -X -L"), "-r 2 -d 5,5,121,99"),
    (("big", "-t 64,64 -u R"), "-t 0"), (("big", "-t 64,64 -u R"), "-t 4"), (("sq", "-I -r 40,20,10 -t 64,64"), "-t 3"),
    (("big", "-t 100,70 -n 4"), "-t 3"), (("p:m12", ""), ""), (("p:m12", "-r 10,1"), "-l 1"), (("p:m16", "-M 64"), "-r 1"),
]


# What tests/golden/make_grok_fixtures.py records under tests/golden/grok/: every decode case, and
# these encode cases with Grok's plain decode, so that each option family and each decode option is
# pinned where no build of Grok exists (tests/test_grok_fixtures.py, tests/test_gpu_grok_live.py).
FIXTURE_ENCODE = [
    ("m8", ""), ("m10", ""), ("m16", ""), ("rgb", "-M 1"), ("rgb", "-M 2"), ("rgb", "-M 4"), ("rgb", "-M 8"),
    ("rgb", "-M 16"), ("rgb", "-M 32"), ("m16", "-M 63"), ("rgb", "-q 30,40"), ("rgb", "-u C"), ("rgb", "-p LRCP -r 30,10 -c [64,64] -S -E"), ("rgb", "-d 1,1 -t 13,7 -n 3"),
    ("rgb", "-d 65,33 -T 64,32 -t 32,32 -X -L -p RPCL"),
    ("sqm16", "-M 64 -t 32,32 -X -L"),
    ("rgb", "-b 1024,4"), ("thin", "-n 6"), ("one", ""),
    ("rgb", "-I -M 38 -r 30,10"),
    ("big", "-n 4 -r 20,10 -P T0=0,0,1,3,3,RLCP/T0=0,0,3,4,3,LRCP"), ("big", "-t 64,64 -u L -r 30,10,1"),
    ("bigm16", "-r 20,5,1 -t 32,64 -n 4"), ("rgb12", "-S -E -I -r 40,20,10"), ("rgb", "-q 28,36,0"),
    ("p:m10", "-t 32,32 -n 3"), ("s:m8", ""),
]
# decode cases that stay live only: their stream is recorded with another decode option already
FIXTURE_LEAVES_OUT = [
    (("big", "-t 64,64 -u R"), "-t 0"), (("big", "-t 64,64 -u R"), "-d 37,51,120,100"), (("rgb16", "-I"), ""), (("rgb12", "-I"), ""),
    (("sq", "-M 64 -t 64,64 -X -L"), "-r 1"), (("rgb", "-p RLCP -r 20,10,1 -c [32,32],[16,16] -S -E"), "-l 2"),
]
FIXTURES = [(c, "") for c in FIXTURE_ENCODE if (c, "") not in DECODE] + [d for d in DECODE if d not in FIXTURE_LEAVES_OUT]
assert all(c in ENCODE for c, _ in FIXTURES)


def fixture_name(i):
    return "%02d_%s" % (i, "".join(ch if ch.isalnum() else "_" for ch in decode_id(FIXTURES[i])).strip("_"))


class GrokFixture:
    """One recording of tests/golden/grok/: Grok's codestream for (image key, flags) and Grok's
    decode of it under dflags."""
    def __init__(self, path):
        import json
        z = np.load(path)
        meta = json.loads(str(z["meta"]))
        self.name = meta["name"]
        self.key, self.flags, self.dflags = meta["key"], meta["flags"], meta["dflags"]
        kind, k = (self.key[0], self.key[2:]) if self.key[1:2] == ":" else ("", self.key)
        assert tuple(meta["synth"]) == IMAGES[k], "the image arguments changed since the recording"
        self.cs = z["cs"].tobytes()
        # Grok's decode; where it was the image itself the recording says so instead of holding it
        self.grok_decoded = (image(self.key)[0] if meta["decoded"] == "source" else z["grok_decoded"]).astype(np.int32)
        self.irreversible = "-I" in self.flags.split()

    def __repr__(self):
        return self.name


def load_fixtures():
    import glob
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grok")
    return [GrokFixture(p) for p in sorted(glob.glob(os.path.join(here, "*.npz")))]

# Streams of tests/test_coc.py and tests/tile_coding.py that mix the HT and the Part-1 block coder
# by component or by tile: Grok's decoder takes one coder for the whole stream (R-BUG-16,
# tests/test_grok_defects.py); OpenJPEG 2.5.4 and the oracle decode them.
MIXED_CODERS_COC = ["ht_and_part1", "part1_under_ht"]
MIXED_CODERS_TILE = ["ht_tile", "part1_coc_under_ht", "part1_tile_under_ht"]


def case_id(c):
    return ("%s %s" % (c[0], c[1])).strip().replace(" ", "_")


def decode_id(d):
    return (case_id(d[0]) + "__" + d[1]).replace(" ", "_")


def grok_encode(key, flags):
    import grok_ref
    img, _, bits, signed = image(key)
    return grok_ref.compress(img, bits, flags, signed=signed)


def oracle_encode(key, flags):
    import oracle as O
    _, seen, bits, signed = image(key)
    return O.encode(seen, bits, signed=signed, **parse_flags(flags))


def parse_decode(dflags):
    """-> dict(layers, reduce, window, tile) of grk_decompress flags."""
    t = dflags.split()
    g = lambda f: t[t.index(f) + 1] if f in t else None
    return dict(layers=int(g("-l") or 0), reduce=int(g("-r") or 0),
                window=tuple(int(v) for v in g("-d").split(",")) if g("-d") else None,
                tile=int(g("-t")) if g("-t") is not None else None)


def tile_window(shape_hw, eflags, n):
    """Tile n's rectangle, relative to the image origin, from the encode flags."""
    kw = parse_flags(eflags)
    h, w = shape_hw
    tw, th = kw["tiles"]
    tx0, ty0 = kw.get("tile_origin") or (0, 0)
    ox, oy = kw.get("origin") or kw.get("tile_origin") or (0, 0)
    ntx = -(-(ox + w - tx0) // tw)
    p, q = n % ntx, n // ntx
    x0, y0 = max(tx0 + p * tw, ox), max(ty0 + q * th, oy)
    x1, y1 = min(tx0 + (p + 1) * tw, ox + w), min(ty0 + (q + 1) * th, oy + h)
    return x0 - ox, y0 - oy, x1 - ox, y1 - oy


def oracle_decode(cs, dflags, eflags=""):
    """The oracle's decode of cs as grk_decompress <dflags> returns it: layers and reduction
    applied, a window or a tile cropped out of the whole decode on the reduced canvas (every edge
    ceil(x / 2^r)), a window under the partial-tile rule it selects."""
    import oracle as O
    d = parse_decode(dflags)
    O.set_decode_layers(d["layers"])
    O.set_decode_reduce(d["reduce"])
    try:
        dec, _ = O.decode(cs, partial=d["window"] is not None)
    finally:
        O.set_decode_layers(0)
        O.set_decode_reduce(0)
    win = d["window"]
    if d["tile"] is not None:
        assert d["reduce"] == 0, "tile crops are taken at full resolution"
        win = tile_window(dec.shape[1:], eflags, d["tile"])
    if win is None:
        return dec
    cd = lambda v: -(-v >> d["reduce"])
    return dec[:, cd(win[1]):cd(win[3]), cd(win[0]):cd(win[2])]
