"""The engine decodes streams written by OpenJPEG's encoder (tests/golden/opj: another encoder's
pass terminations, truncation points, layer splits, step sizes, SOP / EPH, RGN, mode switches, tile
parts, subsampled components) to the samples OpenJPEG's own decoder recorded for them.

Fixtures only: neither Pillow nor libopenjp2 is imported.  Bars: 5/3 streams equal the recording
exactly, full, layer-limited, reduced, windowed and packed.  9/7 streams stay within
TOL_97_MAXABS (1, tests/test_gpu_parity.py) of the oracle's decode, which is the recording itself
(the corpus bound measured at generation is 0, asserted again here and in tests/test_opj_streams.py).
Every stream of the corpus is decoded; none is refused.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import opj_cases as OC
import oracle as O
from conftest import FIXTURES, ROOT
from test_gpu_parity import TOL_97_MAXABS

pytestmark = pytest.mark.gpu

FX = OC.load()
IDS = [f.name for f in FX]
MARKED = [f for f in FX if f.limited]
LIMITS = (("l1", dict(layers=1)), ("r1", dict(reduce=1)), ("r2", dict(reduce=2)))
# reversible streams of several tiles, with and without canvas offsets (window decode)
WINDOWED = [f for f in FX if f.tiled and f.lossless and not f.subsampled]
PACKED = [f for f in FX if not f.subsampled and (f.expect["comps"], f.expect["prec"]) in ((3, 8), (1, 16))]
# decoder splits: streams with layers, mode switches or an ROI
SPLIT = [f.name for f in FX if f.layered or f.expect["mode"] or f.meta["fields"].get("roi")]


@pytest.fixture(scope="module")
def eng():
    import grok_amd as G
    e = G.Engine(0)
    yield e
    e.close()


_want_cache = {}


def _want(f, tag=None, **limits):
    """(planes, tolerance) a decode of f is held to: the recording, exactly, for 5/3; for 9/7 the
    oracle's decode (checked to be the recording) within TOL_97_MAXABS."""
    rec = f.limited[tag] if tag else f.planes
    if f.lossless:
        return rec, 0
    if (f.name, tag) not in _want_cache:
        O.set_decode_reduce(limits.get("reduce", 0))
        O.set_decode_layers(limits.get("layers", 0))
        try:
            ora = OC.planes_of(O.decode(f.cs)[0])
        finally:
            O.set_decode_reduce(0)
            O.set_decode_layers(0)
        assert OC.maxabs(ora, rec) == f.meta["oracle_maxabs_97"] == 0
        _want_cache[(f.name, tag)] = ora
    return _want_cache[(f.name, tag)], TOL_97_MAXABS


def _check(got, f, tag=None, **limits):
    want, tol = _want(f, tag, **limits)
    d = OC.maxabs(got, want)
    assert d is not None, ([np.shape(p) for p in got], [p.shape for p in want])
    assert d <= tol, (f.name, tag, d)


@pytest.mark.parametrize("f", FX, ids=IDS)
def test_full_decode(eng, f):
    _check(eng.decode(f.cs), f)


@pytest.mark.parametrize("f", FX, ids=IDS)
def test_device_resident_stream(eng, f):
    """The codestream in device memory: the engine reads the headers back itself and takes its
    other packet-header path."""
    import torch
    dev = torch.frombuffer(bytearray(f.cs), dtype=torch.uint8).cuda()
    _check(eng.decode(dev, length=len(f.cs)), f)


@pytest.mark.parametrize("f", MARKED, ids=[f.name for f in MARKED])
def test_limited_decodes(eng, f):
    """cp_layer 1, cp_reduce 1 and 2 against OpenJPEG's own limited decodes."""
    try:
        for tag, kw in LIMITS:
            eng.set_decode_layers(kw.get("layers", 0))
            eng.set_decode_reduce(kw.get("reduce", 0))
            _check(eng.decode(f.cs), f, tag, **kw)
    finally:
        eng.set_decode_layers(0)
        eng.set_decode_reduce(0)


def _windows(f):
    """Inside one tile, across a tile corner, and up to the image's last row and column
    (image coordinates, as decode_window takes them)."""
    e = f.expect
    tw, th = e["tiles"]
    tx0, ty0 = e["tile_origin"]
    # the first interior tile corner on the canvas, in image coordinates
    cx = tx0 + tw * (1 + (e["x0"] - tx0) // tw) - e["x0"]
    cy = ty0 + th * (1 + (e["y0"] - ty0) // th) - e["y0"]
    assert 5 < cx < e["w"] - 5 and 5 < cy < e["h"] - 5
    return [(cx + 2, cy + 3, cx + min(tw, e["w"] - cx) - 1, cy + min(th, e["h"] - cy) - 2),
            (cx - 5, cy - 4, cx + 5, cy + 3),
            (e["w"] - 23, e["h"] - 17, e["w"], e["h"])]


@pytest.mark.parametrize("f", WINDOWED, ids=[f.name for f in WINDOWED])
def test_windows(eng, f):
    """decode_window is the crop of the recorded full decode (geometry on which the oracle's
    window rule gives the crop too: none of these tile-components has the single odd sample row
    of DESIGN.md §7)."""
    full = np.stack(f.planes)
    for x0, y0, x1, y1 in _windows(f):
        assert 0 <= x0 < x1 <= f.expect["w"] and 0 <= y0 < y1 <= f.expect["h"]
        got = eng.decode_window(f.cs, (x0, y0, x1, y1))
        assert np.array_equal(got, full[:, y0:y1, x0:x1]), (f.name, (x0, y0, x1, y1))


@pytest.mark.parametrize("f", PACKED, ids=[f.name for f in PACKED])
def test_packed_pixels(eng, f):
    """decode_pixels: the recorded planes interleaved (H, W, C), 8-bit RGB and 16-bit grey."""
    want, tol = _want(f)
    got = eng.decode_pixels(f.cs, sample_bytes=f.expect["prec"] // 8)
    assert got.dtype.itemsize == f.expect["prec"] // 8 and got.shape == np.stack(want).shape[1:] + (len(want),)
    assert int(np.abs(got.astype(np.int64) - np.stack(want).transpose(1, 2, 0)).max()) <= tol


CHILD = r'''
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import grok_amd as G, opj_cases as OC
names = sys.argv[1].split(",")
fx = {f.name: f for f in OC.load()}
e = G.Engine(0)
solo = []
for n in names:
    f = fx[n]
    d = OC.maxabs(e.decode(f.cs), f.planes)
    assert d is not None and d <= (0 if f.lossless else %d), (n, d)
    solo.append(int(e.timings().t1_solo_blocks))
e.close()
print("ok", *solo)
''' % (ROOT, os.path.join(ROOT, "tests"), TOL_97_MAXABS)


@pytest.mark.parametrize("solo", ["0", "5", "100000"])
def test_decoder_splits(solo):
    """GK_T1DEC_SOLO (read once per process) forces the split between solo waves and the
    lane-parallel decoder: none, a few, every block.  One fresh process per value decodes the
    layered, mode-switch and ROI streams and stops at its first failure.  (9/7 within
    TOL_97_MAXABS of the recording, which is the oracle's decode.)"""
    assert len(SPLIT) >= 20
    env = dict(os.environ, GK_T1DEC_SOLO=solo)
    r = subprocess.run([sys.executable, "-c", CHILD, ",".join(SPLIT)], capture_output=True, text=True, timeout=120,
                       env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    # the switch took effect: solo blocks of the last lane-parallel launch after each decode
    # (the mode-switch kernel has no solo waves and leaves the count as it was)
    counts = [int(v) for v in r.stdout.split()[1:]]
    assert len(counts) == len(SPLIT)
    assert max(counts) == 0 if solo == "0" else max(counts) == 5 if solo == "5" else max(counts) > 5


HISTORY = ["rgb8_tiles_offset", "yuv420", "rgb8_layers_mode63_97", "rgb12_cinema4k", "mono8_layers20"]


@pytest.mark.parametrize("name", HISTORY)
def test_engine_history(eng, name):
    """A plan built from another encoder's header leaves nothing behind: an OpenJPEG stream, a
    Grok stream, then the OpenJPEG stream again on one engine give the same samples as alone."""
    f = next(x for x in FX if x.name == name)
    grok = next(x for x in FIXTURES if x.name == "rgb8_tiles")
    first = OC.planes_of(eng.decode(f.cs))
    _check(first, f)
    assert np.array_equal(eng.decode(grok.cs), grok.grok_decoded)
    again = OC.planes_of(eng.decode(f.cs))
    assert OC.maxabs(again, first) == 0
