"""The HIP engine against Grok 9.2.0 itself.

Against the recordings of tests/golden/grok/ (no binary needed): Engine.encode gives Grok's bytes
from host planes and from device planes; Engine.decode gives Grok's decode under the recorded
reduce / layers / window / tile, exactly for 5/3 and within TOL_97_MAXABS for 9/7.

Against the live binaries (tests/grok_ref.py; grk_decompress runs as a CPU child process on the
engine's output), on streams only the engine writes: shaped ROI, HT 9/7 at chosen steps
(set_encode_quant), transcodes, RGB to sYCC encodes, JP2 colour boxes.  HT with ROI stays out
(DESIGN.md R-BUG-9).  Without binaries that start here, this group skips with the reason.

Every figure asserted on is printed first (pytest -s shows them).
"""
import numpy as np
import pytest
import torch

import grok_amd as G
import grok_cases as C
import grok_ref
import htq_ref
import icc_profiles as I
import jp2_boxes as J
from conftest import parse_flags
from test_gpu_grok_known import gk_params
from test_gpu_parity import TOL_97_MAXABS

pytestmark = pytest.mark.gpu

FX = C.load_fixtures()


@pytest.fixture(scope="module")
def eng():
    e = G.Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _clear(eng):
    yield
    eng.set_encode_roi()
    eng.set_encode_quant()
    eng.set_encode_convert(None)
    eng.set_decode_display()
    eng.set_decode_layers(0)
    eng.set_decode_reduce(0)


@pytest.fixture
def grok():
    grok_ref.need()
    return grok_ref


def _maxabs(a, b):
    assert np.shape(a) == np.shape(b), (np.shape(a), np.shape(b))
    return int(np.abs(np.asarray(a, np.int64) - np.asarray(b)).max())


def _params(flags):
    kw = parse_flags(flags)
    origin = kw.pop("origin", None)
    return gk_params(kw), origin


# ------------------------------------------------------------------------- the recordings
def test_recordings_present():
    assert len(FX) == len(C.FIXTURES) >= 50


@pytest.mark.parametrize("fx", FX, ids=[f.name for f in FX])
def test_engine_encode_equals_recorded_grok(eng, fx):
    _, seen, bits, signed = C.image(fx.key)
    p, origin = _params(fx.flags)
    assert eng.encode(seen, bits, signed=signed, params=p, origin=origin) == fx.cs, "host planes"
    dev = torch.from_numpy(np.ascontiguousarray(seen)).cuda()
    assert eng.encode(dev, bits, signed=signed, params=p, origin=origin) == fx.cs, "device planes"


@pytest.mark.parametrize("fx", FX, ids=[f.name for f in FX])
def test_engine_decode_equals_recorded_grok(eng, fx):
    d = C.parse_decode(fx.dflags)
    eng.set_decode_layers(d["layers"])
    eng.set_decode_reduce(d["reduce"])
    win = d["window"]
    if d["tile"] is not None:
        h, w = C.image(fx.key)[0].shape[1:]
        win = C.tile_window((h, w), fx.flags, d["tile"])
    got = eng.decode_window(fx.cs, win) if win else eng.decode(fx.cs)
    diff = _maxabs(got, fx.grok_decoded)
    print("%s: max |engine - Grok| = %d" % (fx.name, diff))
    assert diff <= (TOL_97_MAXABS if fx.irreversible else 0)


# ------------------------------------------------------------------------- the live binaries
def _rgb(seed=5, h=67, w=93, bits=8):
    return C.synth_image(h, w, 3, bits, seed).astype(np.int32)


REGION = [(20, 12, 52, 40)]


def _strokes(h, w):
    m = np.zeros((h, w), np.uint8)
    for i in range(h):
        m[i, i * (w - 1) // (h - 1)] = 255
    return m


@pytest.mark.parametrize("shape", ["rects", "mask"])
@pytest.mark.parametrize("irr", [False, True], ids=["53", "97"])
def test_grok_decodes_shaped_roi(eng, grok, shape, irr):
    """Part-1 maxshift from rectangles or a mask: Grok's decode of the engine's stream equals the
    engine's decode (5/3 exactly and lossless; 9/7 within the bar)."""
    img = _rgb()
    if shape == "rects":
        eng.set_encode_roi(rects=REGION)
    else:
        eng.set_encode_roi(mask=_strokes(67, 93), rects=[(0, 60, 6, 67)])
    cs = eng.encode(img, 8, params=G.default_params(irreversible=irr, numresolution=3 if irr else 4))
    assert b"\xff\x5e" in cs
    theirs, mine = grok.decompress(cs), eng.decode(cs)
    diff = _maxabs(theirs, mine)
    print("shaped ROI %s %s: max |Grok - engine| = %d" % (shape, "9/7" if irr else "5/3", diff))
    if irr:
        assert diff <= TOL_97_MAXABS
    else:
        assert diff == 0
        np.testing.assert_array_equal(theirs, img)


@pytest.mark.parametrize("irr", [False, True], ids=["53", "97"])
def test_grok_sees_the_region_first(eng, grok, irr):
    """At the layer cut of tests/test_gpu_roi_region.py (two layers, the first a fraction of the
    stream), Grok's layer-1 decode is final inside the region too: the source for 5/3, Grok's own
    full decode for 9/7; outside it is not."""
    img = _rgb(7, 96, 96)
    x0, y0, x1, y1 = 32, 32, 56, 56
    eng.set_encode_roi(rects=[(x0, y0, x1, y1)])
    p = G.default_params(irreversible=irr, numresolution=3, layer_rate=[8.0 if irr else 4.0, 0.0])
    cs = eng.encode(img, 8, params=p)
    first, full = grok.decompress(cs, "-l 1"), grok.decompress(cs)
    want = full if irr else img
    if not irr:
        np.testing.assert_array_equal(full, img)
    inside = int((first != want)[:, y0:y1, x0:x1].sum())
    print("region at layer 1 in Grok (%s): %d samples differ inside, %d in all" % ("9/7" if irr else "5/3", inside,
                                                                                    int((first != want).sum())))
    assert inside == 0
    assert (first != want).any()
    eng.set_decode_layers(1)
    diff = _maxabs(first, eng.decode(cs))
    print("layer 1: max |Grok - engine| = %d" % diff)
    assert diff <= (TOL_97_MAXABS if irr else 0)


@pytest.mark.parametrize("notch", [0, 8, 24])
@pytest.mark.parametrize("name", ["rgb", "mono12_tiles"])
def test_grok_decodes_chosen_steps(eng, grok, name, notch):
    """HT 9/7 at ladder notches (set_encode_quant): Grok rebuilds every index where the engine
    does, the centre of its bin, so the two decodes agree within the 9/7 bar."""
    if name == "rgb":
        img, bits, kw = _rgb(), 8, dict(numresolution=4)
    else:
        img, bits, kw = C.synth_image(90, 77, 1, 12, 9).astype(np.int32), 12, dict(numresolution=3, tiles=(64, 64))
    eng.set_encode_quant(step=htq_ref.ladder_step(bits, False, notch))
    cs = eng.encode(img, bits, params=G.default_params(cblk_sty=0x40, irreversible=True, **kw))
    theirs, mine = grok.decompress(cs), eng.decode(cs)
    diff = _maxabs(theirs, mine)
    print("set_encode_quant %s notch %d: %d bytes, max |Grok - engine| = %d" % (name, notch, len(cs), diff))
    assert diff <= TOL_97_MAXABS


TRANSCODES = [("rgb", ""), ("rgb", "-I"), ("m16", ""), ("sq", "-I -t 64,64 -n 4"), ("rgb12", "-I")]


@pytest.mark.parametrize("key,flags", TRANSCODES, ids=[C.case_id(c) for c in TRANSCODES])
def test_grok_decodes_transcodes(eng, grok, key, flags):
    """Part-1 -> HT -> Part-1 at the block-coder level: Grok decodes each transcoded stream to the
    samples it decodes the source stream to, exactly, 5/3 and 9/7."""
    _, seen, bits, signed = C.image(key)
    p, origin = _params(flags)
    src = eng.encode(seen, bits, params=p, origin=origin)
    ht = eng.transcode(src, "ht")
    back = eng.transcode(ht, "part1")
    assert ht != src and back != ht
    want = grok.decompress(src)
    np.testing.assert_array_equal(grok.decompress(ht), want)
    np.testing.assert_array_equal(grok.decompress(back), want)


@pytest.mark.parametrize("chroma", [(1, 1), (2, 1), (2, 2)], ids=["444", "422", "420"])
def test_grok_displays_sycc_encodes(eng, grok, chroma):
    """RGB in, sYCC .jp2 out: what Grok's CLI shows for the file (RGB) is what Engine.decode returns
    under set_decode_display(rgb=True, upsample=True)."""
    img = _rgb(11, 66, 92)
    eng.set_encode_convert("sycc", chroma)
    f = eng.encode(img, 8, params=G.default_params(jp2=True, numresolution=4))
    eng.set_encode_convert(None)
    assert f[4:8] == b"jP  "
    theirs = grok.decompress(f, "-u")
    eng.set_decode_display(rgb=True, upsample=True)
    mine = eng.decode(f)
    diff = _maxabs(theirs, mine)
    print("sYCC %s: max |Grok CLI - engine display| = %d" % (chroma, diff))
    assert diff == 0


@pytest.mark.parametrize("name", ["c1_clamp200", "c6_cdef_only"])
def test_grok_applies_palette_and_cdef(eng, grok, name):
    c = J.cases()[name]
    theirs = grok.decompress(c.file)
    mine = eng.decode(c.file)
    np.testing.assert_array_equal(mine, c.want)
    np.testing.assert_array_equal(theirs, mine)


def test_grok_converts_icc_8bit(eng, grok):
    """An 8-bit RGB .jp2 with an ICC profile (colr METH 2): Grok's CLI converts to sRGB for an
    output that cannot embed the profile, and so does set_decode_display(icc=True), within the one
    level tests/test_icc.py grants the restatement against lcms2.  (Above 8 bits: R-BUG-12.)"""
    img = _rgb(13, 40, 52)
    cs = eng.encode(img, 8, params=G.default_params(numresolution=3, mct=False))
    f = I.jp2(cs, 40, 52, 3, 8, I.colr_profile(I.accepted()["adobe_g22"][0]))
    theirs = grok.decompress(f)
    eng.set_decode_display(icc=True)
    mine = eng.decode(f)
    diff = _maxabs(theirs, mine)
    print("ICC 8-bit: max |Grok CLI - engine| = %d; changed by the profile: %d samples" % (diff, int((mine != img).sum())))
    assert (mine != img).any()
    assert diff <= 1
