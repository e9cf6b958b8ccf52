"""Display stage without a GPU: the restatement (tests/display_ref.py) against answers worked out
by hand from the C, and grok_amd.probe_display, which resolves from the header alone what a
decode under Engine.set_decode_display returns or why it is refused."""
import numpy as np
import pytest

import grok_amd as G
import oracle as O
import jp2_boxes as J
import display_ref as R
import display_cases as C


def _stream(w, h, sub, prec=8, origin=(0, 0), signed=False, seed=3):
    planes = C.random_planes(w, h, sub, prec, origin, seed, signed)
    kw = dict(mct=False, numres=C.numres_for(w, h, sub))
    if origin != (0, 0):
        kw["origin"] = origin
    if all(d == (1, 1) for d in sub):
        return O.encode(np.stack(planes), prec, signed=signed, **kw)
    return O.encode(planes, prec, signed=signed, size=(w, h), subsampling=sub, **kw)


# ---------------------------------------------------------------- 1. known answers
def test_sycc_known_answer():
    # 8 bits, (y, cb, cr) = (100, 200, 50): cb - 128 = 72, cr - 128 = -78
    # r = 100 + (int)(1.402 * -78 = -109.356 -> -109) = -9 -> 0
    # g = 100 - (int)(0.344 * 72 + 0.714 * -78 = 24.768 - 55.692 = -30.924 -> -30) = 130
    # b = 100 + (int)(1.772 * 72 = 127.584 -> 127) = 227
    assert [int(v) for v in R.sycc_to_rgb(128, 255, 100, 200, 50)] == [0, 130, 227]


def test_esycc_known_answer():
    # 8 bits unsigned, (y, cb, cr) = (120, 90, 200): cb = -38, cr = 72
    # r = (int)(120 + 0.0013984 + 100.94328 + 0.5 = 221.4446784) = 221
    # g = (int)(120.036 + 13.07675 - 51.4161216 + 0.5 = 82.1966284) = 82
    # b = (int)(119.97876 - 67.33752 - 0.000576 + 0.5 = 53.140664) = 53
    one = lambda v: np.array([[v]], np.int32)
    got = R.color_esycc_to_rgb([one(120), one(90), one(200)], [(1, 1, 8, 0)] * 3)
    assert [int(v[0, 0]) for v in got] == [221, 82, 53]
    # signed chroma (the components then all signed): cb / cr are taken as they are
    got = R.color_esycc_to_rgb([one(120), one(-38), one(72)], [(1, 1, 8, 1)] * 3)
    assert [int(v[0, 0]) for v in got] == [221, 82, 53]


def test_cmyk_known_answer():
    # 16 bits, (c, m, y, k) = (10000, 30000, 65535, 20000), s = 1 / 65535
    # C = 1 - 0.15259022 = 0.84740978, M = 1 - 0.45777066 = 0.54222934, Y = 1 - 1 = 0 (or -6e-8),
    # K = 1 - 0.30518044 = 0.69481956
    # R = (int)(255 * 0.84740978 * 0.69481956 = 150.143) = 150, G = (int)(96.072) = 96, B = (int)(-0.0) = 0
    one = lambda v: np.array([[v]], np.int32)
    got = R.color_cmyk_to_rgb([one(10000), one(30000), one(65535), one(20000)], [(1, 1, 16, 0)] * 4)
    assert [int(v[0, 0]) for v in got] == [150, 96, 0]


def test_chroma_selection_small():
    # 4:2:2, odd origin, width 4: column 0 alone with (0, 0), then a pair, then the unpaired last column
    cb = np.array([[10, 20]]); cr = np.array([[30, 40]])
    sb, sr = R.sycc422_select(4, 1, cb, cr, 1)
    assert sb.tolist() == [[0, 10, 10, 20]] and sr.tolist() == [[0, 30, 30, 40]]
    # 4:2:0, origin (1, 1), 4 x 4: row 0 alone; rows 1-2 a pair whose first row starts with (0, 0)
    # and whose second row starts with the pair's first chroma sample (:316-320); row 3 unpaired,
    # its columns pairing from 0 (:344-357)
    cb = np.array([[1, 2], [3, 4]]); cr = cb + 10
    sb, _ = R.sycc420_select(4, 4, cb, cr, 1, 1)
    assert sb.tolist() == [[0, 0, 0, 0], [0, 1, 1, 2], [1, 1, 1, 2], [3, 3, 4, 4]]
    # origin (0, 0): plain 2 x 2 blocks
    sb, _ = R.sycc420_select(4, 4, cb, cr, 0, 0)
    assert sb.tolist() == [[1, 1, 2, 2], [1, 1, 2, 2], [3, 3, 4, 4], [3, 3, 4, 4]]
    # origin (1, 0), 3 x 2 (the documented rule where the C's loops leave the planes)
    sb, _ = R.sycc420_select(3, 2, np.array([[7]]), np.array([[8]]), 1, 0)
    assert sb.tolist() == [[0, 7, 7], [0, 7, 7]]


def test_upsample_restatement():
    src = np.array([[1, 2], [3, 4]])
    # bounds (1, 1)-(4, 4), dx = dy = 2: xoff = yoff = 1
    got = R.upsample_component(src, 2, 2, 1, 1, 4, 4)
    assert got.tolist() == [[0, 0, 0], [0, 1, 1], [0, 1, 1]]
    got = R.upsample_component(src, 2, 2, 0, 0, 3, 3)
    assert got.tolist() == [[1, 1, 2], [1, 1, 2], [3, 3, 4]]


# ---------------------------------------------------------------- 2. probe_display
W, H = 34, 18


@pytest.mark.parametrize("origin", [(0, 0), (1, 1)])
@pytest.mark.parametrize("sub", [C.S444, C.S422, C.S420], ids=["444", "422", "420"])
def test_probe_sycc(sub, origin):
    cs = _stream(W, H, sub, origin=origin)
    f = C.wrap(cs, W, H, 3, 8, C.SYCC)
    d = G.probe_display(f, rgb=True)
    assert d.shapes == [(H, W)] * 3 and d.channels == [(1, 1)] * 3 and d.precisions == [8] * 3
    assert (d.colour_space, d.converted, d.upsampled) == (R.CS_SRGB, True, False)
    assert (d.info.numcomps, d.info.prec, d.info.w, d.info.h, d.info.x0, d.info.y0) == (3, 8, W, H) + origin
    # without the flag: the components, still sYCC
    d = G.probe_display(f)
    assert d.channels == sub and (d.colour_space, d.converted, d.upsampled) == (R.CS_SYCC, False, False)
    assert d.shapes == [C.comp_shape(W, H, dx, dy, origin) for dx, dy in sub]


def test_probe_raw_420_is_taken_as_sycc():
    cs = _stream(W, H, C.S420)
    d = G.probe_display(cs, rgb=True)
    assert (d.colour_space, d.converted, d.shapes) == (R.CS_SRGB, True, [(H, W)] * 3)
    assert G.probe_display(cs).colour_space == R.CS_UNKNOWN
    # ... and so is a file that calls itself sRGB
    d = G.probe_display(C.wrap(cs, W, H, 3, 8, C.SRGB), rgb=True)
    assert (d.colour_space, d.converted) == (R.CS_SRGB, True)


def test_probe_two_components_are_grey_and_untouched():
    cs = _stream(W, H, [(1, 1), (1, 1)])
    d = G.probe_display(cs, rgb=True)
    assert (d.colour_space, d.converted, d.upsampled, d.shapes, d.precisions) == (R.CS_GRAY, False, False, [(H, W)] * 2, [8, 8])


def test_probe_sycc_dx4_stays_unconverted():
    sub = [(1, 1), (4, 1), (4, 1)]
    f = C.wrap(_stream(W, H, sub), W, H, 3, 8, C.SYCC)
    d = G.probe_display(f, rgb=True)
    assert (d.colour_space, d.converted, d.upsampled, d.channels) == (R.CS_SYCC, False, False, sub)
    d = G.probe_display(f, rgb=True, upsample=True)
    assert (d.colour_space, d.converted, d.upsampled, d.shapes) == (R.CS_SYCC, False, True, [(H, W)] * 3)


def test_probe_cmyk16():
    f = C.wrap(_stream(W, H, [(1, 1)] * 4, prec=16), W, H, 4, 16, C.CMYK)
    d = G.probe_display(f, rgb=True)
    assert (d.colour_space, d.converted, d.shapes, d.precisions) == (R.CS_SRGB, True, [(H, W)] * 3, [8, 8, 8])
    assert (d.info.numcomps, d.info.prec) == (3, 8) and d.colour.num_comps == 4 and d.colour.num_channels == 3
    d = G.probe_display(f)
    assert (d.colour_space, d.precisions) == (R.CS_CMYK, [16] * 4)


def test_probe_esycc():
    cs = _stream(W, H, C.S444, prec=12)
    d = G.probe_display(C.wrap(cs, W, H, 3, 12, C.EYCC), rgb=True)
    assert (d.colour_space, d.converted, d.precisions) == (R.CS_SRGB, True, [12] * 3)
    # all_components_sanity_check: another precision in component 1 leaves the planes as they are
    d = G.probe_display(C.wrap(C.set_ssiz(cs, 1, 10), W, H, 3, 12, C.EYCC), rgb=True)
    assert (d.colour_space, d.converted, d.precisions) == (R.CS_EYCC, False, [12, 10, 12])
    # ... and so does a sign that differs
    d = G.probe_display(C.wrap(C.set_ssiz(cs, 2, 12, signed=True), W, H, 3, 12, C.EYCC), rgb=True)
    assert (d.colour_space, d.converted, d.signed) == (R.CS_EYCC, False, [False, False, True])
    # signed throughout: the supported signed case
    cs = _stream(W, H, C.S444, prec=8, signed=True)
    d = G.probe_display(C.wrap(cs, W, H, 3, 8, C.EYCC, signed=True), rgb=True)
    assert (d.colour_space, d.converted, d.signed) == (R.CS_SRGB, True, [True] * 3)


@pytest.mark.parametrize("origin", [(0, 0), (1, 1)])
def test_probe_upsample_dx3_dy2(origin):
    sub = [(1, 1), (3, 2), (3, 2)]
    cs = _stream(37, 19, sub, origin=origin)
    d = G.probe_display(cs, upsample=True)
    assert (d.shapes, d.channels, d.converted, d.upsampled) == ([(19, 37)] * 3, [(1, 1)] * 3, False, True)
    assert d.colour_space == R.CS_UNKNOWN
    d = G.probe_display(cs, rgb=True)   # no sYCC pattern, no upsampling asked for
    assert (d.channels, d.converted, d.upsampled) == (sub, False, False)


def test_probe_reduce():
    f = C.wrap(_stream(64, 48, C.S420), 64, 48, 3, 8, C.SYCC)
    d = G.probe_display(f, rgb=True, reduce=1)
    assert (d.shapes, d.converted) == ([(24, 32)] * 3, True)


# ---------------------------------------------------------------- 3. refusals, and flags 0
def _refused(data, needle, **kw):
    with pytest.raises(ValueError) as e:
        G.probe_display(data, **kw)
    assert needle in str(e.value), str(e.value)


def test_refusals_name_their_cause():
    s3 = _stream(W, H, C.S444)
    s4 = _stream(W, H, [(1, 1)] * 4)
    _refused(C.wrap(s4, W, H, 4, 8, C.SYCC), "sYCC: number of components 4", rgb=True)
    _refused(C.wrap(s4, W, H, 4, 8, C.EYCC), "e-sYCC: number of components 4", rgb=True)
    _refused(C.wrap(s3, W, H, 3, 8, C.CMYK), "CMYK: number of components 3", rgb=True)
    # signed components into the sYCC and CMYK conversions
    sg3 = _stream(W, H, C.S444, signed=True)
    _refused(C.wrap(sg3, W, H, 3, 8, C.SYCC, signed=True), "signed", rgb=True)
    sg4 = _stream(W, H, [(1, 1)] * 4, signed=True)
    _refused(C.wrap(sg4, W, H, 4, 8, C.CMYK, signed=True), "signed", rgb=True)
    # upsampling at a reduced resolution
    _refused(_stream(W, H, C.S420), "reduced resolution", upsample=True, reduce=1)
    # a reduction under which the chroma planes no longer pair with the luma plane:
    # canvas [2, 35) halves to luma 17 wide (9 chroma needed), chroma [1, 18) to 8
    _refused(_stream(33, 18, C.S420, origin=(2, 0)), "do not pair", rgb=True, reduce=1)
    assert G.probe_display(_stream(33, 18, C.S420, origin=(2, 0)), rgb=True).converted
    # 4:2:0, odd origin, odd width, even height: the C's last-row loop reads past the chroma row
    _refused(_stream(33, 18, C.S420, origin=(1, 1)), "last-row", rgb=True)
    # e-sYCC / CMYK components of different sizes
    mixed = _stream(W, H, [(1, 1), (1, 1), (2, 2)])
    _refused(C.wrap(mixed, W, H, 3, 8, C.EYCC), "different sizes", rgb=True)
    # a channel definition on a file that would be converted
    f = C.wrap(s3, W, H, 3, 8, C.SYCC, extra=[J.cdef([(0, 0, 2), (1, 0, 1), (2, 0, 3)])])
    _refused(f, "channel definition", rgb=True)
    assert G.probe_display(f).channels == [(1, 1)] * 3   # (flags 0: as before)


def test_flags_zero_report_what_the_probes_report():
    files = [c.file for c in J.cases().values()]
    files += [_stream(W, H, C.S420, origin=(1, 1)), C.wrap(_stream(W, H, C.S422), W, H, 3, 8, C.SYCC),
              C.wrap(_stream(W, H, [(1, 1)] * 4, prec=16), W, H, 4, 16, C.CMYK)]
    for f in files:
        d = G.probe_display(f)
        comps = G.probe_components(f, precision=True)
        assert list(zip(d.channels, d.precisions, d.signed)) == [((dx, dy), p, s) for dx, dy, p, s in comps]
        ci, hi = G.probe_colour(f), G.probe_header(f)
        for name, _ in G.ColourInfo._fields_:
            a, b = getattr(d.colour, name), getattr(ci, name)
            assert (list(a) == list(b)) if hasattr(a, "__len__") else a == b, name
        assert d.colour.display_applied == 0
        for name, _ in G.ImageInfo._fields_:
            assert getattr(d.info, name) == getattr(hi, name), name
