"""Colour management on the GPU (k_icc_rgb / k_lab_rgb, gk_icc.hip) under GK_DISPLAY_ICC.

Judge: tests/icc_ref.py, the float64 restatement that tests/test_icc.py pins to lcms2.  Rule of
every comparison (icc_ref.check): the engine's sample equals the rounded reference, except where
the unrounded reference lies within tau(p) = 2^(p - 19) LSB of a rounding tie, where it may differ
by 1.  Inputs are lossless 5/3 streams from eng.encode, so the decoded planes are the source
samples; for windows and reduced decodes the reference is applied to the same engine's decode
without the flag."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import grok_amd as G
import icc_profiles as P
import icc_ref as R
import jp2_boxes as J

pytestmark = pytest.mark.gpu

NP = {1: np.uint8, 2: np.uint16, 0: np.int32}
TORCH = {1: torch.uint8, 2: torch.int16, 0: torch.int32}
RGB_PROFILES = sorted(n for n, (_, grey) in P.accepted().items() if not grey)
CUSTOM = (100, 0, 180, 1 << 15, 180, 1 << 15, P.CIE_D65)


@pytest.fixture(scope="module")
def eng():
    e = G.Engine(0)
    yield e
    e.close()


@contextlib.contextmanager
def settings(eng, icc=True, force_rgb=False, precision=None, reduce=0):
    eng.set_decode_display(icc=icc, force_rgb=force_rgb)
    eng.set_decode_precision(precision)
    eng.set_decode_reduce(reduce)
    try:
        yield
    finally:
        eng.set_decode_display()
        eng.set_decode_precision(None)
        eng.set_decode_reduce(0)


def encode(eng, planes, prec, signed=False, **kw):
    kw.setdefault("numresolution", 3)
    kw.setdefault("mct", False)
    return eng.encode(np.ascontiguousarray(planes, np.int32), prec, signed=signed, params=G.default_params(**kw))


def samples(nc, h, w, prec, seed):
    a = np.random.RandomState(seed).randint(0, 1 << prec, (nc, h, w)).astype(np.int32)
    a[:, 0, 0], a[:, 0, 1] = 0, (1 << prec) - 1
    return a


def wrap(cs, planes, prec, colr, cdef=None, extra=()):
    nc, h, w = planes.shape
    return P.jp2(cs, h, w, nc, prec, colr, cdef, extra)


def rgb_case(eng, h, w, prec, seed, nc=3):
    planes = samples(nc, h, w, prec, seed)
    if prec <= 8 and w * h >= 8:      # the eight corners of the cube
        for i in range(8):
            planes[:3, h - 1, i] = [((i >> k) & 1) * ((1 << prec) - 1) for k in range(3)]
    return planes, encode(eng, planes, prec)


def dev(data):
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()


def bits(t, sb):
    return t.cpu().numpy().view(NP[sb])


def want_rgb(profile, planes, prec):
    """(unrounded, rounded), channel first like the decode"""
    u, r = R.apply_profile(profile, np.moveaxis(np.asarray(planes[:3], np.int64), 0, -1), prec)
    return np.moveaxis(u, -1, 0), np.moveaxis(r, -1, 0)


def assert_matches(got, unrounded, rounded, prec):
    bad = R.check(got, unrounded, rounded, prec)
    print("max difference", int(np.abs(np.asarray(got, np.int64) - rounded).max()), "outside the rule", bad)
    assert bad == 0


# ---------------------------------------------------------------- RGB profiles at 8 bits
def test_rgb8_every_profile_odd_width(eng):
    planes, cs = rgb_case(eng, 5, 67, 8, 1)
    for name in RGB_PROFILES:
        prof = P.accepted()[name][0]
        f = wrap(cs, planes, 8, P.colr_profile(prof))
        u, r = want_rgb(prof, planes, 8)
        with settings(eng):
            hdr = eng.read_header(f)
            ci = eng.colour_info()
            assert (hdr.numcomps, hdr.prec, ci.colour_space, ci.display_applied) == (3, 8, 2, 8)
            for sb in (1, 0):
                got = eng.decode(f, sample_bytes=sb)
                assert got.dtype == NP[sb] and got.shape == (3, 5, 67)
                assert_matches(got, u, r, 8)
        np.testing.assert_array_equal(eng.decode(f), planes)       # the flag off: the samples as coded
    assert r[:, 4, 0].tolist() == [0, 0, 0] and r[:, 4, 7].tolist() == [255, 255, 255]


def test_grey8_every_level(eng):
    planes = np.arange(256, dtype=np.int32).reshape(1, 16, 16)
    cs = encode(eng, planes, 8)
    for name in ("grey_g22", "grey_table"):
        prof = P.accepted()[name][0]
        f = wrap(cs, planes, 8, P.colr_profile(prof))
        u, r = R.apply_profile(prof, planes[0], 8)
        with settings(eng):
            got = eng.decode(f, sample_bytes=1)
            assert got.shape == (1, 16, 16) and eng.colour_info().colour_space == 3 and eng.colour_info().display_applied == 8
            assert_matches(got[0], u, r, 8)
        with settings(eng, force_rgb=True):
            got = eng.decode(f)
            assert got.shape == (3, 16, 16) and eng.colour_info().colour_space == 2 and eng.colour_info().display_applied == 12
            for k in range(3):
                assert_matches(got[k], u, r, 8)
            np.testing.assert_array_equal(eng.decode_pixels(f, sample_bytes=1), np.moveaxis(got, 0, -1))


# ---------------------------------------------------------------- wider samples: float32 to 12 bits, double above
# (4097-entry tables: three of them are 48 KiB of floats / 96 KiB of doubles, past the 32 KiB the
#  kernel stages in LDS: the global-memory path; the 1,024-entry ones are staged)
LONG = P.curv_table(P.table_curve(4097))
WIDE = {
    "adobe_g22": P.accepted()["adobe_g22"][0],
    "p3_table1024": P.accepted()["p3_table1024"][0],
    "prophoto_para3": P.accepted()["prophoto_para3"][0],
    "adobe_three_curves": P.accepted()["adobe_three_curves"][0],
    "p3_para4": P.accepted()["p3_para4"][0],
    "prophoto_table4097_global": P.rgb_profile("prophoto", [LONG, P.curv_table(P.table_curve(4097, 2.2)), LONG]),
}


@pytest.mark.parametrize("prec", [12, 16, 9, 13])
def test_rgb_wide(eng, prec):
    planes, cs = rgb_case(eng, 48, 64, prec, prec)
    for name, prof in WIDE.items():
        f = wrap(cs, planes, prec, P.colr_profile(prof))
        u, r = want_rgb(prof, planes, prec)
        with settings(eng):
            assert eng.read_header(f).prec == prec
            assert_matches(eng.decode(f, sample_bytes=2), u, r, prec)
            y = torch.zeros((3, 48, 64), dtype=torch.int32, device="cuda")
            fd = dev(f)
            eng.decode(fd, length=len(f), out=y)                      # device bytes to device planes
            assert_matches(y.cpu().numpy(), u, r, prec)


def test_rgb16_pixels_forced_precision(eng):
    planes, cs = rgb_case(eng, 48, 64, 16, 21)
    prof = WIDE["adobe_three_curves"]
    f = wrap(cs, planes, 16, P.colr_profile(prof))
    with settings(eng):
        full = eng.decode(f)
        assert_matches(full, *want_rgb(prof, planes, 16), 16)
        got = eng.decode_pixels(f, sample_bytes=2)
        np.testing.assert_array_equal(got, np.moveaxis(full, 0, -1).astype(np.uint16))
    with settings(eng, precision="8S"):
        assert eng.read_header(f).prec == 8
        got = eng.decode_pixels(f, sample_bytes=1)
        assert got.shape == (48, 64, 3) and got.dtype == np.uint8
        np.testing.assert_array_equal(got, np.moveaxis(full, 0, -1) // 256)     # scale_component down: C division
        y = torch.zeros((48, 64, 3), dtype=torch.uint8, device="cuda")
        eng.decode_pixels(dev(f), length=len(f), out=y)
        np.testing.assert_array_equal(y.cpu().numpy(), got)


# ---------------------------------------------------------------- opacity beside the colours
def test_rgba_and_grey_alpha(eng):
    planes, cs = rgb_case(eng, 5, 67, 8, 31, nc=4)
    prof = P.accepted()["p3_g18"][0]
    f = wrap(cs, planes, 8, P.colr_profile(prof), P.RGBA_CDEF)
    plain = eng.decode(f)
    with settings(eng):
        got = eng.decode(f, sample_bytes=1)
        assert got.shape == (4, 5, 67) and list(eng.colour_info().typ[:4]) == [0, 0, 0, 1]
        assert_matches(got[:3], *want_rgb(prof, planes, 8), 8)
        np.testing.assert_array_equal(got[3], plain[3])               # opacity: bit-identical
        np.testing.assert_array_equal(eng.decode_pixels(f, sample_bytes=1), np.moveaxis(got, 0, -1))
    # a cdef that reorders: B, G, R, A in the codestream
    f = wrap(cs, planes, 8, P.colr_profile(prof), [(0, 0, 3), (1, 0, 2), (2, 0, 1), (3, 1, 0)])
    with settings(eng):
        got = eng.decode(f)
        assert_matches(got[:3], *want_rgb(prof, planes[[2, 1, 0]], 8), 8)
        np.testing.assert_array_equal(got[3], planes[3])
    g = samples(2, 5, 67, 8, 32)
    gprof = P.accepted()["grey_g22"][0]
    f = wrap(encode(eng, g, 8), g, 8, P.colr_profile(gprof), P.GREYA_CDEF)
    u, r = R.apply_profile(gprof, g[0], 8)
    with settings(eng):
        got = eng.decode(f, sample_bytes=1)
        assert got.shape == (2, 5, 67) and eng.colour_info().colour_space == 3
        assert_matches(got[0], u, r, 8)
        np.testing.assert_array_equal(got[1], g[1])
    with settings(eng, force_rgb=True):
        got = eng.decode_pixels(f, sample_bytes=1)
        assert got.shape == (5, 67, 4) and eng.colour_info().colour_space == 2
        for k in range(3):
            assert_matches(got[:, :, k], u, r, 8)
        np.testing.assert_array_equal(got[:, :, 3], g[1])


# ---------------------------------------------------------------- CIELab
@pytest.mark.parametrize("prec,custom", [(8, None), (16, CUSTOM), (12, None)])
def test_cielab(eng, prec, custom):
    planes = samples(3, 9, 67, prec, 40 + prec)
    cs = encode(eng, planes, prec)
    f = wrap(cs, planes, prec, P.colr_lab(custom))
    np.testing.assert_array_equal(eng.decode(f), planes)                 # without the flag: L*, a*, b* as coded
    assert eng.colour_info().colour_space == (7 if custom is None else 8) and eng.cielab() == P.lab_words(custom)
    u, r = R.lab_to_rgb(R.lab_values(np.moveaxis(planes.astype(np.int64), 0, -1), prec, P.lab_words(custom)))
    u, r = np.moveaxis(u, -1, 0), np.moveaxis(r, -1, 0)
    with settings(eng):
        hdr = eng.read_header(f)
        assert (hdr.prec, eng.colour_info().colour_space, eng.colour_info().display_applied) == (16, 2, 8)
        assert [p for p, _ in eng.precisions()] == [16, 16, 16]
        for sb in (2, 0):
            got = eng.decode(f, sample_bytes=sb)
            assert got.dtype == NP[sb]
            assert_matches(got, u, r, 16)
        y = torch.zeros((3, 9, 67), dtype=torch.int16, device="cuda")
        eng.decode(f, out=y)
        assert_matches(bits(y, 2), u, r, 16)
        if prec == 8:
            with pytest.raises(RuntimeError, match="output planes"):     # 16-bit output into 8-bit planes
                eng.decode(f, sample_bytes=1)


# ---------------------------------------------------------------- windows, reduction, where the bytes live
def test_window_reduce_and_placement(eng):
    planes, cs = rgb_case(eng, 5, 67, 8, 51)
    prof = P.accepted()["adobe_para2"][0]
    f = wrap(cs, planes, 8, P.colr_profile(prof))
    win = (3, 3, 64, 5)
    part = eng.decode_window(f, win)
    np.testing.assert_array_equal(part, planes[:, 3:5, 3:64])
    u, r = want_rgb(prof, part, 8)
    with settings(eng):
        for sb in (1, 0):
            assert_matches(eng.decode_window(f, win, sample_bytes=sb), u, r, 8)
        y = torch.zeros((3, 2, 61), dtype=torch.uint8, device="cuda")
        eng.decode_window(dev(f), win, length=len(f), out=y)
        assert_matches(y.cpu().numpy(), u, r, 8)
        got = eng.decode_pixels(f, sample_bytes=1, window=win)
        assert got.shape == (2, 61, 3)
        assert_matches(np.moveaxis(got, -1, 0), u, r, 8)
    with settings(eng, icc=False, reduce=1):
        small = eng.decode(f)
    assert small.shape == (3, 3, 34)
    u, r = want_rgb(prof, small, 8)
    with settings(eng, reduce=1):
        assert_matches(eng.decode(f, sample_bytes=1), u, r, 8)
    # a tiled 16-bit image: windows at every edge, the layer limit
    planes, _ = rgb_case(eng, 48, 64, 16, 52)
    cs = encode(eng, planes, 16, tiles=(32, 32), numresolution=2)
    prof = WIDE["p3_table1024"]
    f = wrap(cs, planes, 16, P.colr_profile(prof))
    for win in ((0, 0, 33, 7), (31, 40, 64, 48), (5, 5, 6, 6)):
        u, r = want_rgb(prof, planes[:, win[1]:win[3], win[0]:win[2]], 16)
        with settings(eng):
            assert_matches(eng.decode_window(f, win, sample_bytes=2), u, r, 16)
    eng.set_decode_layers(1)
    try:
        with settings(eng):
            assert_matches(eng.decode(f), *want_rgb(prof, planes, 16), 16)
    finally:
        eng.set_decode_layers(0)


# ---------------------------------------------------------------- history
def header_fields(eng, data):
    hdr = eng.read_header(data)
    return [getattr(hdr, n) for n, _ in G.ImageInfo._fields_], eng.colour_info().colour_space, eng.precisions()


def test_history(eng):
    planes, cs = rgb_case(eng, 33, 65, 8, 61)
    p16, cs16 = rgb_case(eng, 24, 40, 16, 62)
    a = wrap(cs, planes, 8, P.colr_profile(P.accepted()["adobe_g22"][0]))
    b = wrap(cs16, p16, 16, P.colr_profile(WIDE["prophoto_table4097_global"]))
    bad = wrap(cs, planes, 8, P.colr_profile(P.refused()["curve_overrun"][0]))
    first = eng.decode(a)
    before = header_fields(eng, a)
    with settings(eng):
        one = eng.decode(a)
        assert_matches(one, *want_rgb(P.accepted()["adobe_g22"][0], planes, 8), 8)
        two = eng.decode(b)
        assert_matches(two, *want_rgb(WIDE["prophoto_table4097_global"], p16, 16), 16)
        with pytest.raises(RuntimeError, match="overruns"):
            eng.decode(bad)
        with pytest.raises(RuntimeError, match="overruns"):
            eng.read_header(bad)
        np.testing.assert_array_equal(eng.decode(a), one)             # a refused profile leaves nothing behind
        fresh = G.Engine(0)
        try:
            fresh.set_decode_display(icc=True)
            np.testing.assert_array_equal(fresh.decode(a), one)
            np.testing.assert_array_equal(fresh.decode(b), two)
        finally:
            fresh.close()
    np.testing.assert_array_equal(eng.decode(a), first)               # the flag cleared: the plain decode again
    assert header_fields(eng, a) == before
    np.testing.assert_array_equal(first, planes)


# ---------------------------------------------------------------- refusals
def patch_siz(f, comp, ssiz=None, xrsiz=None):
    b = bytearray(f)
    at = b.index(b"\xff\x4f\xff\x51") + 4 + 2 + 2 + 32 + 2 + 3 * comp
    if ssiz is not None:
        b[at] = ssiz
    if xrsiz is not None:
        b[at + 1] = xrsiz
    return bytes(b)


def test_refusals_reach_the_caller(eng):
    planes, cs = rgb_case(eng, 16, 16, 8, 71)
    adobe, grey = P.accepted()["adobe_g22"][0], P.accepted()["grey_g22"][0]
    sgn = np.random.RandomState(72).randint(-128, 128, (3, 16, 16)).astype(np.int32)
    pal = [J.pclr(np.arange(256 * 3).reshape(256, 3) % 256, [8, 8, 8]), J.cmap([(0, 1, 0), (0, 1, 1), (0, 1, 2)])]
    p17 = wrap(encode(eng, samples(3, 16, 16, 16, 73), 16), planes, 16, P.colr_profile(adobe))
    for c in range(3):
        p17 = patch_siz(p17, c, ssiz=16)
    sub = wrap(cs, planes, 8, P.colr_profile(adobe))
    for c in range(3):
        sub = patch_siz(sub, c, xrsiz=2)
    cases = [
        (P.jp2(encode(eng, sgn, 8, signed=True), 16, 16, 3, 8, P.colr_profile(adobe), signed=True), "signed"),
        (P.jp2(encode(eng, sgn, 8, signed=True), 16, 16, 3, 8, P.colr_lab(), signed=True), "signed"),
        (p17, "17 bits"),
        (wrap(encode(eng, planes[:2], 8), planes[:2], 8, P.colr_profile(adobe)), "RGB profile on an image of 2 channels"),
        (wrap(cs, planes, 8, P.colr_profile(grey)), "grey profile on an image of 3 channels"),
        (sub, "subsampled"),
        (wrap(encode(eng, planes[:1], 8), planes[:1], 8, P.colr_profile(adobe), extra=pal), "palette"),
    ]
    for name, (prof, words) in P.refused().items():
        if not name.startswith("grey"):
            cases.append((wrap(cs, planes, 8, P.colr_profile(prof)), words))
    with settings(eng):
        for f, words in cases:
            out = np.full((4, 16, 16), -7, np.int32)
            with pytest.raises(RuntimeError, match=words):
                eng.read_header(f)
            b = np.frombuffer(f, np.uint8)
            ptrs = (ctypes.c_void_p * 4)(*[out[k].ctypes.data for k in range(4)])
            strides = (ctypes.c_uint32 * 4)(16, 16, 16, 16)
            rc = eng.lib.gk_decode(eng.ctx, b.ctypes.data, len(f), 0, ptrs, strides, 0, 0)
            assert rc != 0 and words in eng.lib.gk_last_error(eng.ctx).decode()
            assert (out == -7).all()                                   # nothing was written
    # a stream that holds only some of its tiles
    big = samples(3, 48, 64, 8, 74)
    p = G.default_params(numresolution=3, mct=False, tiles=(32, 32))
    body, _ = eng.encode_tiles(big, 8, 0, 2, params=p)
    hdr, _, _ = eng.main_header(big.shape, 8, params=p)
    part = wrap(hdr + body + b"\xff\xd9", big, 8, P.colr_profile(adobe))
    with settings(eng):
        with pytest.raises(RuntimeError, match="only some of its tiles"):
            eng.decode(part)
    # 8-bit planes for a 12-bit image
    p12, cs12 = rgb_case(eng, 16, 16, 12, 75)
    with settings(eng):
        with pytest.raises(RuntimeError, match="output planes"):
            eng.decode(wrap(cs12, p12, 12, P.colr_profile(adobe)), sample_bytes=1)
