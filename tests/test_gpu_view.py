"""Views on the GPU (k_view, gk_view.hip) through Engine.decode_view: a region at an exact size,
mirrored and rotated.

Truth: tests/view_ref.py (the size, the reduce level, the area average and the orientation in
numpy) applied to what a fresh engine's decode_pixels(window=region, sample_bytes=0) returns under
set_decode_reduce(r) and the same display / precision settings.  Every comparison is exact.
Streams are written by the engine's encoder."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import grok_amd as G
import display_cases as C
import view_ref as V

pytestmark = pytest.mark.gpu

NP = {1: np.uint8, 2: np.uint16, 0: np.int32}
TORCH = {1: torch.uint8, 2: torch.int16, 0: torch.int32}


@pytest.fixture(scope="module")
def eng():
    e = G.Engine(0)
    yield e
    e.close()


def fresh(call):
    e = G.Engine(0)
    try:
        return call(e)
    finally:
        e.close()


@contextlib.contextmanager
def settings(e, rgb=False, upsample=False, precision=None):
    e.set_decode_display(rgb=rgb, upsample=upsample)
    e.set_decode_precision(precision)
    try:
        yield
    finally:
        e.set_decode_display()
        e.set_decode_precision(None)


def encode(e, planes, prec, signed=False, **kw):
    kw.setdefault("mct", False)
    return e.encode(np.stack(planes).astype(np.int32), prec, signed=signed, params=G.default_params(**kw))


class Case:
    """A stream, its size, the reduce levels it allows and the settings it is decoded under."""

    def __init__(self, data, w, h, max_reduce, **sett):
        self.data, self.w, self.h, self.max_reduce, self.sett = data, w, h, max_reduce, sett
        self.refs = {}

    def reference(self, region, r):
        """A fresh engine's decode_pixels of the region at reduce r: (rh, rw, C) int32, computed once."""
        key = (region, r)
        if key not in self.refs:
            def call(e):
                with settings(e, **self.sett):
                    e.set_decode_reduce(r)
                    return e.decode_pixels(self.data, window=region, sample_bytes=0)
            self.refs[key] = fresh(call)
            self.refs[key].setflags(write=False)
        return self.refs[key]

    def want(self, region=None, size=None, width=None, height=None, fit=False, rotate=0, mirror=False):
        box = region or (0, 0, self.w, self.h)
        ow, oh = size if size else (width or 0, height or 0)
        ow, oh = V.resolve_size(box[2] - box[0], box[3] - box[1], ow, oh, fit)
        r = V.choose_reduce(box, ow, oh, self.max_reduce)
        src = self.reference(region, r)
        x0, y0, x1, y1 = V.reduced(box, r)
        assert src.shape[:2] == (y1 - y0, x1 - x0)
        return V.view(src, ow, oh, rotate, mirror), r, (x0, y0, x1, y1), (ow, oh)


@pytest.fixture(scope="module")
def cases(eng):
    P = C.random_planes
    sub = P(34, 18, C.S420, 8, seed=7)
    p420 = G.default_params(numresolution=C.numres_for(34, 18, C.S420), mct=False)
    f420 = C.wrap(eng.encode([np.ascontiguousarray(p, np.int32) for p in sub], 8, params=p420, subsampling=C.S420, size=(34, 18)),
                  34, 18, 3, 8, C.SYCC)
    return {
        "rgb": Case(encode(eng, P(53, 37, C.S444, 8, seed=1), 8, numresolution=3), 53, 37, 2),
        "tiled": Case(encode(eng, P(64, 48, C.S444, 8, seed=2), 8, numresolution=3, tiles=(32, 32)), 64, 48, 2),
        "grey97": Case(encode(eng, P(45, 31, [(1, 1)], 12, seed=3, signed=True), 12, signed=True, numresolution=3,
                              irreversible=True), 45, 31, 2),
        "c4": Case(encode(eng, P(21, 19, [(1, 1)] * 4, 8, seed=4), 8, numresolution=2), 21, 19, 1),
        "c5": Case(encode(eng, P(21, 19, [(1, 1)] * 5, 10, seed=5), 10, numresolution=2), 21, 19, 1),
        "sycc420": Case(f420, 34, 18, 0, rgb=True, upsample=True),
        "rgb12_8S": Case(encode(eng, P(34, 18, C.S444, 12, seed=6), 12, numresolution=3), 34, 18, 2, precision="8S"),
        "one": Case(encode(eng, P(64, 48, [(1, 1)], 8, seed=8), 8, numresolution=1), 64, 48, 0),
    }


def check(eng, case, sample_bytes=0, **kw):
    want, r, rect, size = case.want(**kw)
    with settings(eng, **case.sett):
        got = eng.decode_view(case.data, sample_bytes=sample_bytes, **kw)
    vr = eng.view_result
    assert (vr.reduce, (vr.rx0, vr.ry0, vr.rx1, vr.ry1), (vr.out_w, vr.out_h)) == (r, rect, size)
    assert (vr.pix_h, vr.pix_w, vr.channels) == got.shape == want.shape
    np.testing.assert_array_equal(got, want.astype(got.dtype))
    return got, vr


# ---------------------------------------------------------------- 1. sizes
def test_identity_size(eng, cases):
    got, vr = check(eng, cases["rgb"], size=(53, 37), sample_bytes=1)
    assert vr.reduce == 0 and got.dtype == np.uint8
    np.testing.assert_array_equal(got, cases["rgb"].reference(None, 0))
    check(eng, cases["tiled"], size=(16, 12))            # a copy of reduce level 2
    assert eng.view_result.reduce == 2


def test_two_to_one(eng, cases):
    check(eng, cases["tiled"], size=(32, 24))            # all of it done by the reduce level
    assert eng.view_result.reduce == 1
    got, vr = check(eng, cases["one"], size=(32, 24))    # all of it done by the kernel: rounded 2 x 2 means
    src = cases["one"].reference(None, 0).astype(np.int64)
    np.testing.assert_array_equal(got, (2 * src.reshape(24, 2, 32, 2, 1).sum(axis=(1, 3)) + 4) // 8)


@pytest.mark.parametrize("name", ["rgb", "grey97", "c4", "c5", "sycc420", "rgb12_8S"])
def test_non_integer_ratios(eng, cases, name):
    c = cases[name]
    check(eng, c, size=(c.w * 29 // 53, c.h * 17 // 37))     # 29 x 17 from 53 x 37, and its like
    check(eng, c, size=(c.w - 1, c.h - 1))
    check(eng, c, size=(c.w // 3 + 1, c.h // 2 + 1), rotate=90, mirror=True)


def test_thin_outputs(eng, cases):
    for name in ("rgb", "tiled", "one", "c5"):
        c = cases[name]
        check(eng, c, size=(1, 1))
        check(eng, c, size=(20, 1))                      # one output row
        check(eng, c, size=(1, 19))                      # one output column
        check(eng, c, size=(c.w, 1), rotate=270)
        check(eng, c, region=(3, 2, 4, 3), size=(1, 1))  # a region of one sample


def test_one_resolution_eight_to_one(eng, cases):
    got, vr = check(eng, cases["one"], size=(8, 6))
    assert vr.reduce == 0 and (vr.rx1, vr.ry1) == (64, 48)
    check(eng, cases["one"], size=(7, 5), rotate=90)     # footprints of 10 x 10 samples with partial edges
    check(eng, cases["one"], size=(1, 1))                # the whole image in one pixel


def test_region_across_tiles(eng, cases):
    c = cases["tiled"]
    for size, r in (((29, 20), 0), ((28, 20), 1), ((25, 17), 1), ((14, 10), 2), ((9, 4), 2)):
        got, vr = check(eng, c, region=(5, 3, 61, 44), size=size)
        assert vr.reduce == r
    check(eng, c, region=(31, 15, 33, 17), size=(2, 2))
    check(eng, c, region=(0, 0, 64, 48), size=(40, 30))


def test_all_zero_region_is_the_whole_image(eng, cases):
    c = cases["rgb"]
    d = torch.from_numpy(np.frombuffer(c.data, np.uint8).copy()).cuda()
    for kw in (dict(size=(1, 5)), dict(height=30, rotate=90), dict(size=(20, 20), fit=True, mirror=True)):
        want = c.want(**kw)[0]
        for data in (c.data, d):       # host bytes: sized by the probe; device bytes: by the binding's rule
            got = eng.decode_view(data, region=(0, 0, 0, 0), length=len(c.data), **kw)
            assert got.shape == want.shape
            np.testing.assert_array_equal(got, want)
    # refusals of device bytes come from the engine as well, and leave it alone
    for needle, kw in (("upscaling", dict(size=(54, 37))), ("both 0", dict()), ("empty or leaves", dict(region=(5, 5, 5, 9), width=1))):
        with pytest.raises(RuntimeError, match=needle):
            eng.decode_view(d, length=len(c.data), **kw)
    np.testing.assert_array_equal(eng.decode_view(d, size=(13, 9), length=len(c.data)), c.want(size=(13, 9))[0])


def test_fit_and_one_sided(eng, cases):
    c = cases["rgb"]
    assert check(eng, c, width=26)[1].out_h == 18
    assert check(eng, c, height=9)[1].out_w == 13
    assert check(eng, c, size=(20, 20), fit=True)[0].shape == (14, 20, 3)
    assert check(eng, c, size=(40, 10), fit=True)[0].shape == (10, 14, 3)
    assert check(eng, c, region=(10, 5, 50, 30), size=(40, 40), fit=True)[0].shape == (25, 40, 3)


@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("rotate", [0, 90, 180, 270])
def test_orientations(eng, cases, rotate, mirror):
    got, vr = check(eng, cases["rgb"], size=(29, 17), rotate=rotate, mirror=mirror, sample_bytes=1)
    assert got.shape == ((29, 17, 3) if rotate in (90, 270) else (17, 29, 3))
    check(eng, cases["c5"], size=(18, 7), rotate=rotate, mirror=mirror)
    check(eng, cases["tiled"], region=(5, 3, 61, 44), size=(25, 17), rotate=rotate, mirror=mirror)


# ---------------------------------------------------------------- 2. sample types and where the bytes live
def test_sample_bytes(eng, cases):
    for sb in (0, 1):
        assert check(eng, cases["rgb"], size=(29, 17), sample_bytes=sb)[0].dtype == NP[sb]
    assert check(eng, cases["rgb12_8S"], size=(20, 11), sample_bytes=1)[0].dtype == np.uint8
    assert check(eng, cases["grey97"], size=(29, 17), sample_bytes=2)[0].dtype == np.int16
    assert check(eng, cases["grey97"], size=(29, 17), sample_bytes=0)[0].min() < 0
    assert check(eng, cases["c5"], size=(11, 9), sample_bytes=2)[0].dtype == np.uint16


def test_device_output_with_padded_rows(eng, cases):
    c = cases["rgb"]
    d = torch.from_numpy(np.frombuffer(c.data, np.uint8).copy()).cuda()
    for rotate, sb in ((0, 1), (90, 1), (180, 0), (270, 2)):
        case = cases["c5"] if sb == 2 else c
        data = d if case is c else case.data
        want = case.want(size=(18, 11), rotate=rotate, mirror=True)[0]
        h, w, nc = want.shape
        es, fill = sb or 4, 77
        row = -(-(w * nc * es + 1) // 64) * 64 // es                 # rows padded to 64 bytes, never tight
        buf = torch.full((h + 2, row), fill, dtype=TORCH[sb], device="cuda")
        out = buf[1:h + 1, :w * nc].unflatten(1, (w, nc))
        eng.decode_view(data, size=(18, 11), rotate=rotate, mirror=True, out=out, length=len(case.data))
        b = buf.cpu().numpy().view(NP[sb])
        np.testing.assert_array_equal(b[1:h + 1, :w * nc].reshape(h, w, nc), want.astype(NP[sb]))
        assert (b[1:h + 1, w * nc:] == fill).all()                   # past each row
        assert (b[0] == fill).all() and (b[h + 1] == fill).all()     # before the first and past the last row
    y = torch.zeros((17, 29, 3), dtype=torch.uint8, device="cuda")   # tight rows, device bytes in, device pixels out
    eng.decode_view(d, size=(29, 17), out=y, length=len(c.data))
    np.testing.assert_array_equal(y.cpu().numpy(), c.want(size=(29, 17))[0])
    got = eng.decode_view(d, size=(29, 17), length=len(c.data), sample_bytes=1)   # device bytes in, host pixels out
    np.testing.assert_array_equal(got, c.want(size=(29, 17))[0])


# ---------------------------------------------------------------- 3. refusals
def test_refusals_name_their_cause_and_leave_the_engine_alone(eng, cases):
    c = cases["rgb"]
    first = fresh(lambda e: e.decode(c.data))
    for needle, kw in (("rotate 45", dict(size=(5, 5), rotate=45)), ("mirror must be", dict(size=(5, 5), mirror=2)),
                       ("fit must be", dict(size=(5, 5), fit=2)), ("empty or leaves", dict(region=(0, 0, 54, 37), size=(1, 1))),
                       ("empty or leaves", dict(region=(7, 7, 7, 9), size=(1, 1))), ("upscaling", dict(size=(54, 37))),
                       ("upscaling", dict(width=60)), ("both 0", dict())):
        with pytest.raises(RuntimeError, match=needle):
            eng.decode_view(c.data, **kw)
    eng.set_decode_reduce(1)
    try:
        with pytest.raises(RuntimeError, match="gk_set_decode_reduce"):
            eng.decode_view(c.data, size=(5, 5))
        assert np.asarray(eng.decode(c.data)).shape == (3, 19, 27)   # the sticky level is still 1
    finally:
        eng.set_decode_reduce(0)
    # whatever the pixel calls refuse
    with pytest.raises(RuntimeError, match="GK_DISPLAY_UPSAMPLE"):
        eng.decode_view(cases["sycc420"].data, size=(8, 4))
    with pytest.raises(RuntimeError, match="sample_bytes"):
        eng.decode_view(cases["rgb12_8S"].data, size=(8, 4), sample_bytes=1)
    many = encode(eng, C.random_planes(16, 8, [(1, 1)] * 17, 8, seed=93), 8, numresolution=2)
    with pytest.raises(RuntimeError, match="planar calls"):
        eng.decode_view(many, size=(4, 4))
    # (row_bytes is the binding's to compute: the C entry is called with a short and an odd one)
    b = np.frombuffer(cases["rgb12_8S"].data, np.uint8)
    out = np.zeros((11, 20, 3), np.uint16)
    v, res = G.View(0, 0, 0, 0, 20, 11, 0, 0, 0), G.ViewResult()
    for row_bytes in (20 * 3 * 2 - 2, 20 * 3 * 2 + 1):
        rc = eng.lib.gk_decode_view_pixels(eng.ctx, ctypes.c_void_p(b.ctypes.data), len(b), 0, ctypes.byref(v),
                                           ctypes.c_void_p(out.ctypes.data), row_bytes, 2, 0, ctypes.byref(res))
        assert rc != 0 and "row_bytes" in eng.lib.gk_last_error(eng.ctx).decode()
    assert not out.any() and res.pix_w == 0
    # a stream that holds only some of its tiles
    planes = np.stack(C.random_planes(64, 48, C.S444, 8, seed=95)).astype(np.int32)
    p = G.default_params(numresolution=3, mct=False, tiles=(32, 32))
    part = eng.main_header(planes.shape, 8, params=p)[0] + eng.encode_tiles(planes, 8, 0, 2, params=p)[0] + b"\xff\xd9"
    with pytest.raises(RuntimeError, match="only some of its tiles"):
        eng.decode_view(part, size=(20, 20))
    # after all of them: a plain decode is a fresh engine's, at full resolution
    np.testing.assert_array_equal(eng.decode(c.data), first)


# ---------------------------------------------------------------- 4. history
def test_view_after_a_dense_decode(eng, cases):
    big = encode(eng, C.random_planes(300, 200, C.S444, 12, seed=111), 12, numresolution=4)
    c = cases["tiled"]
    kw = dict(region=(5, 3, 61, 44), size=(25, 17), rotate=90)
    alone = fresh(lambda e: e.decode_view(c.data, **kw))
    eng.decode(big)
    np.testing.assert_array_equal(eng.decode_view(c.data, **kw), alone)
    np.testing.assert_array_equal(alone, c.want(**kw)[0])


def test_plain_decodes_after_a_view(eng, cases):
    c, o = cases["tiled"], cases["rgb"]
    planar = fresh(lambda e: e.decode(c.data))
    pixels = fresh(lambda e: e.decode_pixels(o.data, sample_bytes=1))
    window = fresh(lambda e: e.decode_pixels(c.data, window=(5, 3, 61, 44)))
    eng.decode_view(c.data, region=(5, 3, 61, 44), size=(14, 10), rotate=270, mirror=True)
    assert eng.view_result.reduce == 2
    np.testing.assert_array_equal(eng.decode(c.data), planar)                       # full resolution again
    eng.decode_view(o.data, size=(13, 9))
    np.testing.assert_array_equal(eng.decode_pixels(o.data, sample_bytes=1), pixels)
    eng.decode_view(c.data, size=(16, 12))
    np.testing.assert_array_equal(eng.decode_pixels(c.data, window=(5, 3, 61, 44)), window)
    hdr = eng.read_header(c.data)
    assert (hdr.w, hdr.h, hdr.numcomps, hdr.prec) == (64, 48, 3, 8)


def test_refused_view_then_a_plain_decode(eng, cases):
    c = cases["tiled"]
    planar = fresh(lambda e: e.decode(c.data))
    with pytest.raises(RuntimeError, match="upscaling"):
        eng.decode_view(c.data, region=(5, 3, 61, 44), size=(57, 41))
    got = eng.decode(c.data)
    assert np.asarray(got).shape == (3, 48, 64)                                     # the sticky reduce is still 0
    np.testing.assert_array_equal(got, planar)
    np.testing.assert_array_equal(eng.decode_view(c.data, size=(16, 12)), c.want(size=(16, 12))[0])
