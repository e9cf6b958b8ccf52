"""Float tensors on the GPU (k_tensor, gk_tensor.hip) through Engine.decode_tensor.

Truth: tests/tensor_ref.py (the rule in numpy: two float32 roundings, then the output type's)
applied to what the same engine's decode_view(..., sample_bytes=0) returns for the same view; the
view itself is pinned by test_gpu_view.py.  Every comparison is on bit patterns.  Streams are
written by the engine's encoder."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import grok_amd as G
import display_cases as C
import tensor_ref as T

pytestmark = pytest.mark.gpu

TORCH = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
DTYPES = ["float32", "float16", "bfloat16"]
LAYOUTS = ["chw", "hwc"]
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
NAN16 = 0x7FC1          # a NaN in float16 and in bfloat16: the fill of buffers that must stay untouched


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
    """A stream, its channel count, precision and sign as decoded, and the settings it is decoded under."""

    def __init__(self, data, nc, prec, signed=False, **sett):
        self.data, self.nc, self.prec, self.signed, self.sett = data, nc, prec, signed, sett


@pytest.fixture(scope="module")
def cases(eng):
    P = C.random_planes
    sub = P(34, 18, C.S420, 8, seed=7)
    p420 = G.default_params(numresolution=C.numres_for(34, 18, C.S420), mct=False)
    f420 = C.wrap(eng.encode([np.ascontiguousarray(p, np.int32) for p in sub], 8, params=p420, subsampling=C.S420, size=(34, 18)),
                  34, 18, 3, 8, C.SYCC)
    ramp = np.arange(65536, dtype=np.int32).reshape(1, 256, 256)
    big = np.full((16, 16), 2 ** 24, np.int64)
    big.reshape(-1)[:12] += [1, 3, 5, 7, 9, 11, -1, -3, -5, -7, -9, -11]
    big[15, 15] = 2 ** 25 - 1
    return {
        "rgb": Case(encode(eng, P(53, 37, C.S444, 8, seed=1), 8, numresolution=3), 3, 8),
        "tiled": Case(encode(eng, P(64, 48, C.S444, 8, seed=2), 8, numresolution=3, tiles=(32, 32)), 3, 8),
        "grey97": Case(encode(eng, P(45, 31, [(1, 1)], 12, seed=3, signed=True), 12, signed=True, numresolution=3,
                              irreversible=True), 1, 12, signed=True),
        "c5": Case(encode(eng, P(21, 19, [(1, 1)] * 5, 10, seed=5), 10, numresolution=2), 5, 10),
        "sycc420": Case(f420, 3, 8, rgb=True, upsample=True),
        "rgb12_8S": Case(encode(eng, P(34, 18, C.S444, 12, seed=6), 12, numresolution=3), 3, 8, precision="8S"),
        "ramp16": Case(encode(eng, ramp, 16, numresolution=3), 1, 16),
        "big25": Case(encode(eng, big[None].astype(np.int32), 25, numresolution=1), 1, 25),
    }


def tensor_bits(x):
    """The bit patterns of a numpy array or a torch tensor, as numpy."""
    if isinstance(x, np.ndarray):
        return T.bits(x)
    x = x.contiguous()
    if x.dtype == torch.float32:
        return x.view(torch.int32).cpu().numpy().view(np.uint32)
    return x.view(torch.int16).cpu().numpy().view(np.uint16)


def check(eng, case, dtype="float32", layout="chw", device=True, affine=None, **view):
    """decode_tensor of `view` against the rule applied to decode_view's int32 pixels.  affine: None
    (scale 1, bias 0), ("sb", scale, bias) or ("ms", mean, std, unit)."""
    kw, scale, bias = {}, None, None
    if affine and affine[0] == "sb":
        kw = dict(scale=affine[1], bias=affine[2])
        scale, bias = affine[1], affine[2]
    elif affine:
        kw = dict(mean=affine[1], std=affine[2], unit=affine[3])
        scale, bias = G._tensor_affine(affine[1], affine[2], affine[3], case.prec, case.signed)
    with settings(eng, **case.sett):
        pix = eng.decode_view(case.data, sample_bytes=0, **view)
        vr = eng.view_result
        want = T.apply(pix, scale, bias, dtype, layout)
        if device:
            out = torch.full(want.shape, float("nan"), dtype=TORCH[dtype], device="cuda")
            got = eng.decode_tensor(case.data, layout=layout, out=out, **kw, **view)
            assert got is out
        else:
            got = eng.decode_tensor(case.data, dtype=dtype, layout=layout, **kw, **view)
            assert isinstance(got, np.ndarray) and got.dtype == np.dtype(dtype) and got.flags.c_contiguous
    tr = eng.view_result
    assert [getattr(tr, f) for f, _ in tr._fields_] == [getattr(vr, f) for f, _ in vr._fields_]
    assert tuple(got.shape) == want.shape == ((vr.channels, vr.pix_h, vr.pix_w) if layout == "chw" else (vr.pix_h, vr.pix_w, vr.channels))
    np.testing.assert_array_equal(tensor_bits(got), T.bits(want))
    return got, pix


# ---------------------------------------------------------------- 1. identity
@pytest.mark.parametrize("layout", LAYOUTS)
def test_identity_is_the_pixels_as_floats(eng, cases, layout):
    got, pix = check(eng, cases["rgb"], "float32", layout, size=(53, 37))
    want = pix.astype(np.float32)
    np.testing.assert_array_equal(got.cpu().numpy(), want.transpose(2, 0, 1) if layout == "chw" else want)
    # none of the sizes: the region's own
    with settings(eng):
        a = eng.decode_tensor(cases["rgb"].data, layout=layout)
        b = eng.decode_tensor(cases["rgb"].data, region=(5, 3, 50, 30), layout=layout)
    np.testing.assert_array_equal(a, got.cpu().numpy())
    np.testing.assert_array_equal(b, a[:, 3:30, 5:50] if layout == "chw" else a[3:30, 5:50])


# ---------------------------------------------------------------- 2. normalised, at non-integer ratios
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_mean_std_at_non_integer_ratios(eng, cases, dtype, layout):
    check(eng, cases["rgb"], dtype, layout, affine=("ms", MEAN, STD, None), size=(20, 13))
    assert eng.view_result.reduce == 1
    check(eng, cases["tiled"], dtype, layout, affine=("ms", MEAN, STD, None), region=(5, 3, 61, 44), size=(25, 17))
    check(eng, cases["rgb"], dtype, layout, affine=("sb", [2.0, 0.5, 1.0 / 3], [-1.0, 0.125, 100.0]), size=(17, 16))   # exactly one tile high, just over one wide


# ---------------------------------------------------------------- 3. orientation
@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("rotate", [0, 90, 180, 270])
def test_orientations(eng, cases, rotate, mirror):
    got, _ = check(eng, cases["rgb"], "float16", "chw", affine=("ms", MEAN, STD, None), size=(29, 17), rotate=rotate, mirror=mirror)
    assert tuple(got.shape) == ((3, 29, 17) if rotate in (90, 270) else (3, 17, 29))
    check(eng, cases["rgb"], "float32", "chw", size=(53, 37), rotate=rotate, mirror=mirror)   # the copy branch


# ---------------------------------------------------------------- 4. more than one channel group
@pytest.mark.parametrize("layout", LAYOUTS)
def test_five_channels(eng, cases, layout):
    c = cases["c5"]
    check(eng, c, "bfloat16", layout, affine=("ms", 0.485, 0.229, None), size=(18, 7))                  # n = 1: broadcast
    check(eng, c, "float16", layout, affine=("ms", MEAN + [0.3, 0.7], STD + [0.5, 0.25], None), size=(18, 7))   # n = 5
    check(eng, c, "float32", layout, affine=("sb", [1.0, 2.0], [0.0, -3.0]), size=(21, 19))           # n = 2: the last entry repeats
    check(eng, c, "float32", layout, device=False, size=(1, 1))


# ---------------------------------------------------------------- 5. signed samples
def test_signed_needs_a_unit(eng, cases):
    c = cases["grey97"]
    for dtype in DTYPES:
        got, pix = check(eng, c, dtype, "chw", affine=("ms", 0.1, 0.5, 2047), size=(29, 17))
    assert pix.min() < 0
    with pytest.raises(ValueError, match="signed"):
        eng.decode_tensor(c.data, size=(29, 17), mean=0.1, std=0.5)
    with pytest.raises(ValueError, match="not both"):
        eng.decode_tensor(c.data, size=(29, 17), mean=0.1, scale=2.0)


# ---------------------------------------------------------------- 6. sticky settings
def test_sticky_settings_are_honoured(eng, cases):
    for layout in LAYOUTS:
        check(eng, cases["sycc420"], "float16", layout, affine=("ms", MEAN, STD, None), size=(23, 11))
        check(eng, cases["rgb12_8S"], "bfloat16", layout, affine=("ms", MEAN, STD, None), size=(20, 11))   # unit: 255, not 4095
    with settings(eng, precision="8S"):
        a = eng.decode_tensor(cases["rgb12_8S"].data, size=(20, 11), mean=0.0, std=1.0)
    assert 0.5 < a.max() <= 1.0


# ---------------------------------------------------------------- 7. every 16-bit value
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_16_bit_value(eng, cases, dtype):
    """The conversion's rounding over its whole input range.  float32 and bfloat16 take mean 0.485,
    std 0.229.  Under those the value nearest the mean gives 3.3e-5, below float16's smallest normal
    (6.1e-5), which the rule leaves to the device's float mode; float16 takes std 0.1, whose steps of
    1.5e-4 keep the two values beside the mean at 7.2e-5 and 8.0e-5 (tensor_ref asserts it)."""
    std = 0.1 if dtype == "float16" else 0.229
    got, pix = check(eng, cases["ramp16"], dtype, "chw", affine=("ms", 0.485, std, None), size=(256, 256))
    np.testing.assert_array_equal(pix.reshape(-1), np.arange(65536))
    # (host output where numpy has the type)
    check(eng, cases["ramp16"], dtype, "hwc", device=dtype == "bfloat16", affine=("ms", 0.485, std, None), size=(256, 256))


# ---------------------------------------------------------------- 8. above 2^24
def test_int_to_float_rounds_to_even(eng, cases):
    got, pix = check(eng, cases["big25"], "float32", "chw", size=(16, 16))
    assert eng.view_result.prec == 25
    flat, g = pix.reshape(-1).astype(np.int64), got.cpu().numpy().reshape(-1).astype(np.float64)
    assert flat[:6].tolist() == [2 ** 24 + k for k in (1, 3, 5, 7, 9, 11)] and flat[255] == 2 ** 25 - 1
    assert g[:6].tolist() == [2 ** 24 + k for k in (0, 4, 4, 8, 8, 12)]          # ties go to the even neighbour
    assert g[6:12].tolist() == [2 ** 24 - k for k in (1, 3, 5, 7, 9, 11)]        # below 2^24: exact
    assert g[255] == 2 ** 25
    check(eng, cases["big25"], "bfloat16", "hwc", affine=("ms", 0.5, 0.25, None), size=(16, 16))


# ---------------------------------------------------------------- 9. one image of a batch
def test_batch_slices_leave_the_rest_alone(eng, cases):
    c = cases["rgb"]
    H, W, kw = 13, 20, dict(size=(20, 13), mean=MEAN, std=STD)
    with settings(eng):
        pix = eng.decode_view(c.data, size=(20, 13))
    scale, bias = G._tensor_affine(MEAN, STD, None, 8, False)
    # (N, C, H + 2, W + 3) bfloat16
    buf = torch.full((3, 3, H + 2, W + 3), NAN16, dtype=torch.int16, device="cuda")
    batch = buf.view(torch.bfloat16)
    eng.decode_tensor(c.data, out=batch[1, :, :H, :W], **kw)
    want = np.full(buf.shape, NAN16, np.uint16)
    want[1, :, :H, :W] = T.apply(pix, scale, bias, "bfloat16", "chw")
    np.testing.assert_array_equal(buf.cpu().numpy().view(np.uint16), want)
    # (N, H + 2, W + 3, C) float16
    buf = torch.full((3, H + 2, W + 3, 3), NAN16, dtype=torch.int16, device="cuda")
    batch = buf.view(torch.float16)
    eng.decode_tensor(c.data, out=batch[1, :H, :W, :], layout="hwc", **kw)
    want = np.full(buf.shape, NAN16, np.uint16)
    want[1, :H, :W, :] = T.bits(T.apply(pix, scale, bias, "float16", "hwc"))
    np.testing.assert_array_equal(buf.cpu().numpy().view(np.uint16), want)
    # a channels_last image: shape (C, H, W), strides of (H, W, C)
    x = torch.full((1, 3, H, W), float("nan"), dtype=torch.float32, device="cuda").contiguous(memory_format=torch.channels_last)
    assert x[0].stride() == (1, 3 * W, 3)
    eng.decode_tensor(c.data, out=x[0], **kw)
    np.testing.assert_array_equal(tensor_bits(x[0]), T.bits(T.apply(pix, scale, bias, "float32", "chw")))


# ---------------------------------------------------------------- 10. host output
def test_host_output_equals_device_output(eng, cases):
    for case, dtype, layout, view in ((cases["rgb"], "float32", "chw", dict(size=(29, 17), rotate=90)),
                                      (cases["tiled"], "float16", "hwc", dict(region=(5, 3, 61, 44), size=(25, 17), mirror=True))):
        dev, _ = check(eng, case, dtype, layout, affine=("ms", MEAN, STD, None), **view)
        host, _ = check(eng, case, dtype, layout, device=False, affine=("ms", MEAN, STD, None), **view)
        np.testing.assert_array_equal(T.bits(host), tensor_bits(dev))
    d = torch.from_numpy(np.frombuffer(cases["rgb"].data, np.uint8).copy()).cuda()      # device bytes in: sized by the binding's rule
    got = eng.decode_tensor(d, length=len(cases["rgb"].data), dtype="float16", mean=MEAN, std=STD, size=(29, 17), rotate=90)
    np.testing.assert_array_equal(T.bits(got), T.bits(eng.decode_tensor(cases["rgb"].data, dtype="float16", mean=MEAN, std=STD, size=(29, 17), rotate=90)))
    with pytest.raises(ValueError, match="bfloat16"):
        eng.decode_tensor(cases["rgb"].data, dtype="bfloat16", size=(29, 17))


def test_timings_hold_the_tensor_pass(eng, cases):
    eng.decode_tensor(cases["tiled"].data, size=(40, 30))
    t = eng.timings()
    assert 0 < t.mct_ms <= t.total_ms


# ---------------------------------------------------------------- 11. refusals
def test_refusals_name_their_cause_and_leave_the_engine_alone(eng, cases):
    c = cases["rgb"]
    view_first = fresh(lambda e: e.decode_view(c.data, size=(20, 13)))
    plain_first = fresh(lambda e: e.decode(c.data))
    new = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")
    out = new(3, 13, 20)
    # the description
    for needle, kw in (("17 scale / bias entries", dict(scale=[1.0] * 17)),
                       ("scale entry 1 is not finite", dict(scale=[1.0, float("nan")])),
                       ("bias entry 0 is not finite", dict(bias=float("inf"))),
                       ("scale entry 0 is not finite", dict(mean=0.5, std=0.0)),
                       ("stride_c is 0", dict(out=new(1, 13, 20).expand(3, 13, 20))),
                       ("overlapping strides", dict(out=torch.as_strided(new(3 * 13 * 20), (3, 13, 20), (259, 20, 1)))),
                       ("overlapping strides", dict(out=torch.as_strided(new(3 * 13 * 20), (3, 13, 20), (1, 60, 2))))):
        kw.setdefault("out", out)
        with pytest.raises(RuntimeError, match=needle):
            eng.decode_tensor(c.data, size=(20, 13), **kw)
    # what the binding refuses itself
    for needle, kw in (("shape", dict(out=new(3, 20, 13))), ("shape", dict(out=new(13, 20, 3))), ("shape", dict(out=np.zeros((3, 13, 20), np.float32))),
                       ("dtype", dict(out=new(3, 13, 20, dtype=torch.int32))), ("dtype", dict(dtype="float64")), ("layout", dict(layout="nchw"))):
        with pytest.raises(ValueError, match=needle):
            eng.decode_tensor(c.data, size=(20, 13), **kw)
    # the raw call: no description, no data, an unknown dtype, a misaligned device pointer, a host tensor with padded rows
    b = np.frombuffer(c.data, np.uint8)
    v, res = G.View(0, 0, 0, 0, 20, 13, 0, 0, 0), G.ViewResult()
    raw = torch.zeros(3 * 13 * 20 * 4 + 8, dtype=torch.uint8, device="cuda")
    host = np.zeros(3 * 13 * 23, np.float32)

    def call(t):
        rc = eng.lib.gk_decode_view_tensor(eng.ctx, ctypes.c_void_p(b.ctypes.data), len(b), 0, ctypes.byref(v),
                                           ctypes.byref(t) if t is not None else None, ctypes.byref(res))
        return rc, eng.lib.gk_last_error(eng.ctx).decode()

    for needle, t in (("no description", None), ("no data", G.Tensor(None, 1, 1, 260, 20, 1, 0, None, None)),
                      ("dtype 7", G.Tensor(raw.data_ptr(), 1, 7, 260, 20, 1, 0, None, None)),
                      ("not aligned", G.Tensor(raw[1:].data_ptr(), 1, 1, 260, 20, 1, 0, None, None)),
                      ("not aligned", G.Tensor(raw[1:].data_ptr(), 1, 3, 260, 20, 1, 0, None, None)),
                      ("n = 2 without scale", G.Tensor(raw.data_ptr(), 1, 1, 260, 20, 1, 2, None, None)),
                      ("stride_y is -20", G.Tensor(raw.data_ptr(), 1, 1, 260, -20, 1, 0, None, None)),
                      ("must be dense", G.Tensor(host.ctypes.data, 0, 1, 13 * 23, 23, 1, 0, None, None))):
        rc, err = call(t)
        assert rc != 0 and needle in err, (needle, err)
    assert not raw.any() and not host.any() and res.pix_w == 0
    # the settings
    eng.set_decode_render("window", windows=[(0, 255)])
    try:
        with pytest.raises(RuntimeError, match="gk_set_decode_render is set: clear it"):
            eng.decode_tensor(c.data, size=(20, 13), out=out)
        assert eng.decode_view(c.data, size=(20, 13), sample_bytes=1).dtype == np.uint8   # still set
    finally:
        eng.set_decode_render(None)
    eng.set_decode_reduce(1)
    try:
        with pytest.raises(RuntimeError, match="gk_set_decode_reduce"):
            eng.decode_tensor(c.data, size=(5, 5))
        assert np.asarray(eng.decode(c.data)).shape == (3, 19, 27)   # the sticky level is still 1
    finally:
        eng.set_decode_reduce(0)
    # everything the view refuses
    for needle, kw in (("rotate 45", dict(size=(5, 5), rotate=45)), ("empty or leaves", dict(region=(0, 0, 54, 37), size=(1, 1))),
                       ("upscaling", dict(size=(54, 37))), ("upscaling", dict(width=60))):
        with pytest.raises(RuntimeError, match=needle):
            eng.decode_tensor(c.data, **kw)
    with pytest.raises(RuntimeError, match="both 0"):
        _both_zero(eng, b, raw)
    with pytest.raises(RuntimeError, match="GK_DISPLAY_UPSAMPLE"):
        eng.decode_tensor(cases["sycc420"].data, size=(8, 4))
    many = encode(eng, C.random_planes(16, 8, [(1, 1)] * 17, 8, seed=93), 8, numresolution=2)
    with pytest.raises(RuntimeError, match="planar calls"):
        eng.decode_tensor(many, size=(4, 4))
    planes = np.stack(C.random_planes(64, 48, C.S444, 8, seed=95)).astype(np.int32)
    p = G.default_params(numresolution=3, mct=False, tiles=(32, 32))
    part = eng.main_header(planes.shape, 8, params=p)[0] + eng.encode_tiles(planes, 8, 0, 2, params=p)[0] + b"\xff\xd9"
    with pytest.raises(RuntimeError, match="only some of its tiles"):
        eng.decode_tensor(part, size=(20, 20))
    assert not out.any()
    # after all of them: a view and a plain decode are a fresh engine's
    np.testing.assert_array_equal(eng.decode_view(c.data, size=(20, 13)), view_first)
    np.testing.assert_array_equal(eng.decode(c.data), plain_first)


def _both_zero(eng, b, raw):
    """Both sizes 0 reach the engine only through the raw call (the binding fills in the region's own)."""
    v, res = G.View(0, 0, 0, 0, 0, 0, 0, 0, 0), G.ViewResult()
    t = G.Tensor(raw.data_ptr(), 1, 1, 260, 20, 1, 0, None, None)
    if eng.lib.gk_decode_view_tensor(eng.ctx, ctypes.c_void_p(b.ctypes.data), len(b), 0, ctypes.byref(v), ctypes.byref(t), ctypes.byref(res)) != 0:
        raise RuntimeError(eng.lib.gk_last_error(eng.ctx).decode())


# ---------------------------------------------------------------- 12. history
def test_tensor_after_a_dense_decode(eng, cases):
    big = encode(eng, C.random_planes(300, 200, C.S444, 12, seed=111), 12, numresolution=4)
    c = cases["tiled"]
    kw = dict(region=(5, 3, 61, 44), size=(25, 17), rotate=90, dtype="float16", mean=MEAN, std=STD)
    alone = fresh(lambda e: e.decode_tensor(c.data, **kw))
    eng.decode(big)
    np.testing.assert_array_equal(T.bits(eng.decode_tensor(c.data, **kw)), T.bits(alone))


def test_plain_decodes_after_a_tensor(eng, cases):
    c, o = cases["tiled"], cases["rgb"]
    planar = fresh(lambda e: e.decode(c.data))
    pixels = fresh(lambda e: e.decode_pixels(o.data, sample_bytes=1))
    view = fresh(lambda e: e.decode_view(c.data, region=(5, 3, 61, 44), size=(25, 17)))
    eng.decode_tensor(c.data, region=(5, 3, 61, 44), size=(14, 10), rotate=270, mirror=True, mean=MEAN, std=STD)
    assert eng.view_result.reduce == 2
    np.testing.assert_array_equal(eng.decode(c.data), planar)                       # full resolution again
    eng.decode_tensor(o.data, size=(13, 9), dtype="float16")
    np.testing.assert_array_equal(eng.decode_pixels(o.data, sample_bytes=1), pixels)
    eng.decode_tensor(c.data, size=(16, 12), layout="hwc")
    np.testing.assert_array_equal(eng.decode_view(c.data, region=(5, 3, 61, 44), size=(25, 17)), view)
