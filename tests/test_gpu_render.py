"""The render stage and the levels call on the GPU (k_render, k_levels: gk_render.hip).

Truth for a render: tests/render_ref.py (numpy int64) applied to what the same call on the same
engine returns with no render and sample_bytes 0; for the levels: numpy on the int32 pixels the same
view returns.  Every comparison is exact.  Streams are written by the engine's encoder at the sizes
used here; one case starts from the oracle's decode instead."""
import numpy as np
import pytest
import torch

import grok_amd as G
import oracle as O
import pixels_ref as P
import render_ref as R
import view_ref as V

pytestmark = pytest.mark.gpu

RAMP = np.stack([np.arange(256), 255 - np.arange(256), (np.arange(256) * 7) % 256], axis=1).astype(np.uint8)
SIGMOID = np.floor(255.0 / (1.0 + np.exp(-(np.arange(256) - 127.5) / 24.0)) + 0.5).astype(np.uint8)


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


def noise(c, h, w, prec, seed=1, signed=False):
    lo, hi = (-(1 << (prec - 1)), 1 << (prec - 1)) if signed else (0, 1 << prec)
    return np.random.default_rng(seed).integers(lo, hi, size=(c, h, w)).astype(np.int32)


def encode(e, img, prec, signed=False, **kw):
    kw.setdefault("mct", False)
    kw.setdefault("numresolution", 1 if min(img.shape[1:]) < 4 else 3)
    return e.encode(np.ascontiguousarray(img, np.int32), prec, signed=signed, params=G.default_params(**kw))


@pytest.fixture(scope="module")
def streams(eng):
    s = {}
    for w, h in ((1, 1), (16, 16), (17, 5), (67, 93)):
        s["u12_%dx%d" % (w, h)] = encode(eng, noise(1, h, w, 12, seed=w), 12)
    for c in (1, 2, 3, 4, 5, 16):
        s["c%d" % c] = encode(eng, noise(c, 19, 21, 12, seed=10 + c), 12)
    s["u16"] = encode(eng, noise(1, 31, 45, 16, seed=3), 16)
    s["s16"] = encode(eng, noise(1, 31, 45, 16, seed=4, signed=True), 16, signed=True)
    s["s16c2"] = encode(eng, noise(2, 17, 33, 16, seed=5, signed=True), 16, signed=True)
    s["every16"] = encode(eng, np.random.default_rng(6).permutation(65536).reshape(1, 256, 256), 16, numresolution=4)
    s["view"] = encode(eng, noise(3, 75, 100, 12, seed=7), 12, numresolution=4)
    s["const"] = encode(eng, np.full((1, 64, 80), 1234), 12)
    return s


def rendered(e, call, **render):
    """(the call's int32 pixels without a render, its bytes under `render`) on one engine."""
    e.set_decode_render(None)
    ref = call(e, 0)
    e.set_decode_render(**render)
    try:
        got = call(e, 1)
    finally:
        e.set_decode_render(None)
    assert ref.dtype == np.int32 and got.dtype == np.uint8
    return ref, got


def check(e, call, **render):
    ref, got = rendered(e, call, **render)
    want = R.render(ref, render["mode"], render["windows"], render.get("tints"),
                    render.get("curve") if "gamma" not in render else R.gamma_curve(render["gamma"]), render.get("map"))
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    return ref, got


def pixels(cs, **kw):
    return lambda e, sb: e.decode_pixels(cs, sample_bytes=sb, **kw)


def view(cs, **kw):
    return lambda e, sb: e.decode_view(cs, sample_bytes=sb, **kw)


# ---------------------------------------------------------------- 1. sizes, channel counts, depths
@pytest.mark.parametrize("w,h", [(1, 1), (16, 16), (17, 5), (67, 93)])
def test_sizes_through_every_pixel_call(eng, streams, w, h):
    cs = streams["u12_%dx%d" % (w, h)]
    check(eng, pixels(cs), mode="window", windows=[(300, 3000)])
    win = (w // 3, h // 3, w, h - h // 4)
    check(eng, pixels(cs, window=win), mode="window", windows=[(3000, 300)], curve=SIGMOID)
    check(eng, view(cs, size=(w, h)), mode="blend", windows=[(0, 4095)], tints=[(255, 128, 1)])
    check(eng, view(cs, size=(max(1, (2 * w) // 3), max(1, (3 * h) // 4))), mode="map", windows=[(100, 4000)], map=RAMP)


@pytest.mark.parametrize("c", [1, 2, 3, 4, 5, 16])
def test_channel_counts(eng, streams, c):
    cs = streams["c%d" % c]
    wins = [(100 * k, 4095 - 150 * k) if k % 3 else (4095 - 10 * k, 17 * k) for k in range(c)]
    tints = [((37 * k) % 256, (91 * k + 5) % 256, (200 - 13 * k) % 256) for k in range(c)]
    for call in (pixels(cs), pixels(cs, window=(2, 3, 21, 17)), view(cs, size=(13, 11)), view(cs, size=(21, 19), rotate=180)):
        _, got = check(eng, call, mode="window", windows=wins)
        assert got.shape[2] == c
        _, got = check(eng, call, mode="blend", windows=wins, tints=tints)
        assert got.shape[2] == 3
    # fewer entries than channels: the last one serves the rest
    check(eng, pixels(cs), mode="window", windows=wins[:2])


def test_depths_and_signed_windows(eng, streams):
    check(eng, pixels(streams["c1"]), mode="window", windows=[(0, 4095)])
    check(eng, pixels(streams["u16"]), mode="window", windows=[(0, 65535)])
    check(eng, pixels(streams["u16"]), mode="window", windows=[(1000, 4000)], gamma=2.2)
    for wins in ([(-32768, 32767)], [(-20000, -1000)], [(-1, 0)], [(5000, -5000)], [(-2 ** 31, 2 ** 31 - 1)]):
        check(eng, pixels(streams["s16"]), mode="window", windows=wins)
        check(eng, view(streams["s16"], size=(29, 23)), mode="window", windows=wins)
    check(eng, view(streams["s16c2"], size=(20, 11)), mode="blend", windows=[(-30000, 100), (200, -200)],
          tints=[(255, 0, 64), (0, 255, 64)])


def test_every_16_bit_value_once(eng, streams):
    cs = streams["every16"]
    ref, got = check(eng, pixels(cs), mode="window", windows=[(0, 65535)])
    assert np.array_equal(np.sort(ref.ravel()), np.arange(65536))   # lossless: every value once
    assert np.bincount(got.ravel(), minlength=256).min() >= 128     # every display level is used
    check(eng, pixels(cs), mode="window", windows=[(60000, 1000)])
    check(eng, pixels(cs), mode="window", windows=[(20000, 20001)], curve=SIGMOID)
    check(eng, pixels(cs), mode="map", windows=[(123, 54321)], curve=SIGMOID, map=RAMP)


def test_windows_outside_the_data(eng, streams):
    for wins, level in (([(5000, 9000)], 0), ([(-900, -100)], 255), ([(9000, 5000)], 255), ([(-100, -900)], 0)):
        _, got = check(eng, pixels(streams["c3"]), mode="window", windows=wins)
        assert (got == level).all()


def test_map_and_blend(eng, streams):
    check(eng, pixels(streams["c1"]), mode="map", windows=[(0, 4095)], map=RAMP)
    check(eng, view(streams["c1"], size=(10, 9), rotate=270), mode="map", windows=[(4095, 0)], map=RAMP, gamma=0.5)
    # white on one channel: grey as RGB
    ref, got = check(eng, pixels(streams["c1"]), mode="blend", windows=[(0, 4095)], tints=[(255, 255, 255)])
    assert (got[:, :, 0] == got[:, :, 1]).all() and (got[:, :, 0] == R.level(ref[:, :, 0], 0, 4095)).all()
    # two channels on one colour saturate
    _, got = check(eng, pixels(streams["c2"]), mode="blend", windows=[(0, 2000)], tints=[(255, 0, 0), (255, 40, 0)])
    assert (got[:, :, 0] == 255).any() and (got[:, :, 0] < 255).any() and (got[:, :, 2] == 0).all()
    # a channel left out by a zero tint
    check(eng, pixels(streams["c3"]), mode="blend", windows=[(0, 4095)], tints=[(255, 0, 0), (0, 0, 0), (0, 0, 255)])


# ---------------------------------------------------------------- 2. views
@pytest.mark.parametrize("kw", [dict(size=(37, 29)), dict(size=(1, 40)), dict(size=(50, 1)), dict(size=(37, 29), rotate=90, mirror=True),
                                dict(region=(10, 5, 90, 70), width=33, rotate=270), dict(size=(100, 75), mirror=True),
                                dict(size=(12, 9))],
                         ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()).replace(" ", ""))
def test_views(eng, streams, kw):
    cs = streams["view"]   # 100 x 75, three channels
    ref, got = check(eng, view(cs, **kw), mode="window", windows=[(0, 4095), (500, 600), (4000, 100)])
    vr = eng.view_result
    assert (vr.pix_h, vr.pix_w, vr.channels, vr.prec, vr.sgnd) == got.shape + (8, 0)
    check(eng, view(cs, **kw), mode="blend", windows=[(0, 4095)], tints=[(255, 0, 0), (0, 255, 0), (90, 90, 255)], curve=SIGMOID)


def test_from_the_oracles_decode(eng, streams):
    planes, prec = O.decode(streams["view"])
    assert prec == 12
    pix = P.pack(list(planes))                                   # (75, 100, 3), what decode_pixels returns
    wins, tints = [(200, 3900), (3000, 1000), (0, 4095)], [(255, 10, 0), (0, 255, 10), (10, 0, 255)]
    eng.set_decode_render("blend", wins, tints, gamma=1.8)
    try:
        got_pix = eng.decode_pixels(streams["view"])
        got_view = eng.decode_view(streams["view"], size=(67, 51), rotate=90)     # no resolution is discarded: 67 > 50
    finally:
        eng.set_decode_render(None)
    assert eng.view_result.reduce == 0
    np.testing.assert_array_equal(got_pix, R.render(pix, "blend", wins, tints, R.gamma_curve(1.8)))
    np.testing.assert_array_equal(got_view, R.render(V.view(pix, 67, 51, 90, False), "blend", wins, tints, R.gamma_curve(1.8)))


# ---------------------------------------------------------------- 3. output buffers
@pytest.mark.parametrize("how", ["pixels", "window", "view"])
def test_device_output_with_padded_rows(eng, streams, how):
    cs = streams["c5"]   # 21 x 19
    call = {"pixels": pixels(cs), "window": pixels(cs, window=(1, 2, 20, 18)), "view": view(cs, size=(13, 11), rotate=90)}[how]
    wins = [(0, 4095), (4095, 0), (1000, 1100)]
    for mode, cout in (("window", 5), ("blend", 3)):
        render = dict(mode=mode, windows=wins, tints=[(200, 100, 50), (0, 0, 0), (50, 100, 200)] if mode == "blend" else None)
        ref, host = check(eng, call, **render)
        h, w = host.shape[:2]
        pad = 13
        buf = torch.full((h, w * cout + pad), 0xAB, dtype=torch.uint8, device="cuda")
        out = torch.as_strided(buf, (h, w, cout), (w * cout + pad, cout, 1))
        eng.set_decode_render(**render)
        try:
            if how == "view":
                eng.decode_view(cs, size=(13, 11), rotate=90, out=out)
            else:
                eng.decode_pixels(cs, out=out, window=None if how == "pixels" else (1, 2, 20, 18))
        finally:
            eng.set_decode_render(None)
        full = buf.cpu().numpy()
        np.testing.assert_array_equal(full[:, :w * cout].reshape(h, w, cout), host)
        assert (full[:, w * cout:] == 0xAB).all()   # bytes past the row are never written


def test_buffer_refusals(eng, streams):
    cs = streams["c3"]
    b = np.frombuffer(cs, np.uint8)
    out = np.zeros(19 * 21 * 3 * 4, np.uint8)
    eng.set_decode_render("window", [(0, 4095)])
    try:
        for sb in (0, 2, 4):
            assert eng.lib.gk_decode_pixels(eng.ctx, b.ctypes.data, len(b), 0, out.ctypes.data, 21 * 3 * 4, sb, 0) != 0
            assert "sample_bytes must be 1" in eng.lib.gk_last_error(eng.ctx).decode()
        assert eng.lib.gk_decode_pixels(eng.ctx, b.ctypes.data, len(b), 0, out.ctypes.data, 21 * 3 - 1, 1, 0) != 0
        assert "row_bytes 62 is below" in eng.lib.gk_last_error(eng.ctx).decode()
        eng.set_decode_render("map", [(0, 4095)], map=RAMP)
        with pytest.raises(RuntimeError, match="map mode on 3 output channels"):
            eng.decode_pixels(cs)
    finally:
        eng.set_decode_render(None)
    assert not out.any()


# ---------------------------------------------------------------- 4. levels
def check_levels(eng, cs, bins, origin=None, shift=None, **kw):
    size_kw = {k: v for k, v in kw.items() if k in ("region", "size", "width", "height", "fit")}
    pix = eng.decode_view(cs, sample_bytes=0, **size_kw) if size_kw else eng.decode_pixels(cs)
    lv = eng.levels(cs, bins=bins, origin=origin, shift=shift, **size_kw)
    c = pix.shape[2]
    assert len(lv.min) == c
    want = R.stats(pix, bins, list(zip(lv.origin, lv.shift)))
    for k in range(c):
        assert (lv.min[k], lv.max[k], lv.sum[k], lv.count[k]) == (want[k]["min"], want[k]["max"], want[k]["sum"], want[k]["count"])
        if bins:
            np.testing.assert_array_equal(lv.hist[k], want[k]["hist"])
            assert int(lv.hist[k].sum()) == pix.shape[0] * pix.shape[1]
    return lv, pix


def test_levels_noise_and_sizes(eng, streams):
    lv, pix = check_levels(eng, streams["u12_67x93"], 4096)
    assert lv.shift == [0] and lv.origin == [int(pix.min())]
    check_levels(eng, streams["u12_67x93"], 4096, size=(33, 17))
    check_levels(eng, streams["u12_17x5"], 256, origin=0, shift=4)
    check_levels(eng, streams["u12_1x1"], 16)
    check_levels(eng, streams["view"], 512, region=(10, 5, 90, 70), width=33)
    check_levels(eng, streams["view"], 0, size=(37, 29))


def test_levels_constant_image(eng, streams):
    lv, _ = check_levels(eng, streams["const"], 4096, origin=0, shift=0)
    assert lv.hist[0][1234] == 64 * 80 and lv.min == lv.max == [1234]
    lv, _ = check_levels(eng, streams["const"], 4096, size=(33, 17))
    assert lv.hist[0][0] == 33 * 17 and lv.origin == [1234]


def test_levels_signed_shift_and_end_bins(eng, streams):
    lv, _ = check_levels(eng, streams["s16"], 1024, origin=-32768, shift=6)        # a negative origin, 64 values a bin
    assert lv.hist[0][:512].sum() > 0 and lv.hist[0][512:].sum() > 0
    lv, pix = check_levels(eng, streams["s16"], 64, origin=-4096, shift=7)         # -4096 .. 4095: both end bins take the rest
    assert lv.hist[0][0] >= (pix < -4096).sum() > 0 and lv.hist[0][63] >= (pix > 4095).sum() > 0
    check_levels(eng, streams["s16c2"], 4096, origin=[-32768, -100], shift=[4, 0], size=(20, 11))
    check_levels(eng, streams["s16"], 4096, origin=-2 ** 31, shift=31)             # two bins: below 0, from 0
    check_levels(eng, streams["s16"], 4096, origin=2 ** 31 - 1, shift=0)           # everything below the origin: bin 0


def test_levels_channels_and_bin_counts(eng, streams):
    for bins in (1, 4096):
        check_levels(eng, streams["c5"], bins)
        check_levels(eng, streams["c5"], bins, size=(13, 11))
    check_levels(eng, streams["c16"], 64, origin=0, shift=6)
    check_levels(eng, streams["c4"], 4096)


def test_levels_two_calls_on_16_bits(eng, streams):
    lv, pix = check_levels(eng, streams["every16"], 4096)
    assert (lv.min, lv.max, lv.origin, lv.shift) == ([0], [65535], [0], [4]) and (lv.hist[0] == 16).all()
    assert lv.window(0, 1000) == [(0, 65535)] and lv.window(500, 500) == [(32752, 32767)]
    assert lv.window(10, 990) == [R.percentile_window(lv.hist[0], 0, 4, 10, 990)]
    lv, _ = check_levels(eng, streams["s16"], 4096)
    assert lv.origin == lv.min and lv.shift == [4]
    # a window chosen from the data, then used
    lo, hi = lv.window(20, 980)[0]
    _, got = check(eng, pixels(streams["s16"]), mode="window", windows=[(lo, hi)])
    assert got.min() == 0 and got.max() == 255


def test_levels_refusals(eng, streams):
    cs = streams["c3"]
    with pytest.raises(RuntimeError, match="4097 bins"):
        eng.levels(cs, bins=4097)
    with pytest.raises(RuntimeError, match="shift of 32"):
        eng.levels(cs, bins=16, origin=0, shift=32)
    with pytest.raises(RuntimeError, match="upscaling"):
        eng.levels(cs, bins=16, size=(50, 50))
    b = np.frombuffer(cs, np.uint8)
    v = G.View(0, 0, 0, 0, 21, 19, 0, 0, 0)
    st, hist = (G.ChannelLevels * 16)(), np.zeros(3 * 16, np.uint64)
    assert eng.lib.gk_decode_levels(eng.ctx, b.ctypes.data, len(b), 0, v, None, 0, 16, st, hist.ctypes.data, 47, None) != 0
    assert "hist_cap 47 is below channels * bins = 48" in eng.lib.gk_last_error(eng.ctx).decode()
    assert eng.lib.gk_decode_levels(eng.ctx, b.ctypes.data, len(b), 0, v, None, 0, 16, st, None, 0, None) != 0
    assert not hist.any()
    eng.set_decode_reduce(1)
    try:
        with pytest.raises(RuntimeError, match="gk_set_decode_reduce is set"):
            eng.levels(cs, bins=16)
    finally:
        eng.set_decode_reduce(0)


# ---------------------------------------------------------------- 5. history
def test_set_decode_clear_decode(eng, streams):
    cs = streams["c3"]
    want_plain = fresh(lambda e: (e.decode_pixels(cs), e.decode_view(cs, size=(13, 11)), e.decode(cs)))
    eng.set_decode_render("blend", [(0, 4095)], tints=[(255, 0, 0), (0, 255, 0), (0, 0, 255)])
    a = eng.decode_pixels(cs)
    eng.set_decode_render(None)
    assert a.dtype == np.uint8
    for got, want in zip((eng.decode_pixels(cs), eng.decode_view(cs, size=(13, 11)), eng.decode(cs)), want_plain):
        assert got.dtype == want.dtype
        np.testing.assert_array_equal(got, want)


def test_refused_description_keeps_the_previous_one(eng, streams):
    cs = streams["c3"]
    eng.set_decode_render("window", [(100, 3000)])
    try:
        want = eng.decode_pixels(cs)
        for bad in (dict(mode="window", windows=[(0, 5), (7, 7)]), dict(mode="map", windows=[(0, 5)]),
                    dict(mode="blend", windows=[(0, 5)], tints=[(0, 0, 0)]), dict(mode="window", windows=[])):
            with pytest.raises(RuntimeError, match="render: "):
                eng.set_decode_render(**bad)
            np.testing.assert_array_equal(eng.decode_pixels(cs), want)
    finally:
        eng.set_decode_render(None)
    np.testing.assert_array_equal(want, R.render(eng.decode_pixels(cs), "window", [(100, 3000)]))


def test_planar_calls_refuse_under_a_render(eng, streams):
    cs = streams["c3"]
    want = fresh(lambda e: (e.decode(cs), e.decode_window(cs, (2, 3, 20, 17))))
    eng.set_decode_render("window", [(0, 4095)])
    try:
        with pytest.raises(RuntimeError, match="gk_decode: gk_set_decode_render is set"):
            eng.decode(cs)
        with pytest.raises(RuntimeError, match="gk_decode_window: gk_set_decode_render is set"):
            eng.decode_window(cs, (2, 3, 20, 17))
    finally:
        eng.set_decode_render(None)
    np.testing.assert_array_equal(eng.decode(cs), want[0])
    np.testing.assert_array_equal(eng.decode_window(cs, (2, 3, 20, 17)), want[1])


def test_levels_between_two_decodes(eng, streams):
    cs, other = streams["view"], streams["s16c2"]
    render = dict(mode="window", windows=[(0, 4095), (4095, 0)], curve=SIGMOID)
    eng.set_decode_render(**render)
    try:
        a = eng.decode_view(cs, size=(37, 29), rotate=90)
        lv = eng.levels(other, bins=4096, size=(20, 11))       # another stream, under the render, which it ignores
        b = eng.decode_view(cs, size=(37, 29), rotate=90)
        c = eng.decode_pixels(cs)
    finally:
        eng.set_decode_render(None)
    np.testing.assert_array_equal(a, b)
    plain = eng.decode_view(other, size=(20, 11))
    assert lv.min == [int(plain[:, :, k].min()) for k in range(2)] and lv.count == [220, 220]
    want = fresh(lambda e: (e.set_decode_render(**render), e.decode_view(cs, size=(37, 29), rotate=90), e.decode_pixels(cs))[1:])
    np.testing.assert_array_equal(a, want[0])
    np.testing.assert_array_equal(c, want[1])


def test_header_calls_describe_the_output(eng, streams):
    cs = streams["c5"]
    info = eng.read_header(cs)
    assert (info.numcomps, info.prec, info.sgnd) == (5, 12, 0)
    eng.set_decode_render("window", [(0, 4095)])
    try:
        info = eng.read_header(cs)
        assert (info.numcomps, info.prec, info.sgnd, info.w, info.h) == (5, 8, 0, 21, 19)
        assert eng.precisions() == [(8, False)] * 5 and eng.subsampling() == [(1, 1)] * 5
        eng.set_decode_render("blend", [(0, 4095)], tints=[(1, 2, 3)])
        info = eng.read_header(cs)
        assert (info.numcomps, info.prec, info.sgnd) == (3, 8, 0)
        assert eng.precisions() == [(8, False)] * 3
        ci = eng.colour_info()
        assert (ci.colour_space, ci.num_channels) == (2, 3) and list(ci.asoc[:3]) == [1, 2, 3]
        eng.set_decode_render("map", [(0, 4095)], map=RAMP)
        with pytest.raises(RuntimeError, match="map mode on 5 output channels"):
            eng.read_header(cs)
        info = eng.read_header(streams["s16"])
        assert (info.numcomps, info.prec, info.sgnd) == (3, 8, 0)
    finally:
        eng.set_decode_render(None)
    info = eng.read_header(streams["s16"])
    assert (info.numcomps, info.prec, info.sgnd) == (1, 16, 1)
    assert eng.colour_info().num_channels == 1
