"""The output stage on the GPU (k_pixels, gk_pixels.hip): forced precision, grey to RGB and packed
(H, W, C) pixels through Engine.decode_pixels and, for the precision list, the planar decode.

Truth: tests/pixels_ref.py applied to the same engine's planar decode of the same bytes under the
same rgb / upsample flags, with no list and no force_rgb (those decodes are pinned to the oracle
and to display_ref by the other suites).  Inputs are lossless 5/3 streams from eng.encode unless a
test says otherwise."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import grok_amd as G
import display_ref as R
import display_cases as C
import jp2_boxes as J
import pixels_ref as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = G.Engine(0)
    yield e
    e.close()


@contextlib.contextmanager
def settings(eng, rgb=False, upsample=False, force_rgb=False, precision=None):
    eng.set_decode_display(rgb=rgb, upsample=upsample, force_rgb=force_rgb)
    eng.set_decode_precision(precision)
    try:
        yield
    finally:
        eng.set_decode_display()
        eng.set_decode_precision(None)


def encode(eng, planes, prec, signed=False, sub=None, origin=None, size=None, **kw):
    if sub is None or all(d == (1, 1) for d in sub):
        h, w = planes[0].shape
        kw.setdefault("numresolution", C.numres_for(w, h, [(1, 1)]))
        kw.setdefault("mct", False)
        return eng.encode(np.stack(planes).astype(np.int32), prec, signed=signed, params=G.default_params(**kw), origin=origin)
    kw.setdefault("numresolution", C.numres_for(size[0], size[1], sub))
    kw.setdefault("mct", False)
    return eng.encode([np.ascontiguousarray(p, np.int32) for p in planes], prec, signed=signed, params=G.default_params(**kw),
                      origin=origin, subsampling=sub, size=size)


def truth(eng, data, rgb=False, upsample=False, force_rgb=False, precision=None, window=None):
    """(planes, comps) the output stage must produce: the restatement on the planar decode."""
    with settings(eng, rgb=rgb, upsample=upsample):
        got = eng.decode(data) if window is None else eng.decode_window(data, window)
        comps = [(dx, dy, p, int(s)) for (dx, dy), (p, s) in zip(eng.subsampling(), eng.precisions())]
        cs = eng.colour_info().colour_space
    planes, comps, _ = P.finish(list(got), comps, cs, force_rgb, precision)
    return planes, comps


def dev(data):
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()


TORCH = {1: torch.uint8, 2: torch.int16, 0: torch.int32}
NP = {1: np.uint8, 2: np.uint16, 0: np.int32}


def bits(t, sb):
    """A device tensor's samples as the unsigned 8 / 16-bit or int32 numbers they hold."""
    return t.cpu().numpy().view(NP[sb])


# ---------------------------------------------------------------- 1. pack geometry
# (2051 columns: past the 256 * 8 columns of one workgroup, with a partial last group)
@pytest.mark.parametrize("w", [1, 7, 8, 9, 33, 2051])
@pytest.mark.parametrize("nc", [1, 2, 3, 4, 5])
def test_pack_geometry(eng, nc, w):
    h = 5
    for prec, sbs in ((8, (1,)), (12, (2, 0))):
        planes = C.random_planes(w, h, [(1, 1)] * nc, prec, seed=nc * 7 + w + prec)
        data = encode(eng, planes, prec)
        want = P.pack(planes)
        d = dev(data)
        for sb in sbs:
            es, fill = sb or 4, 77
            wnt = want.astype(NP[sb])
            got = eng.decode_pixels(data, sample_bytes=sb)                       # host array
            assert got.shape == (h, w, nc) and got.dtype == NP[sb]
            np.testing.assert_array_equal(got, wnt)
            y = torch.zeros((h, w, nc), dtype=TORCH[sb], device="cuda")          # tight rows (mostly unaligned)
            eng.decode_pixels(d, length=len(data), out=y)
            np.testing.assert_array_equal(bits(y, sb), wnt)
            row = -(-(w * nc * es) // 64) * 64 // es                             # rows padded to 64 bytes
            buf = torch.full((h, row), fill, dtype=TORCH[sb], device="cuda")
            eng.decode_pixels(d, length=len(data), out=buf[:, :w * nc].unflatten(1, (w, nc)))
            b = bits(buf, sb)
            np.testing.assert_array_equal(b[:, :w * nc].reshape(h, w, nc), wnt)
            assert (b[:, w * nc:] == fill).all()
            big = torch.full((h * w * nc + 2,), fill, dtype=TORCH[sb], device="cuda")   # base one sample off
            eng.decode_pixels(d, length=len(data), out=big[1:1 + h * w * nc].view(h, w, nc))
            b = bits(big, sb)
            np.testing.assert_array_equal(b[1:-1].reshape(h, w, nc), wnt)
            assert b[0] == fill and b[-1] == fill


# ---------------------------------------------------------------- 2. every value through every op
def _every(eng, side, prec, signed, spec, must=()):
    n = side * side
    v = np.arange(n, dtype=np.int64).reshape(side, side) - ((1 << (prec - 1)) if signed else 0)
    assert n == 1 << prec
    data = encode(eng, [v], prec, signed=signed)
    planes, comps = truth(eng, data, precision=spec)
    np.testing.assert_array_equal(np.asarray(eng.decode(data))[0], v)
    want = planes[0]
    for a, b in must:
        assert int(want[v == a][0]) == b
    newp = comps[0][2]
    sb = (newp + 7) // 8
    with settings(eng, precision=spec):
        assert eng.read_header(data).prec == newp
        for s in (sb, 0):
            dt = np.dtype(NP[s]) if not signed or s == 0 else np.dtype({1: np.int8, 2: np.int16}[s])
            got = eng.decode_pixels(data, sample_bytes=s)
            assert got.shape == (side, side, 1) and got.dtype == dt
            np.testing.assert_array_equal(got[:, :, 0], want.astype(dt))
            got = eng.decode(data, sample_bytes=s)                                # planar, under the list
            assert got.shape == (1, side, side) and got.dtype == dt
            np.testing.assert_array_equal(got[0], want.astype(dt))
    return want


@pytest.mark.parametrize("spec", ["8S", "8C"])
def test_every_16bit_value_down(eng, spec):
    want = _every(eng, 256, 16, False, spec)
    assert want.min() == 0 and want.max() == 255


def test_every_12bit_value_up(eng):
    _every(eng, 64, 12, False, "16S", must=[(1229, 19668), (4095, 65535)])
    _every(eng, 64, 12, False, "13S", must=[(2048, 4096), (2049, 4098)])


def test_every_8bit_value_up(eng):
    want = _every(eng, 16, 8, False, "16S")
    np.testing.assert_array_equal(want.ravel(), 257 * np.arange(256))


@pytest.mark.parametrize("spec,must", [("12S", [(-128, -2048), (-1, -16), (127, 2032)]),
                                       ("4S", [(-5, 0), (-16, -1), (-17, -1), (127, 7), (-128, -8)]),
                                       ("4C", [(-128, -8), (-9, -8), (-8, -8), (7, 7), (8, 7), (127, 7)])])
def test_every_signed_8bit_value(eng, spec, must):
    _every(eng, 16, 8, True, spec, must=must)


# ---------------------------------------------------------------- 3. per-channel lists
def test_per_channel_lists(eng):
    w, h = 33, 17
    planes = C.random_planes(w, h, C.S444, 12, seed=31)
    data = encode(eng, planes, 12)
    want, comps = truth(eng, data, precision="8S,12C,0S")
    assert [c[2] for c in comps] == [8, 12, 12]
    with settings(eng, precision="8S,12C,0S"):
        assert eng.read_header(data).prec == 12
        assert [p for p, _ in eng.precisions()] == [8, 12, 12]
        got = eng.decode_pixels(data, sample_bytes=2)
        assert got.dtype == np.uint16
        np.testing.assert_array_equal(got, P.pack(want))
        np.testing.assert_array_equal(eng.decode(data, sample_bytes=2), np.stack(want))
        with pytest.raises(RuntimeError, match="sample_bytes"):
            eng.decode_pixels(data, sample_bytes=1)
    want, comps = truth(eng, data, precision="8S")
    assert [c[2] for c in comps] == [8, 8, 8]
    with settings(eng, precision="8S"):
        assert eng.read_header(data).prec == 8
        got = eng.decode_pixels(data, sample_bytes=1)
        assert got.dtype == np.uint8 and got.shape == (h, w, 3)
        np.testing.assert_array_equal(got, P.pack(want))
        y = torch.zeros((3, h, w), dtype=torch.uint8, device="cuda")              # a 12-bit image into u8 planes
        eng.decode(data, out=y)
        np.testing.assert_array_equal(y.cpu().numpy(), np.stack(want))


# ---------------------------------------------------------------- 4. grey to RGB
def test_grey_to_rgb(eng):
    w, h = 33, 17
    g = C.random_planes(w, h, [(1, 1)] * 2, 8, seed=41)
    one, two = encode(eng, g[:1], 8), encode(eng, g, 8)
    with settings(eng, force_rgb=True):
        got = eng.decode_pixels(one, sample_bytes=1)
        assert got.shape == (h, w, 3)
        for k in range(3):
            np.testing.assert_array_equal(got[:, :, k], g[0])
        ci = eng.colour_info()
        assert (ci.colour_space, ci.display_applied, ci.num_channels) == (R.CS_SRGB, 4, 3)
        np.testing.assert_array_equal(eng.decode(one), np.stack([g[0]] * 3))      # planar: three planes
        got = eng.decode_pixels(two)
        assert got.shape == (h, w, 4) and got.dtype == np.int32
        np.testing.assert_array_equal(got, P.pack([g[0], g[0], g[0], g[1]]))
    g16 = C.random_planes(w, h, [(1, 1)], 16, seed=42)
    data = encode(eng, g16, 16)
    want, comps = truth(eng, data, force_rgb=True, precision="8S")
    assert len(want) == 3 and [c[2] for c in comps] == [8] * 3
    np.testing.assert_array_equal(want[0], g16[0] // 256)
    with settings(eng, force_rgb=True, precision="8S"):
        np.testing.assert_array_equal(eng.decode_pixels(data, sample_bytes=1), P.pack(want))
    rgb = encode(eng, C.random_planes(w, h, C.S444, 8, seed=43), 8)               # a raw 3-component stream
    with settings(eng, force_rgb=True):
        with pytest.raises(RuntimeError, match="unknown"):
            eng.decode_pixels(rgb)
        with pytest.raises(RuntimeError, match="unknown"):
            eng.decode(rgb)
        f = C.wrap(rgb, w, h, 3, 8, C.SRGB)                                      # ... in an sRGB file: as it is
        np.testing.assert_array_equal(eng.decode_pixels(f), P.pack(list(eng.decode(f))))


# ---------------------------------------------------------------- 5. after the other stages
def test_after_sycc420_conversion(eng):
    w, h, org = 33, 17, (1, 1)
    planes = C.random_planes(w, h, C.S420, 8, org, seed=51)
    f = C.wrap(encode(eng, planes, 8, sub=C.S420, origin=org, size=(w, h)), w, h, 3, 8, C.SYCC)
    want, _ = truth(eng, f, rgb=True)
    assert len(want) == 3 and want[0].shape == (h, w)
    with settings(eng, rgb=True):
        np.testing.assert_array_equal(eng.decode_pixels(f, sample_bytes=1), P.pack(want))
        y = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        eng.decode_pixels(dev(f), length=len(f), out=y)
        np.testing.assert_array_equal(y.cpu().numpy(), P.pack(want))
    want8, _ = truth(eng, f, rgb=True, precision="4S")
    with settings(eng, rgb=True, precision="4S"):
        np.testing.assert_array_equal(eng.decode_pixels(f), P.pack(want8))


def test_after_upsampling(eng):
    w, h = 33, 17
    planes = C.random_planes(w, h, C.S420, 8, seed=52)
    data = encode(eng, planes, 8, sub=C.S420, size=(w, h))
    want, _ = truth(eng, data, upsample=True)
    with settings(eng, upsample=True):
        np.testing.assert_array_equal(eng.decode_pixels(data, sample_bytes=1), P.pack(want))


def test_after_cmyk16_into_u8(eng):
    w, h = 37, 19
    planes = C.random_planes(w, h, [(1, 1)] * 4, 16, seed=53)
    f = C.wrap(encode(eng, planes, 16), w, h, 4, 16, C.CMYK)
    want, comps = truth(eng, f, rgb=True)
    assert len(want) == 3 and [c[2] for c in comps] == [8] * 3
    with settings(eng, rgb=True):
        got = eng.decode_pixels(f, sample_bytes=1)
        assert got.shape == (h, w, 3) and got.dtype == np.uint8
        np.testing.assert_array_equal(got, P.pack(want))


def test_after_palette(eng):
    c = J.cases()["c2_odd_12bit"]
    got = eng.decode_pixels(c.file, sample_bytes=2)
    assert got.shape == c.want.shape[1:] + (3,)
    np.testing.assert_array_equal(got, P.pack(list(eng.decode(c.file))))
    np.testing.assert_array_equal(got, P.pack(list(c.want)))
    want, _ = truth(eng, c.file, precision="8S")
    with settings(eng, precision="8S"):
        np.testing.assert_array_equal(eng.decode_pixels(c.file, sample_bytes=1), P.pack(want))


# ---------------------------------------------------------------- 6. window and reduce
def test_window_and_reduce(eng):
    w, h = 200, 150
    planes = C.random_planes(w, h, C.S444, 8, seed=61)
    data = encode(eng, planes, 8, tiles=(64, 64), numresolution=3)
    win = (37, 21, 141, 98)
    want = P.pack(list(eng.decode_window(data, win)))
    np.testing.assert_array_equal(want, P.pack(planes)[21:98, 37:141])
    got = eng.decode_pixels(data, sample_bytes=1, window=win)
    assert got.shape == (77, 104, 3)
    np.testing.assert_array_equal(got, want)
    y = torch.zeros((77, 104, 3), dtype=torch.uint8, device="cuda")
    eng.decode_pixels(dev(data), length=len(data), out=y, window=win)
    np.testing.assert_array_equal(y.cpu().numpy(), want)
    eng.set_decode_reduce(1)
    try:
        want = P.pack(list(eng.decode(data)))
        got = eng.decode_pixels(data, sample_bytes=1)
        assert got.shape == (75, 100, 3)
        np.testing.assert_array_equal(got, want)
    finally:
        eng.set_decode_reduce(0)


# ---------------------------------------------------------------- 7. where the bytes live
def test_codestream_and_output_placement(eng):
    w, h = 65, 33
    planes = C.random_planes(w, h, C.S444, 8, seed=71)
    data = encode(eng, planes, 8)
    want = P.pack(planes)
    y = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    eng.decode_pixels(dev(data), length=len(data), out=y)                          # device to device
    np.testing.assert_array_equal(y.cpu().numpy(), want)
    np.testing.assert_array_equal(eng.decode_pixels(data, sample_bytes=1), want)   # host to host
    y.zero_()
    eng.decode_pixels(data, out=y)                                                 # host to device
    np.testing.assert_array_equal(y.cpu().numpy(), want)
    np.testing.assert_array_equal(eng.decode_pixels(dev(data), length=len(data), sample_bytes=1), want)


# ---------------------------------------------------------------- 8. lossy and HT streams
@pytest.mark.parametrize("kind", ["97_layers", "ht"])
def test_other_coders_pack_their_planar_decode(eng, kind):
    w, h = 64, 48
    planes = C.random_planes(w, h, C.S444, 12, seed=81)
    if kind == "97_layers":
        data = encode(eng, planes, 12, irreversible=True, mct=True, layer_rate=[40, 20, 10], numresolution=3)
    else:
        data = encode(eng, planes, 12, cblk_sty=0x40, numresolution=3)
    want = P.pack(list(eng.decode(data)))
    np.testing.assert_array_equal(eng.decode_pixels(data, sample_bytes=2), want)
    want8, _ = truth(eng, data, precision="8S")
    with settings(eng, precision="8S"):
        np.testing.assert_array_equal(eng.decode_pixels(data, sample_bytes=1), P.pack(want8))


# ---------------------------------------------------------------- 9. refusals
def test_refusals_name_their_cause(eng):
    w, h = 33, 17
    sub = encode(eng, C.random_planes(w, h, C.S420, 8, seed=91), 8, sub=C.S420, size=(w, h))
    with pytest.raises(RuntimeError, match="GK_DISPLAY_UPSAMPLE"):
        eng.decode_pixels(sub)
    rgb12 = encode(eng, C.random_planes(w, h, C.S444, 12, seed=92), 12)
    with pytest.raises(RuntimeError, match="sample_bytes"):
        eng.decode_pixels(rgb12, sample_bytes=1)
    # (row_bytes is the binding's to compute: the C entry is called with a short and an odd one)
    b = np.frombuffer(rgb12, np.uint8)
    out = np.zeros((h, w, 3), np.uint16)
    rc = eng.lib.gk_decode_pixels(eng.ctx, ctypes.c_void_p(b.ctypes.data), len(rgb12), 0, ctypes.c_void_p(out.ctypes.data),
                                  w * 3 * 2 - 2, 2, 0)
    assert rc != 0 and "row_bytes" in eng.lib.gk_last_error(eng.ctx).decode()
    assert not out.any()
    rc = eng.lib.gk_decode_pixels(eng.ctx, ctypes.c_void_p(b.ctypes.data), len(rgb12), 0, ctypes.c_void_p(out.ctypes.data),
                                  w * 3 * 2 + 1, 2, 0)
    assert rc != 0 and "row_bytes" in eng.lib.gk_last_error(eng.ctx).decode()
    many = encode(eng, C.random_planes(16, 8, [(1, 1)] * 17, 8, seed=93), 8)
    with pytest.raises(RuntimeError, match="planar calls"):
        eng.decode_pixels(many)
    assert np.asarray(eng.decode(many)).shape == (17, 8, 16)
    with settings(eng, precision="17S"):
        with pytest.raises(RuntimeError, match="17"):
            eng.decode_pixels(rgb12)


def test_some_tiles_only_is_refused(eng):
    planes = np.stack(C.random_planes(64, 48, C.S444, 8, seed=95)).astype(np.int32)
    p = G.default_params(numresolution=3, mct=False, tiles=(32, 32))
    body, _ = eng.encode_tiles(planes, 8, 0, 2, params=p)
    hdr, _, _ = eng.main_header(planes.shape, 8, params=p)
    part = hdr + body + b"\xff\xd9"
    with pytest.raises(RuntimeError, match="only some of its tiles"):
        eng.decode_pixels(part)


# ---------------------------------------------------------------- 10. history
def test_history(eng):
    w, h = 65, 33
    a = encode(eng, C.random_planes(w, h, C.S444, 12, seed=101), 12)
    b = encode(eng, C.random_planes(40, 24, [(1, 1)], 16, seed=102), 16)
    first = eng.decode(a)
    hdr = eng.read_header(a)
    before = [getattr(hdr, n) for n, _ in G.ImageInfo._fields_]
    with settings(eng, force_rgb=True, precision="8S"):
        got = eng.decode_pixels(b, sample_bytes=1)
        assert got.shape == (24, 40, 3)
    with settings(eng, precision="8S"):
        assert eng.read_header(a).prec == 8
        eng.decode_pixels(a, sample_bytes=1)
    again = eng.decode(a)
    np.testing.assert_array_equal(first, again)
    hdr = eng.read_header(a)
    assert [getattr(hdr, n) for n, _ in G.ImageInfo._fields_] == before
    assert [p for p, _ in eng.precisions()] == [12, 12, 12]
