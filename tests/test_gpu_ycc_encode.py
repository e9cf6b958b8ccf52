"""RGB to sYCC on encode, on the GPU (k_rgb_ycc, gk_rgbycc.hip) through Engine.set_encode_convert.

Truth: tests/ycc_ref.py, the integer definition of the conversion.  The kernel gets no tolerance: a
stream written under a conversion is byte for byte the planar encode of the restated planes on
another engine with the colour space set (and, for raw codestreams, oracle.encode of them), and the
engine's own flag-0 decode of a lossless stream returns the restated planes.  The only bounds are
those of tests/test_ycc_encode.py: restated inverse of restated forward against the source.

The shapes walk every path of the kernel: the partial group (widths 1, 2, 7, 9, 17), one whole lane
(8), the second workgroup in x (2049, 4099), the 4-unit row group (3, 4, 5, 7, 9 rows), the last row
and column without a partner, and the column / row in front of the first box (odd origins)."""
import ctypes

import numpy as np
import pytest
import torch

import grok_amd as G
import display_cases as C
import display_ref as D
import oracle as O
import ycc_ref as Y
from test_ycc_encode import ROUND_TRIP, sample_colours

pytestmark = pytest.mark.gpu

LAYOUTS = {"444": Y.S444, "422": Y.S422, "420": Y.S420}
# kind: (numpy dtype, torch dtype, precision)
KINDS = {
    "u8": (np.uint8, torch.uint8, 8),
    "u16p12": (np.uint16, torch.int16, 12),
    "u16p16": (np.uint16, torch.int16, 16),
    "i32p8": (np.int32, torch.int32, 8),
}
SIZES = [(1, 1), (2, 2), (7, 3), (8, 4), (9, 5), (17, 9), (2049, 7), (4099, 3)]
ORIGINS = [(0, 0), (1, 0), (0, 1), (1, 1)]


@pytest.fixture(scope="module")
def eng():
    e = G.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def planar():
    """Another engine, colour space sYCC, never given a conversion: the planar encodes compared with."""
    e = G.Engine(0)
    e.set_encode_colour("sycc")
    yield e
    e.close()


def pixels(w, h, kind, seed=0):
    """(h, w, 3) random samples over the kind's whole range; the first pixels are the range's corners."""
    dt, _, prec = KINDS[kind]
    rng = np.random.RandomState(seed * 131 + w * 7 + h * 3)
    x = rng.randint(0, 1 << prec, (h, w, 3)).astype(np.int64)
    top = (1 << prec) - 1
    corners = [(top, 0, 0), (0, top, 0), (0, 0, top), (top, top, top), (0, 0, 0), (top, top, 0), (0, top, top), (top, 0, top)]
    flat = x.reshape(-1, 3)
    flat[:min(len(corners), len(flat))] = corners[:len(flat)]
    return flat.reshape(h, w, 3).astype(dt)


def ref_planes(pix, kind, sub, origin=(0, 0)):
    dt, _, prec = KINDS[kind]
    return [p.astype(dt) for p in Y.rgb_to_ycc(pix, prec, sub, origin)]


def params(w, h, sub, **kw):
    kw.setdefault("numresolution", C.numres_for(w, h, Y.subsampling(sub)))
    return G.default_params(**kw)   # (mct=True: the conversion and the colour space clear it)


def planar_encode(planar, planes, prec, sub, size, p, origin):
    return planar.encode(planes, prec, params=p, origin=origin, subsampling=Y.subsampling(sub), size=size)


def to_dev(a, tdt):
    return torch.from_numpy(a.view({1: np.uint8, 2: np.int16, 4: np.int32}[a.dtype.itemsize]).copy()).to("cuda").view(tdt)


# ---------------------------------------------------------------- every colour
def test_every_8_bit_colour(eng):
    v = np.arange(1 << 24, dtype=np.uint32)
    pix = np.stack([v >> 16, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    want = np.stack(Y.rgb_to_ycc(pix, 8))
    eng.set_encode_convert("sycc", (1, 1))
    try:
        cs = eng.encode_pixels(to_dev(pix, torch.uint8), 8, params=G.default_params(numresolution=6))
    finally:
        eng.set_encode_convert(None)
    got = eng.decode(cs)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want)


def test_16_bit_corners_edges_and_sample(eng):
    pts = sample_colours(16, n=512 * 512)[0]                         # 512 * 512 + 12 * 65536 colours
    assert len(pts) == 512 * 2048
    pix = pts.reshape(512, 2048, 3).astype(np.uint16)
    want = np.stack(Y.rgb_to_ycc(pix, 16))
    eng.set_encode_convert("sycc", (1, 1))
    try:
        cs = eng.encode_pixels(to_dev(pix, torch.int16), 16, params=G.default_params(numresolution=6))
    finally:
        eng.set_encode_convert(None)
    np.testing.assert_array_equal(eng.decode(cs), want)


# ---------------------------------------------------------------- bytes
def both(fn_got, fn_want):
    """fn_got() == fn_want(), or both refuse with the same message (whatever the subsampled planar
    encode refuses, the conversion refuses)."""
    try:
        want = fn_want()
    except RuntimeError as e:
        with pytest.raises(RuntimeError) as r:
            fn_got()
        assert str(r.value).split(": ", 1)[-1] == str(e).split(": ", 1)[-1]
        print("both refuse:", e)
        return None
    got = fn_got()
    assert got == want
    return got


@pytest.mark.parametrize("origin", ORIGINS, ids=lambda o: "o%d%d" % o)
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_bytes_equal_the_planar_encode_of_the_restated_planes(eng, planar, layout, kind, origin):
    sub = LAYOUTS[layout]
    _, _, prec = KINDS[kind]
    eng.set_encode_convert("sycc", sub)
    try:
        for w, h in SIZES:
            pix = pixels(w, h, kind)
            planes = ref_planes(pix, kind, sub, origin)
            p = params(w, h, sub)
            got = both(lambda: eng.encode_pixels(pix, prec, params=p, origin=origin),
                       lambda: planar_encode(planar, planes, prec, sub, (w, h), p, origin))
            if got is not None:
                want = O.encode([q.astype(np.int32) for q in planes], prec, size=(w, h), subsampling=Y.subsampling(sub),
                                mct=False, origin=origin, numres=p.numresolution)
                assert got == want, (w, h)
    finally:
        eng.set_encode_convert(None)


def misaligned(pix, tdt, off_bytes):
    """The pixels as a device tensor with a padded row stride whose base lies off_bytes past a
    256-byte boundary."""
    h, w, c = pix.shape
    es = pix.dtype.itemsize
    pitch = -(-(w * c * es + 13) // 64) * 64 // es            # elements; a multiple of 64 bytes
    off = off_bytes // es
    flat = np.full(h * pitch + off + 64, 0x55, pix.dtype)
    rows = flat[off:off + h * pitch].reshape(h, pitch)
    rows[:, :w * c] = pix.reshape(h, w * c)
    t = to_dev(flat, tdt)[off:off + h * pitch].view(h, pitch)[:, :w * c].unflatten(1, (w, c))
    assert t.data_ptr() % 4 == off_bytes % 4 and t.stride(0) == pitch
    return t


@pytest.mark.parametrize("origin", [(0, 0), (1, 1)], ids=lambda o: "o%d%d" % o)
@pytest.mark.parametrize("kind", ["u8", "u16p12"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_input_variants(eng, planar, layout, kind, origin):
    sub = LAYOUTS[layout]
    dt, tdt, prec = KINDS[kind]
    eng.set_encode_convert("sycc", sub)
    try:
        for w, h in [(17, 9), (2049, 7)]:
            pix = pixels(w, h, kind, seed=1)
            p = params(w, h, sub)
            want = planar_encode(planar, ref_planes(pix, kind, sub, origin), prec, sub, (w, h), p, origin)
            enc = lambda x: eng.encode_pixels(x, prec, params=p, origin=origin)
            assert enc(pix) == want, "host array"
            assert enc(to_dev(pix, tdt)) == want, "device tensor"
            for off in ((1, 2, 3) if kind == "u8" else (2,)):
                assert enc(misaligned(pix, tdt, off)) == want, "device tensor %d bytes off a dword" % off
            chw = np.ascontiguousarray(np.moveaxis(pix, 2, 0))
            assert eng.encode(chw, prec, params=p, origin=origin) == want, "host planes"
            assert eng.encode(to_dev(chw, tdt), prec, params=p, origin=origin) == want, "device planes"
            out = torch.zeros(w * h * 12 + (1 << 20), dtype=torch.uint8, device="cuda")
            n = eng.encode_pixels(to_dev(pix, tdt), prec, params=p, origin=origin, out=out)
            assert out[:n].cpu().numpy().tobytes() == want, "device output"
    finally:
        eng.set_encode_convert(None)


# ---------------------------------------------------------------- coding parameters pass through
@pytest.mark.parametrize("name,kw", [
    ("tiles64", dict(tiles=(64, 64), numresolution=3)),
    ("97_layers", dict(irreversible=True, layer_rate=[40, 20, 10], numresolution=4)),
    ("ht", dict(cblk_sty=0x40, numresolution=4)),
])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_coding_parameters_pass_through(eng, planar, layout, name, kw):
    sub = LAYOUTS[layout]
    w, h = 200, 136
    pix = pixels(w, h, "u8", seed=len(name))
    p = G.default_params(**kw)
    want = planar_encode(planar, ref_planes(pix, "u8", sub), 8, sub, (w, h), p, None)
    eng.set_encode_convert("sycc", sub)
    try:
        assert eng.encode_pixels(pix, 8, params=p) == want
        assert eng.encode_pixels(to_dev(pix, torch.uint8), 8, params=p) == want
    finally:
        eng.set_encode_convert(None)


def test_a_tile_size_the_factor_does_not_divide_is_refused_as_by_the_planar_encode(eng, planar):
    w, h = 200, 136
    pix = pixels(w, h, "u8")
    p = G.default_params(tiles=(63, 64), numresolution=3)
    eng.set_encode_convert("sycc", Y.S420)
    try:
        with pytest.raises(RuntimeError, match="does not divide the tile size"):
            planar_encode(planar, ref_planes(pix, "u8", Y.S420), 8, Y.S420, (w, h), p, None)
        with pytest.raises(RuntimeError, match="does not divide the tile size"):
            eng.encode_pixels(pix, 8, params=p)
        p = G.default_params(tiles=(64, 64), numresolution=3)
        assert eng.encode_pixels(pix, 8, params=p) == \
            planar_encode(planar, ref_planes(pix, "u8", Y.S420), 8, Y.S420, (w, h), p, None)
    finally:
        eng.set_encode_convert(None)


# ---------------------------------------------------------------- JP2 and the way back
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_jp2_boxes_and_decode_to_rgb(eng, layout):
    sub = LAYOUTS[layout]
    w, h, prec = 67, 45, 8
    comps = [(dx, dy, prec, 0) for dx, dy in Y.subsampling(sub)]
    eng.set_encode_convert("sycc", sub)
    eng.set_decode_display(rgb=True)
    try:
        for name, pix in (("random", pixels(w, h, "u8", seed=2)),
                          ("box-constant", Y.box_constant(np.random.RandomState(4), w, h, prec, sub).astype(np.uint8))):
            p = params(w, h, sub)
            raw = eng.encode_pixels(pix, prec, params=p)
            p2 = params(w, h, sub, jp2=True)
            jp2 = eng.encode_pixels(pix, prec, params=p2)
            assert jp2 == G.jp2_boxes((3, h, w), prec, len(raw), space="sycc") + raw, name
            planes = Y.rgb_to_ycc(pix, prec, sub)
            want, _ = D.color_sycc_to_rgb(planes, comps, 0, 0)
            got = eng.decode_pixels(jp2, sample_bytes=1)
            np.testing.assert_array_equal(got, np.stack(want, -1).astype(np.uint8), err_msg=name)
            if name == "box-constant":
                err = [int(np.abs(got[:, :, k].astype(np.int64) - pix[:, :, k]).max()) for k in range(3)]
                print(layout, "round trip max error", err)
                assert all(err[k] <= ROUND_TRIP[8][0][k] for k in range(3))
    finally:
        eng.set_decode_display()
        eng.set_encode_convert(None)


def test_esycc_jp2_and_decode_to_rgb(eng):
    w, h, prec = 67, 45, 8
    pix = pixels(w, h, "u8", seed=6)
    p = params(w, h, Y.S444, jp2=True)
    eng.set_encode_convert("esycc")
    eng.set_decode_display(rgb=True)
    try:
        jp2 = eng.encode_pixels(pix, prec, params=p)
        boxes = G.jp2_boxes((3, h, w), prec, 0, space="esycc")
        assert jp2[:len(boxes) - 8] == boxes[:-8]                    # (everything in front of the jp2c box header)
        assert G.probe_colour(jp2).enumcs == 24
        planes = Y.rgb_to_ycc(pix, prec)
        want = D.color_esycc_to_rgb(planes, [(1, 1, prec, 0)] * 3)
        got = eng.decode_pixels(jp2, sample_bytes=1)
        np.testing.assert_array_equal(got, np.stack(want, -1).astype(np.uint8))
        err = [int(np.abs(got[:, :, k].astype(np.int64) - pix[:, :, k]).max()) for k in range(3)]
        print("e-sYCC round trip max error", err)
        assert all(err[k] <= ROUND_TRIP[8][1][k] for k in range(3))
    finally:
        eng.set_decode_display()
        eng.set_encode_convert(None)


def test_an_encode_colour_of_the_same_space_is_honoured(eng, planar):
    """The caller's sYCC description with a channel definition: its cdef is written as the planar
    call writes it."""
    w, h = 40, 24
    pix = pixels(w, h, "u8", seed=8)
    p = params(w, h, Y.S420, jp2=True)
    channels = [(0, 1), (0, 2), (1, 0)]
    eng.set_encode_convert("sycc", Y.S420)
    try:
        plain = eng.encode_pixels(pix, 8, params=p)
        eng.set_encode_colour("sycc", channels=channels)
        planar.set_encode_colour("sycc", channels=channels)
        got = eng.encode_pixels(pix, 8, params=p)
        assert got == planar_encode(planar, ref_planes(pix, "u8", Y.S420), 8, Y.S420, (w, h), p, None)
        assert got != plain and b"cdef" in got and b"cdef" not in plain
    finally:
        planar.set_encode_colour("sycc")
        eng.set_encode_colour()
        eng.set_encode_convert(None)


# ---------------------------------------------------------------- history
def test_history_a_conversion_leaves_no_trace(eng):
    plain = pixels(90, 33, "u8", seed=5)
    pp = G.default_params(numresolution=3)
    first = eng.encode_pixels(plain, 8, params=pp)
    big, small = pixels(300, 77, "u8", seed=6), pixels(21, 10, "u8", seed=7)
    subs = C.S420
    sub_planes = C.random_planes(50, 30, subs, 8, seed=3)
    sub_first = eng.encode(sub_planes, 8, params=pp, subsampling=subs, size=(50, 30))
    fresh = G.Engine(0)
    try:
        fresh.set_encode_colour("sycc")
        eng.set_encode_convert("sycc", Y.S420)
        for pix in (big, small):
            h, w, _ = pix.shape
            assert eng.encode_pixels(pix, 8, params=pp) == \
                planar_encode(fresh, ref_planes(pix, "u8", Y.S420), 8, Y.S420, (w, h), pp, None)
        with pytest.raises(RuntimeError, match="4 channels"):
            eng.encode_pixels(np.zeros((8, 8, 4), np.uint8), 8, params=pp)
        eng.set_encode_convert("sycc", Y.S422)
        p16 = pixels(131, 20, "u16p12", seed=8)
        assert eng.encode_pixels(p16, 12, params=pp) == \
            planar_encode(fresh, ref_planes(p16, "u16p12", Y.S422), 12, Y.S422, (131, 20), pp, None)
        eng.set_encode_convert(None)
        fresh.set_encode_colour()
        again = eng.encode_pixels(plain, 8, params=pp)
        assert again == first
        assert fresh.encode_pixels(plain, 8, params=pp) == first
        assert eng.encode(sub_planes, 8, params=pp, subsampling=subs, size=(50, 30)) == sub_first
        assert fresh.encode(sub_planes, 8, params=pp, subsampling=subs, size=(50, 30)) == sub_first
    finally:
        eng.set_encode_convert(None)
        fresh.close()


# ---------------------------------------------------------------- refusals that need the engine
def test_refusals_name_the_cause_and_leave_the_engine_usable(eng, planar):
    w, h = 40, 24
    pix = pixels(w, h, "u8", seed=9)
    chw = np.ascontiguousarray(np.moveaxis(pix, 2, 0)).astype(np.int32)
    p = params(w, h, Y.S420)
    want = planar_encode(planar, ref_planes(pix, "u8", Y.S420), 8, Y.S420, (w, h), p, None)
    eng.set_encode_convert("sycc", Y.S420)

    def still_good():
        assert eng.encode_pixels(pix, 8, params=p) == want

    try:
        still_good()
        with pytest.raises(RuntimeError, match="gk_encode_tiles while gk_set_encode_convert is set"):
            eng.encode_tiles(chw, 8, 0, 1, params=p)
        still_good()
        with pytest.raises(RuntimeError, match="gk_main_header while gk_set_encode_convert is set"):
            eng.main_header((3, h, w), 8, params=p)
        still_good()
        info = G.ImageInfo(w, h, 3, 8, 0, 0)
        ptrs = (ctypes.c_void_p * 3)(*[chw[k].ctypes.data for k in range(3)])
        strides = (ctypes.c_uint32 * 3)(w, w, w)
        rc = eng.lib.gk_encode_blocks(ctypes.c_void_p(eng.ctx), ctypes.byref(info), ptrs, strides, 0, ctypes.byref(p), None, None, None, None)
        assert rc == -1 and "gk_encode_blocks while gk_set_encode_convert is set" in eng.lib.gk_last_error(eng.ctx).decode()
        still_good()
        assert eng.lib.gk_set_subsampling(eng.ctx, 3, (ctypes.c_uint32 * 3)(1, 2, 2), (ctypes.c_uint32 * 3)(1, 2, 2)) == 0
        try:
            with pytest.raises(RuntimeError, match="convert: gk_set_subsampling is active"):
                eng.encode_pixels(pix, 8, params=p)
            with pytest.raises(RuntimeError, match="convert: gk_set_subsampling is active"):
                eng.encode(chw, 8, params=p)
        finally:
            assert eng.lib.gk_set_subsampling(eng.ctx, 0, None, None) == 0
        still_good()
        for space in ("srgb", "esycc"):
            eng.set_encode_colour(space)
            with pytest.raises(RuntimeError, match="the encode colour names colour space"):
                eng.encode_pixels(pix, 8, params=p)
        eng.set_encode_colour()
        still_good()
        for bad, name in ((np.zeros((8, 8, 4), np.uint8), "4 channels"), (np.zeros((8, 8), np.uint8), "1 channels")):
            with pytest.raises(RuntimeError, match=name):
                eng.encode_pixels(bad, 8, params=p)
        with pytest.raises(RuntimeError, match="signed"):
            eng.encode_pixels(pix.astype(np.int8), 8, signed=True, params=p)
        with pytest.raises(RuntimeError, match="precision 17"):
            eng.encode_pixels(pix.astype(np.int32), 17, params=p)
        with pytest.raises(RuntimeError, match="2 channels"):
            eng.encode(chw[:2], 8, params=p)
        still_good()
        # a refused spec leaves none set: the next call is the plain one
        with pytest.raises(ValueError, match="e-sYCC with subsampled chroma"):
            eng.set_encode_convert("esycc", Y.S420)
        with pytest.raises(ValueError, match="chroma subsampling 1 x 2"):
            eng.set_encode_convert("sycc", (1, 2))
        pp = params(w, h, Y.S444)
        assert eng.encode_pixels(pix, 8, params=pp) == eng.encode(chw, 8, params=pp)
    finally:
        eng.set_encode_colour()
        eng.set_encode_convert(None)
