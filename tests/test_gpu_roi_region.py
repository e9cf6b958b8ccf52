"""Shaped region of interest on the GPU: the mask kernels against tests/roi_ref.py, the region encode
against the whole-component ROI the oracle pins, lossless round trips through three decoders, the
region's place in a layered or rate-limited stream, and the engine's state."""
import functools

import numpy as np
import pytest
import torch

import grok_amd as G
import j2k_markers as M
import oracle as O
import roi_ref as RR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = G.Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _clear(eng):
    yield
    eng.set_encode_roi()
    eng.set_decode_layers(0)


def _img(seed, c, h, w, bits=8):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (np.sin(xx / 9.0 + seed) * np.cos(yy / 7.0) + 1) * (1 << (bits - 2))
    return np.clip(base[None].repeat(c, 0) + rng.integers(0, 1 << (bits - 3), size=(c, h, w)), 0,
                   (1 << bits) - 1).astype(np.int32)


def _strokes(h, w):
    m = np.zeros((h, w), np.uint8)
    for i in range(h):
        m[i, i * (w - 1) // (h - 1)] = 255
        m[i, (w - 1) - i * (w - 1) // (h - 1)] = 1
    return m


def _regions(h, w):
    """name -> (rects, mask).  The rectangles are chosen for 40 x 32 tiles from the canvas origin
    under an image origin of (3, 5) as well as for one tile."""
    return {
        "inside": ([(5, 6, 20, 18)], None),
        "crossing": ([(30, 20, 55, 50)], None),
        "border": ([(0, 0, 9, 7), (w - 6, h - 5, w, h)], None),
        "pixel": ([(w // 2, h // 2, w // 2 + 1, h // 2 + 1)], None),
        "strokes": ([], _strokes(h, w)),
        "strokes_device": ([], "device"),
        "both": ([(30, 20, 55, 50), (0, h - 3, 4, h)], _strokes(h, w)),
    }


def _level0(h, w, rects, mask):
    m = np.zeros((h, w), bool)
    for x0, y0, x1, y1 in rects:
        m[y0:y1, x0:x1] = True
    if mask is not None:
        m |= np.asarray(mask) != 0
    return m


def _set(eng, h, w, rects, mask, **kw):
    if isinstance(mask, str):
        mask = torch.from_numpy(_strokes(h, w)).cuda()
    eng.set_encode_roi(rects=rects, mask=mask, **kw)
    return _level0(h, w, rects, _strokes(h, w) if mask is not None else None)


CASES = {
    # name: (h, w, origin, tiles, numresolution)
    "one_tile": (88, 72, None, None, 4),
    "tiles_odd_origin": (90, 75, (3, 5), (40, 32), 6),
}


@functools.lru_cache(maxsize=None)
def _ref_masks(case, region, transform):
    h, w, origin, tiles, numres = CASES[case]
    rects, mask = _regions(h, w)[region]
    m0 = _level0(h, w, rects, _strokes(h, w) if mask is not None else None)
    return RR.image_band_masks(m0, origin or (0, 0), tiles, (0, 0), numres - 1, transform)


# ------------------------------------------------------------------------------------- 1. masks
@pytest.mark.parametrize("transform", ["53", "97"])
@pytest.mark.parametrize("region", list(_regions(8, 8)))
@pytest.mark.parametrize("case", list(CASES))
def test_band_masks_equal_the_reference(eng, case, region, transform):
    """Every band of every tile, byte for byte.  (5-bit samples: the masks do not depend on the
    precision, and 9/7 with five levels is accepted only up to 5 bits.)"""
    h, w, origin, tiles, numres = CASES[case]
    rects, mask = _regions(h, w)[region]
    _set(eng, h, w, rects, mask)
    p = G.default_params(numresolution=numres, irreversible=transform == "97", tiles=tiles, mct=False)
    ref = _ref_masks(case, region, transform)
    assert ref
    for (t, r, b), want in ref.items():
        got = eng.roi_band_mask((1, h, w), 5, p, comp=0, tile=t, resolution=r, band=b, origin=origin or (0, 0))
        assert got.shape == want.shape, (t, r, b)
        assert np.array_equal(got != 0, want), (t, r, b)
    # into device memory
    (t, r, b), want = max(ref.items(), key=lambda kv: kv[1].size)
    out = torch.zeros(want.size, dtype=torch.uint8, device="cuda")
    assert eng.roi_band_mask((1, h, w), 5, p, comp=0, tile=t, resolution=r, band=b, origin=origin or (0, 0), out=out) == want.shape
    assert np.array_equal(out.cpu().numpy().reshape(want.shape) != 0, want)


# ---------------------------------------------------------------------- 2. the whole image as region
@pytest.mark.parametrize("kw", [
    dict(), dict(cblk_sty=5), dict(cblk_sty=0x40), dict(irreversible=True, numresolution=3),
    dict(irreversible=True, numresolution=3, cblk_sty=0x40), dict(tiles=(40, 32), tlm=True),
    dict(cblk_sty=0x40, tiles=(40, 32)), dict(layer_rate=[8.0, 0.0]),
], ids=lambda k: "-".join("%s=%s" % kv for kv in k.items()) or "default")
def test_whole_image_region_is_the_component_roi(eng, kw):
    """One component, the whole image as the region: byte for byte the stream of -ROI c=0,U=s."""
    img = _img(2, 1, 88, 72)
    s = G.probe_encode_roi(img.shape, 8, G.default_params(**kw), rects=[(0, 0, 72, 88)])[0]
    want = eng.encode(img, 8, params=G.default_params(roi=(0, s), **kw))
    eng.set_encode_roi(rects=[(0, 0, 72, 88)], shift=s, components=[0])
    assert eng.encode(img, 8, params=G.default_params(**kw)) == want
    eng.set_encode_roi(mask=np.ones((88, 72), np.uint8))   # shift 0: the smallest legal one, s
    assert eng.encode(img, 8, params=G.default_params(**kw)) == want


# --------------------------------------------------------------------------- 3. lossless round trip
def _rgn_components(cs):
    ms, _ = M.main_markers(cs)
    return [cs[o + 4] for o, m, L in ms if m == 0xff5e], [cs[o + 6] for o, m, L in ms if m == 0xff5e]


@pytest.mark.parametrize("kw", [dict(), dict(cblk_sty=5), dict(cblk_sty=0x40), dict(tiles=(40, 32), tlm=True, plt=True)],
                         ids=["part1", "modeswitch", "ht", "tiles"])
@pytest.mark.parametrize("region", list(_regions(8, 8)))
def test_lossless_round_trip(eng, region, kw):
    h, w = 90, 75
    img = _img(4, 3, h, w)
    rects, mask = _regions(h, w)[region]
    p = G.default_params(**kw)
    mb = G.probe_encode_roi(img.shape, 8, p, rects=[(0, 0, 1, 1)])[0]   # the smallest legal shift
    for shift, comps in ((0, None), (mb + 1, [0, 2])):
        _set(eng, h, w, rects, mask, shift=shift, components=comps)
        cs = eng.encode(img, 8, params=p, origin=(3, 5))
        listed, shifts = _rgn_components(cs)
        assert listed == (comps or [0, 1, 2]) and shifts == [shift or mb] * len(listed)
        assert np.array_equal(eng.decode(cs), img)
        assert np.array_equal(O.decode(cs)[0], img)


def test_lossless_round_trip_pixels_jp2_device_output(eng):
    h, w = 88, 72
    img = _img(5, 3, h, w)
    _set(eng, h, w, *_regions(h, w)["both"])
    plain = eng.encode(img, 8)
    assert _rgn_components(plain)[0] == [0, 1, 2]
    # packed pixels, host and device, give the planar stream
    pix = np.ascontiguousarray(img.transpose(1, 2, 0)).astype(np.uint8)
    assert eng.encode_pixels(pix, 8) == plain
    assert eng.encode_pixels(torch.from_numpy(pix).cuda(), 8) == plain
    # device planes in, device bytes out
    out = torch.zeros(len(plain) + 4096, dtype=torch.uint8, device="cuda")
    n = eng.encode(torch.from_numpy(img).cuda(), 8, out=out)
    assert out[:n].cpu().numpy().tobytes() == plain
    # a .jp2 wraps the same codestream
    jp2 = eng.encode(img, 8, params=G.default_params(jp2=True))
    assert jp2.endswith(plain) and jp2[4:8] == b"jP  "
    assert np.array_equal(eng.decode(jp2), img)
    assert np.array_equal(eng.decode(plain), img)
    assert np.array_equal(O.decode(plain)[0], img)
    assert np.array_equal(O.decode(jp2[jp2.index(b"\xff\x4f\xff\x51"):])[0], img)


@pytest.mark.parametrize("sty", [4, 0x3e])
def test_termall_under_a_region_fits_its_slots(eng, sty):
    """Every pass terminated and 22 coded bit-planes: the slots of a component with an ROI shift hold
    the terminations too (the same image with -ROI c=0,U=11 used to end in a slot overflow)."""
    h, w = 90, 75
    img = _img(6, 3, h, w)
    p = G.default_params(cblk_sty=sty)
    for region in ("crossing", "both"):
        _set(eng, h, w, *_regions(h, w)[region])
        cs = eng.encode(img, 8, params=p, origin=(3, 5))
        assert np.array_equal(eng.decode(cs), img)
        assert np.array_equal(O.decode(cs)[0], img)
    eng.set_encode_roi()
    cs = eng.encode(img, 8, params=G.default_params(cblk_sty=sty, roi=(0, 11)), origin=(3, 5))
    assert cs == O.encode(img, 8, cblk_sty=sty, roi=(0, 11), origin=(3, 5))


def test_openjpeg_reads_the_part1_streams(eng):
    """OpenJPEG 2.5.4 decodes the region streams of the default coder and of the mode-switch coder.
    (Not with BYPASS, bit 0 of the style: it misreads every ROI stream that has raw segments, the
    oracle's whole-component -ROI streams with cblk_sty 1 or 5 included, so that says nothing
    about a region.)"""
    import openjpeg as OJ
    if not OJ.available():
        pytest.skip("no OpenJPEG library on this machine")
    h, w = 90, 75
    img = _img(6, 3, h, w)
    for region in ("crossing", "both"):
        _set(eng, h, w, *_regions(h, w)[region])
        for kw in (dict(), dict(cblk_sty=4), dict(cblk_sty=0x2a), dict(tiles=(40, 32))):
            cs = eng.encode(img, 8, params=G.default_params(**kw), origin=(3, 5))
            dec = OJ.decode(cs)
            assert all(np.array_equal(dec[c][2], img[c]) for c in range(3))


# ------------------------------------------------------------------- 4. / 5. the region comes first
REGION_4 = [(40, 48, 104, 112)]   # 64 x 64 of 256 x 256: 1/16 of the image
RATIO_53 = 2.8


def _layer1(eng, cs):
    eng.set_decode_layers(1)
    try:
        return eng.decode(cs)
    finally:
        eng.set_decode_layers(0)


def _layer_sizes(eng, img, p1, p2):
    return len(eng.encode(img, 8, params=p1)), len(eng.encode(img, 8, params=p2))


def test_region_is_exact_in_the_first_layer_53(eng):
    """Two layers, the first at compression ratio 2.8 (RATIO_53), the second with everything.
    Measured on an MI355X: a one-layer stream at that ratio is 70,043 bytes, the lossless stream
    140,511 bytes (half, as asked; the test asserts 40 .. 60 %), the two-layer region stream
    144,238 bytes.  The region's own share is 1/16 of the image, so layer 1 holds several times
    its passes, which are steeper than any background pass by 2^(2 shift).  With the region the
    layer-1 decode is the source at every region sample (0 of 12,288 differ) and not outside
    (160,392 differ); without the region it is not exact there."""
    img = _img(7, 3, 256, 256)
    x0, y0, x1, y1 = REGION_4[0]
    p = G.default_params(layer_rate=[RATIO_53, 0.0])
    l1, full = _layer_sizes(eng, img, G.default_params(layer_rate=[RATIO_53]), G.default_params())
    print("5/3: ratio %.2f, layer 1 %d bytes, all layers %d bytes" % (RATIO_53, l1, full))
    assert 0.4 * full <= l1 <= 0.6 * full
    plain = _layer1(eng, eng.encode(img, 8, params=p))
    assert not np.array_equal(plain[:, y0:y1, x0:x1], img[:, y0:y1, x0:x1])
    eng.set_encode_roi(rects=REGION_4)
    cs = eng.encode(img, 8, params=p)
    assert np.array_equal(eng.decode(cs), img)
    dec = _layer1(eng, cs)
    print("5/3: region stream %d bytes; layer-1 samples that differ: %d inside, %d in all" % (
        len(cs), int((dec != img)[:, y0:y1, x0:x1].sum()), int((dec != img).sum())))
    assert np.array_equal(dec[:, y0:y1, x0:x1], img[:, y0:y1, x0:x1])
    assert not np.array_equal(dec, img)


def test_region_is_final_in_the_first_layer_97(eng):
    """9/7, two layers (ratio 8, then everything): inside the region the layer-1 decode equals the
    full decode of the same stream sample for sample; outside it does not."""
    img = _img(8, 3, 256, 256)
    x0, y0, x1, y1 = REGION_4[0]
    p = G.default_params(irreversible=True, numresolution=3, layer_rate=[8.0, 0.0])
    plain = eng.encode(img, 8, params=p)
    assert not np.array_equal(_layer1(eng, plain)[:, y0:y1, x0:x1], eng.decode(plain)[:, y0:y1, x0:x1])
    eng.set_encode_roi(rects=REGION_4)
    cs = eng.encode(img, 8, params=p)
    full, dec = eng.decode(cs), _layer1(eng, cs)
    print("9/7: layer-1 samples that differ from the full decode: %d inside, %d in all" % (
        int((dec != full)[:, y0:y1, x0:x1].sum()), int((dec != full).sum())))
    assert np.array_equal(dec[:, y0:y1, x0:x1], full[:, y0:y1, x0:x1])
    assert not np.array_equal(dec, full)


# ----------------------------------------------------------------- 6. the region is better at a rate
def _psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b) ** 2))


def test_region_is_better_at_a_rate_97(eng):
    img = _img(9, 3, 256, 256)
    x0, y0, x1, y1 = REGION_4[0]
    inside = np.zeros(img.shape, bool)
    inside[:, y0:y1, x0:x1] = True
    p = G.default_params(irreversible=True, numresolution=3, layer_rate=[16.0])
    without = eng.decode(eng.encode(img, 8, params=p))
    eng.set_encode_roi(rects=REGION_4)
    with_roi = eng.decode(eng.encode(img, 8, params=p))
    v = [_psnr(with_roi[inside], img[inside]), _psnr(without[inside], img[inside]),
         _psnr(with_roi[~inside], img[~inside]), _psnr(without[~inside], img[~inside])]
    print("9/7 at ratio 16, PSNR dB: inside %.2f with / %.2f without, outside %.2f with / %.2f without" % tuple(v))
    assert v[0] > v[1]
    assert v[2] < v[3]


# ------------------------------------------------------------------------------------------ 7. state
def _fresh(fn):
    e = G.Engine(0)
    try:
        return fn(e)
    finally:
        e.close()


def test_clearing_the_region_restores_the_plain_stream(eng):
    img = _img(10, 3, 88, 72)
    want = _fresh(lambda e: e.encode(img, 8))
    assert want == O.encode(img, 8)
    eng.set_encode_roi(rects=[(8, 8, 40, 40)])
    assert eng.encode(img, 8) != want
    eng.set_encode_roi()
    assert eng.encode(img, 8) == want


def test_a_refused_description_leaves_none(eng):
    img = _img(10, 3, 88, 72)
    eng.set_encode_roi(rects=[(8, 8, 40, 40)])
    with pytest.raises(ValueError, match="empty rectangle"):
        eng.set_encode_roi(rects=[(8, 8, 8, 40)])
    assert eng.encode(img, 8) == O.encode(img, 8)
    with pytest.raises(ValueError, match="empty region"):
        eng.set_encode_roi(mask=torch.zeros((88, 72), dtype=torch.uint8, device="cuda"))
    assert eng.encode(img, 8) == O.encode(img, 8)


def test_a_region_for_another_image_is_refused_and_forgotten_by_the_next_call(eng):
    a, b = _img(11, 3, 88, 72), _img(12, 3, 96, 64)
    eng.set_encode_roi(rects=[(50, 8, 70, 40)], mask=_strokes(88, 72))
    want = _fresh(lambda e: (e.set_encode_roi(rects=[(50, 8, 70, 40)], mask=_strokes(88, 72)), e.encode(a, 8))[1])
    with pytest.raises(RuntimeError, match="roi: rectangle .* outside the 64 x 96 image"):
        eng.encode(b, 8)
    assert eng.encode(a, 8) == want
    eng.set_encode_roi(mask=_strokes(88, 72))
    with pytest.raises(RuntimeError, match="roi: the mask is 72 x 88, the image 64 x 96"):
        eng.encode(b, 8)
    eng.set_encode_roi()
    assert eng.encode(b, 8) == O.encode(b, 8)


# ------------------------------------------------------------- 8. refusals that need an engine
def test_tile_ranges_and_subsampling_are_refused(eng):
    img = _img(13, 3, 96, 64)
    eng.set_encode_roi(rects=[(8, 8, 40, 40)])
    with pytest.raises(RuntimeError, match="roi: gk_encode_tiles while gk_set_encode_roi is set"):
        eng.encode_tiles(img, 8, 0, 1, params=G.default_params(tiles=(32, 32)))
    with pytest.raises(RuntimeError, match="roi: gk_main_header while gk_set_encode_roi is set"):
        eng.main_header((3, 96, 64), 8, params=G.default_params(tiles=(32, 32)))
    planes = [img[0], img[1][::2, ::2].copy(), img[2][::2, ::2].copy()]
    with pytest.raises(RuntimeError, match="roi: subsampled components"):
        eng.encode(planes, 8, subsampling=[(1, 1), (2, 2), (2, 2)], size=(64, 96))
    eng.set_encode_convert("sycc", (2, 2))
    try:
        with pytest.raises(RuntimeError, match="roi: subsampled components"):
            eng.encode(img, 8)
    finally:
        eng.set_encode_convert()
    with pytest.raises(RuntimeError, match="roi: a region together with roi_compno / roi_shift"):
        eng.encode(img, 8, params=G.default_params(roi=(0, 11)))
    with pytest.raises(RuntimeError, match="ROI shift too large for this precision"):
        eng.encode(_img(14, 1, 64, 64, 16), 16)
    with pytest.raises(RuntimeError, match="roi: no region is set"):
        eng.set_encode_roi()
        eng.roi_band_mask((1, 64, 64), 8)
