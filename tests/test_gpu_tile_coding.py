"""Tiles coded with their own parameters (tile-part COD / COC / QCD / QCC) on the HIP path; the
oracle half, pinned by OpenJPEG, is tests/test_tile_coding.py.  The engine decodes the tiles with
the main header's coding in one pass and every other tile in a pass of its own (its plan and
quantisation), into one output: full and reduced, host and device (TLM-located) streams, 8-bit
output, windows across tiles of both kinds, and Grok's whole-tile rule for a tile decode."""
import numpy as np
import pytest

import oracle as O
from tile_coding import CASES, expected, stream, tile_rects

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import grok_amd as G
    e = G.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_engine_tile_coding(eng, name):
    cs = stream(name)
    want = expected(name)
    np.testing.assert_array_equal(O.decode(cs)[0], want)
    np.testing.assert_array_equal(eng.decode(cs), want)


@pytest.mark.parametrize("name", ["levels_cblk", "coc_form", "prog_layers_sop", "scope_irrev"])
def test_engine_tile_coding_device_tlm(eng, name):
    import torch
    cs = stream(name, tlm=True)
    d = torch.frombuffer(bytearray(cs), dtype=torch.uint8).cuda()
    np.testing.assert_array_equal(eng.decode(d, len(cs)), expected(name))


@pytest.mark.parametrize("name", ["levels_cblk", "rev_to_irrev", "coc_form", "ht_tile", "ragged_tiles", "origin_tiles"])
def test_engine_tile_coding_reduced(eng, name):
    eng.set_decode_reduce(1)
    try:
        got = eng.decode(stream(name))
    finally:
        eng.set_decode_reduce(0)
    np.testing.assert_array_equal(got, expected(name, reduce=1))


def test_engine_tile_coding_u8(eng):
    got = eng.decode(stream("ht_tile"), sample_bytes=1)
    assert got.dtype == np.uint8
    np.testing.assert_array_equal(got.astype(np.int32), expected("ht_tile"))


@pytest.mark.parametrize("name", ["levels_cblk", "rev_to_irrev", "modes_tile", "ragged_tiles", "origin_tiles"])
@pytest.mark.parametrize("win", [(5, 7, 61, 50), (40, 30, 60, 45), (0, 0, 20, 20)])
def test_engine_tile_coding_window(eng, name, win):
    H, W = CASES[name][:2]
    x0, y0, x1, y1 = win
    x1, y1 = min(x1, W), min(y1, H)
    want = expected(name, partial=True)[:, y0:y1, x0:x1]
    np.testing.assert_array_equal(eng.decode_window(stream(name), (x0, y0, x1, y1)), want)


@pytest.mark.parametrize("name", ["levels_cblk", "scope_irrev"])
def test_engine_tile_coding_tile_decode(eng, name):
    # -tile t without a window: Grok's whole-tile rule, each tile (B or A coded) on its own
    cs = stream(name)
    want = expected(name)
    eng.set_window_rule(True)
    try:
        for t, (x0, y0, x1, y1) in tile_rects(name).items():
            got = eng.decode_window(cs, (x0, y0, x1, y1))
            np.testing.assert_array_equal(got, want[:, y0:y1, x0:x1], err_msg=f"tile {t}")
    finally:
        eng.set_window_rule(False)


def test_engine_tile_coding_reduce_past_a_tile_refused(eng):
    eng.set_decode_reduce(2)
    try:
        with pytest.raises(RuntimeError, match="reduce must be less"):
            eng.decode(stream("ragged_tiles"))
    finally:
        eng.set_decode_reduce(0)


@pytest.mark.parametrize("reduce", [0, 1])
def test_engine_tile_coding_device_output(eng, reduce):
    # the passes write straight into the caller's device planes
    import torch
    name = "levels_cblk"
    want = expected(name, reduce=reduce)
    out = torch.full(want.shape, -1, dtype=torch.int32, device="cuda")
    eng.set_decode_reduce(reduce)
    try:
        eng.decode(stream(name), out=out)
    finally:
        eng.set_decode_reduce(0)
    np.testing.assert_array_equal(out.cpu().numpy(), want)


def test_engine_tile_coding_subsampled():
    # a 4:2:0 stream whose tile 1 is coded with its own levels and code-blocks
    import grok_amd as G
    import tile_coding as TC
    from subsampling_cases import comp_shape
    W, H, sub = 96, 80, [(1, 1), (2, 2), (2, 2)]
    rng = np.random.default_rng(5)
    src = [rng.integers(0, 256, size=comp_shape(W, H, dx, dy)).astype(np.int32) for dx, dy in sub]
    a = O.encode(src, 8, size=(W, H), subsampling=sub, tiles=TC.TILES, numres=3)
    b = O.encode(src, 8, size=(W, H), subsampling=sub, tiles=TC.TILES, numres=2, cblk=(16, 16))
    cs = TC.splice(a, b, {1}, "cod")
    want, _ = O.decode(cs)
    e = G.Engine(0)
    try:
        got = e.decode(cs)
    finally:
        e.close()
    for g, w, s in zip(got, want, src):
        np.testing.assert_array_equal(g, w)
        np.testing.assert_array_equal(g, s)   # (lossless either way)


# ---- the output, display and colour stages over tile passes: each stage decodes the components
# once, the component decode splits into passes.  Truth: the oracle's planar decode of the raw
# codestream, through the restatements the stages' own suites use.
def _jp2(cs, nc, h, w, boxes):
    import jp2_boxes as J
    return J.jp2_file(cs, [J.ihdr(h, w, nc, 8), J.colr_enum(16)] + boxes)


def _dev(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def _spliced(src, **kw):
    # as test_engine_tile_coding_subsampled splices: tile 1 with its own levels and code-blocks
    import tile_coding as TC
    a = O.encode(src, 8, tiles=TC.TILES, numres=3, **kw)
    b = O.encode(src, 8, tiles=TC.TILES, numres=2, cblk=(16, 16), **kw)
    return TC.splice(a, b, {1}, "cod")


def test_pixels_over_passes(eng):
    import torch
    name = "levels_cblk"
    cs = stream(name)
    want = np.moveaxis(O.decode(cs)[0], 0, -1)
    got = eng.decode_pixels(cs, sample_bytes=1)
    assert got.dtype == np.uint8
    np.testing.assert_array_equal(got, want)
    y = torch.full(want.shape, 0xA5, dtype=torch.uint8, device="cuda")
    eng.decode_pixels(cs, out=y)
    np.testing.assert_array_equal(y.cpu().numpy(), want)
    x0, y0, x1, y1 = win = (5, 7, 61, 50)
    got = eng.decode_pixels(cs, sample_bytes=1, window=win)
    np.testing.assert_array_equal(got, np.moveaxis(expected(name, partial=True)[:, y0:y1, x0:x1], 0, -1))


def test_forced_precision_over_passes(eng):
    import pixels_ref as P
    name, spec = "rev_to_irrev", "6S,10S,5C"   # every channel changes: scaled down, scaled up, clamped
    cs = stream(name)
    planes, _ = O.decode(cs)
    want, comps = P.force_precision(list(planes), [(1, 1, 8, 0)] * 3, spec)
    assert [c[2] for c in comps] == [6, 10, 5] and all((w != p).any() for w, p in zip(want, planes))
    eng.set_decode_precision(spec)
    try:
        got = eng.decode(cs)
    finally:
        eng.set_decode_precision(None)
    np.testing.assert_array_equal(got, np.stack(want))


@pytest.mark.parametrize("device", [False, True])
def test_cdef_over_passes(eng, device):
    import jp2_boxes as J
    name, entries = "coc_form", [(0, 0, 3), (1, 0, 2), (2, 0, 1)]   # channels 0 and 2 change places
    H, W = CASES[name][:2]
    cs = stream(name, tlm=device)
    planes, _ = O.decode(cs)
    want, _ = J.expected(list(planes), cdef_entries=entries)
    np.testing.assert_array_equal(want, planes[[2, 1, 0]])
    f = _jp2(cs, 3, H, W, [J.cdef(entries)])
    got = eng.decode(_dev(f), len(f)) if device else eng.decode(f)
    np.testing.assert_array_equal(got, want)


def test_palette_over_passes(eng):
    import jp2_boxes as J
    W, H = 96, 80
    idx = J._indices(H, W, 256, 3)[None]
    cs = _spliced(idx, mct=False)
    planes, _ = O.decode(cs)
    np.testing.assert_array_equal(planes, idx)
    lut, cm = J._lut(256, [8, 8, 8], 4), [(0, 1, 0), (0, 1, 1), (0, 1, 2)]
    want, _ = J.expected(list(planes), lut, cm)
    got = eng.decode(_jp2(cs, 1, H, W, [J.pclr(lut, [8, 8, 8]), J.cmap(cm)]))
    np.testing.assert_array_equal(got, want)


def test_upsampling_over_passes(eng):
    import display_ref as R
    from subsampling_cases import comp_shape
    W, H, sub = 96, 80, [(1, 1), (2, 2), (2, 2)]
    rng = np.random.default_rng(5)
    src = [rng.integers(0, 256, size=comp_shape(W, H, dx, dy)).astype(np.int32) for dx, dy in sub]
    cs = _spliced(src, size=(W, H), subsampling=sub)
    planes, _ = O.decode(cs)
    want = R.post_process(planes, [(dx, dy, 8, 0) for dx, dy in sub], 0, (0, 0, W, H), upsample=True)[0]
    want = np.stack(want)
    assert want.shape == (3, H, W)
    eng.set_decode_display(upsample=True)
    try:
        got = eng.decode(cs)
        pix = eng.decode_pixels(cs, sample_bytes=1)   # output -> display -> components -> passes
    finally:
        eng.set_decode_display()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(pix, np.moveaxis(want, 0, -1))


@pytest.mark.parametrize("name", ["ht_and_part1", "mode_switches", "wide_block"])
def test_engine_tile_cod_resets_main_coc(eng, name):
    import j2k_markers as J
    import test_coc
    cs = test_coc.stream(name)
    t = J.insert_tile_part(cs, J.cod(cs))
    for g, w in zip(eng.decode(t), O.decode(t)[0]):
        np.testing.assert_array_equal(g, w)
