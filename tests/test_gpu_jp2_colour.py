"""JP2 colour boxes on the GPU: decodes of the case files (tests/jp2_boxes.py: palettes through
k_jp2_palette's LDS and global-gather paths, direct channels, cdef reorders, colour description
only) equal the numpy restatement built from the lossless sources: whole image, windows, reduced
resolution, host int32 and device 8 / 16-bit planes, and through the Grok C API."""
import os
import subprocess

import numpy as np
import pytest
import torch

import grok_amd as G
import oracle as O
import jp2_boxes as J
from conftest import ROOT
from grok_amd.synth import synth_image

pytestmark = pytest.mark.gpu

CASES = J.cases()
NAMES = sorted(CASES)
WINDOWS = [(1, 1, 2, 2), (37, 5, 47, 33)]
STRADDLE = (60, 50, 140, 130)   # case 3: across the 64 x 64 tile grid


@pytest.fixture(scope="module")
def eng():
    e = G.Engine(0)
    yield e
    e.close()


def _narrow(c):
    """(torch dtype, numpy view) of the 8 / 16-bit planes sized by the widest output channel."""
    return (torch.uint8, np.uint8) if max(c.out_prec) <= 8 else (torch.int16, np.uint16)


def _dev(data):
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()


@pytest.mark.parametrize("name", NAMES)
def test_decode_equals_expected(eng, name):
    c = CASES[name]
    dec = eng.decode(c.file)
    assert dec.dtype == np.int32
    np.testing.assert_array_equal(dec, c.want)
    ci = eng.colour_info()
    assert (ci.num_comps, ci.num_channels, ci.colour_space) == (c.src.shape[0], c.want.shape[0], c.colour_space)
    assert bool(ci.has_palette) == (c.lut is not None)   # (c6, c7: no palette, so no palette launch)
    assert [t for t, _ in ci.channels()] == c.typ
    assert eng.icc_profile() == (c.icc or b"")
    # device-resident file bytes into device planes of the narrow type
    tdt, view = _narrow(c)
    y = torch.zeros(c.want.shape, dtype=tdt, device="cuda")
    eng.decode(_dev(c.file), length=len(c.file), out=y)
    np.testing.assert_array_equal(y.cpu().numpy().view(view), c.want.astype(view))


@pytest.mark.parametrize("name", NAMES)
def test_windows_equal_the_crop(eng, name):
    c = CASES[name]
    d = _dev(c.file)
    tdt, view = _narrow(c)
    for (x0, y0, x1, y1) in WINDOWS + ([STRADDLE] if name == "c3_tiles_1024" else []):
        want = c.want[:, y0:y1, x0:x1]
        np.testing.assert_array_equal(eng.decode_window(c.file, (x0, y0, x1, y1)), want)
        y = torch.zeros(want.shape, dtype=tdt, device="cuda")
        eng.decode_window(d, (x0, y0, x1, y1), length=len(c.file), out=y)
        np.testing.assert_array_equal(y.cpu().numpy().view(view), want.astype(view))


@pytest.mark.parametrize("name", ["c2_odd_12bit", "c5_direct_cdef"])
def test_padded_rows_take_vector_stores_with_a_tail(eng, name):
    # rows padded to 64 samples are aligned for the kernel's vector stores; the width (47) is not a
    # multiple of the vector, so every row ends in the scalar tail.  The padding stays untouched.
    c = CASES[name]
    nch, h, w = c.want.shape
    tdt, view = _narrow(c)
    buf = torch.full((nch, h, 64), 77, dtype=tdt, device="cuda")
    eng.decode_window(_dev(c.file), (0, 0, w, h), length=len(c.file), out=buf[:, :, :w])
    got = buf.cpu().numpy().view(view)
    np.testing.assert_array_equal(got[:, :, :w], c.want.astype(view))
    assert (got[:, :, w:] == 77).all()
    buf32 = torch.full((nch, h, 64), -5, dtype=torch.int32, device="cuda")
    eng.decode_window(c.file, (0, 0, w, h), out=buf32[:, :, :w])
    np.testing.assert_array_equal(buf32.cpu().numpy()[:, :, :w], c.want)
    assert (buf32.cpu().numpy()[:, :, w:] == -5).all()


def test_reduced_decode_applies_the_palette(eng):
    c = CASES["c3_tiles_1024"]
    O.set_decode_reduce(1)
    try:
        planes, _ = O.decode(c.cs)
    finally:
        O.set_decode_reduce(0)
    want = c.expected_of(planes)
    eng.set_decode_reduce(1)
    try:
        np.testing.assert_array_equal(eng.decode(c.file), want)
        x0, y0, x1, y1 = STRADDLE
        cd = lambda v: -(-v >> 1)
        np.testing.assert_array_equal(eng.decode_window(c.file, STRADDLE), want[:, cd(y0):cd(y1), cd(x0):cd(x1)])
    finally:
        eng.set_decode_reduce(0)


@pytest.mark.parametrize("name", ["c1_clamp200", "c5_direct_cdef", "c6_cdef_only"])
def test_set_decode_colour_false_returns_the_components(eng, name):
    c = CASES[name]
    eng.set_decode_colour(False)
    try:
        assert eng.read_header(c.file).numcomps == c.src.shape[0]
        np.testing.assert_array_equal(eng.decode(c.file), c.src)
        np.testing.assert_array_equal(eng.decode_window(c.file, (1, 1, 20, 9)), c.src[:, 1:9, 1:20])
    finally:
        eng.set_decode_colour(True)
    np.testing.assert_array_equal(eng.decode(c.file), c.want)


def test_malformed_file_is_refused_on_decode(eng):
    data, boxname = J.malformed()["prec_above_ne"]
    with pytest.raises(RuntimeError) as e:
        eng.decode(data)
    assert boxname in str(e.value) and "Grok" in str(e.value)


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    d = tmp_path_factory.mktemp("capi_colour")
    exe = str(d / "grk_api_colour")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "capi", "grk_api_colour.c"), "-o", exe,
                           "-L", os.path.dirname(G.LIB_PATH), "-lgrok_amd", "-Wl,-rpath," + os.path.dirname(G.LIB_PATH)])
    return exe, d


def _fields(out, tag):
    """The program's report lines of `tag`: (image line as a dict, [component dicts])."""
    rows = [l.split() for l in out.splitlines() if l.startswith(tag + " ")]
    as_dict = lambda t: {t[i]: int(t[i + 1]) for i in range(0, len(t) - 1, 2)}
    head = [r for r in rows if r[1] == "comps"][0]
    comps = [as_dict(r[1:]) for r in rows if r[1] == "comp"]
    return as_dict(head[1:]), comps


@pytest.mark.parametrize("name", ["c1_clamp200", "c5_direct_cdef", "c7_icc"])
def test_grk_api_applies_colour(tool, name):
    c = CASES[name]
    exe, d = tool
    path, raw, icc = d / (name + ".jp2"), d / (name + ".raw"), d / (name + ".icc")
    path.write_bytes(c.file)
    r = subprocess.run([exe, str(path), str(raw), str(icc)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    head, hcomps = _fields(r.stdout, "header")
    # after the header read: the codestream's components, the colr box's space, the ICC bytes
    assert (head["comps"], head["space"], head["applied"]) == (c.src.shape[0], c.colour_space, 0)
    assert [k["prec"] for k in hcomps] == [c.prec] * c.src.shape[0]
    assert head["icc"] == (len(c.icc) if c.icc else 0)
    if c.icc:
        assert icc.read_bytes() == c.icc
    # after the decompress: the same image object holds the output channels
    img, comps = _fields(r.stdout, "image")
    applies = c.lut is not None or c.cdef is not None
    assert (img["comps"], img["space"], img["applied"]) == (c.want.shape[0], c.colour_space, int(applies))
    assert [k["prec"] for k in comps] == c.out_prec
    assert [k["sgnd"] for k in comps] == [0] * len(comps)
    if applies:
        assert [k["type"] for k in comps] == c.typ
    np.testing.assert_array_equal(np.fromfile(raw, np.int32).reshape(c.want.shape), c.want)


@pytest.mark.parametrize("kw", [dict(), dict(tiles=(64, 64), tlm=True, plt=True), dict(irreversible=True),
                                dict(cblk_sty=0x40, tiles=(128, 64), tlm=True, plt=True)])
def test_plain_jp2_decodes_as_its_codestream(eng, kw):
    # the files of test_jp2_encode_matches_oracle (ihdr + colr only) take the unchanged path: the
    # same planes as the bare codestream, the components as channels
    img = synth_image(150, 230, 3, 8, 31).astype(np.int32)
    f = O.encode(img, 8, jp2=True, **kw)
    cs = O.encode(img, 8, **kw)
    assert f.endswith(cs)
    dec = eng.decode(f)
    ci = eng.colour_info()
    assert (ci.num_comps, ci.num_channels, ci.has_palette, ci.has_cdef, ci.colour_space) == (3, 3, 0, 0, 2)
    np.testing.assert_array_equal(dec, eng.decode(cs))
    if not kw.get("irreversible"):
        np.testing.assert_array_equal(dec, img)
    np.testing.assert_array_equal(eng.decode_window(f, (37, 5, 147, 133)), eng.decode_window(cs, (37, 5, 147, 133)))
