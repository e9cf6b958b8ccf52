"""JP2 colour boxes on encode, on the GPU: with Engine.set_encode_colour the engine's JP2 encodes
carry the boxes of tests/encode_colour_cases.py in front of the codestream they carry today; sYCC
and e-sYCC clear the MCT, in raw codestreams too; the engine decodes its own palette files to the
restatement of tests/jp2_boxes.py; the description is sticky until cleared and leaves no trace
afterwards; and a C program written against Grok's API writes the engine's files."""
import os
import struct
import subprocess

import numpy as np
import pytest

import grok_amd as G
import jp2_boxes as J
import encode_colour_cases as E
from conftest import ROOT

pytestmark = pytest.mark.gpu

CASES = E.cases()
NAMES = sorted(CASES)


@pytest.fixture(scope="module")
def eng():
    e = G.Engine(0)
    yield e
    e.close()


def params(**kw):
    kw.setdefault("numresolution", 3)
    return G.default_params(**kw)


def split(data):
    """(bytes before the jp2c payload, payload) of a JP2 file whose jp2c box is its last."""
    at = data.index(b"jp2c") + 4
    assert struct.unpack(">I", data[at - 8:at - 4])[0] == len(data) - (at - 8)
    return data[:at], data[at:]


def described(eng, c, **kw):
    eng.set_encode_colour(**c.kw)
    try:
        return eng.encode(c.src, c.prec, params=params(**kw))
    finally:
        eng.set_encode_colour()


@pytest.mark.parametrize("name", NAMES)
def test_boxes_and_payload(eng, name):
    c = CASES[name]
    mct = c.src.shape[0] >= 3
    got = described(eng, c, jp2=True, mct=mct)
    head, payload = split(got)
    assert head[:-8] == c.prefix()
    assert head == G.jp2_boxes(c.src.shape, c.prec, len(payload), **c.kw)
    # the codestream is the one an encode without a description carries; sYCC / e-sYCC clear the MCT
    plain_mct = mct and c.space not in ("sycc", "esycc")
    assert payload == eng.encode(c.src, c.prec, params=params(mct=plain_mct))
    assert payload == split(eng.encode(c.src, c.prec, params=params(jp2=True, mct=plain_mct)))[1]
    if c.space in ("sycc", "esycc"):
        assert payload != eng.encode(c.src, c.prec, params=params(mct=True))
        assert described(eng, c, mct=True) == payload              # a raw codestream loses the MCT too
    ci = G.probe_colour(got)
    assert ci.colour_space == E.SPACE[c.space][0]


@pytest.mark.parametrize("name", [n for n in NAMES if CASES[n].palette is not None])
def test_engine_decodes_its_palette_files(eng, name):
    c = CASES[name]
    want, typ = c.expected()
    got = eng.decode(described(eng, c, jp2=True, mct=False))
    np.testing.assert_array_equal(np.asarray(got), want)
    assert [t for t, _ in eng.colour_info().channels()] == typ


def test_round_trip_rgba_pixels(eng):
    x = np.ascontiguousarray(np.moveaxis(CASES["rgba"].src, 0, 2)).astype(np.uint8)
    eng.set_encode_colour(space="srgb", channels=E.RGBA)
    try:
        data = eng.encode_pixels(x, 8, params=params(jp2=True, mct=True))
    finally:
        eng.set_encode_colour()
    assert split(data)[0][:-8] == CASES["rgba"].prefix()
    np.testing.assert_array_equal(eng.decode_pixels(data, sample_bytes=1), x)
    ci = eng.colour_info()
    assert ci.channels() == [(0, 1), (0, 2), (0, 3), (1, 0)] and ci.colour_space == 2


def test_jp2_header_follows_the_description(eng):
    c = CASES["icc_opacity"]
    eng.set_encode_colour(**c.kw)
    try:
        assert eng.jp2_header(c.src.shape, c.prec, 4321) == G.jp2_boxes(c.src.shape, c.prec, 4321, **c.kw)
    finally:
        eng.set_encode_colour()
    assert eng.jp2_header(c.src.shape, c.prec, 4321) == G.jp2_boxes(c.src.shape, c.prec, 4321)


# ---------------------------------------------------------------- history
def test_set_encode_clear_encode_equals_a_fresh_engine(eng):
    c = CASES["sycc"]
    p = params(jp2=True, mct=True)
    described(eng, c, jp2=True, mct=True)
    second = eng.encode(c.src, c.prec, params=p)
    raw = eng.encode(c.src, c.prec, params=params(mct=True))
    fresh = G.Engine(0)
    try:
        assert fresh.encode(c.src, c.prec, params=p) == second
        assert fresh.encode(c.src, c.prec, params=params(mct=True)) == raw
    finally:
        fresh.close()


def test_refused_description_leaves_the_next_encode_unchanged(eng):
    c = CASES["rgba"]
    p = params(jp2=True, mct=True)
    want = eng.encode(c.src, c.prec, params=p)
    with pytest.raises(ValueError, match="icc"):                    # refused when set: nothing stays
        eng.set_encode_colour(space="srgb", icc=E.ICC)
    assert eng.encode(c.src, c.prec, params=p) == want
    eng.set_encode_colour(space="cmyk", channels=[(0, 1), (0, 2), (1, 0)])   # refused by the image it meets
    try:
        with pytest.raises(RuntimeError, match="cdef"):
            eng.encode(c.src[:3], c.prec, params=p)
    finally:
        eng.set_encode_colour()
    assert eng.encode(c.src, c.prec, params=p) == want
    eng.set_encode_colour(space="srgb", palette=(J._lut(4, [8, 8, 8], 1), [8, 8, 8], [(0, 1, 0), (0, 1, 1), (0, 1, 2)]))
    try:
        with pytest.raises(RuntimeError, match="pclr"):             # 8-bit components, four entries
            eng.encode(c.src[:1], c.prec, params=params(jp2=True, mct=False))
    finally:
        eng.set_encode_colour()
    assert eng.encode(c.src, c.prec, params=p) == want


# ---------------------------------------------------------------- the grk_* API
@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    d = tmp_path_factory.mktemp("capi_encode_colour")
    exe = str(d / "grk_api_encode_colour")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "capi", "grk_api_encode_colour.c"), "-o", exe,
                           "-L", os.path.dirname(G.LIB_PATH), "-lgrok_amd", "-Wl,-rpath," + os.path.dirname(G.LIB_PATH)])
    return exe, d


@pytest.mark.parametrize("mode,fmt", [("rgba", "jp2"), ("sycc", "jp2"), ("sycc", "j2k")])
def test_grk_api_writes_the_engines_files(eng, tool, mode, fmt):
    exe, d = tool
    c = CASES[mode]
    raw, out = d / (mode + ".raw"), d / (mode + "." + fmt)
    np.ascontiguousarray(c.src, dtype=np.int32).tofile(raw)
    _, h, w = c.src.shape
    r = subprocess.run([exe, str(raw), str(w), str(h), str(out), mode, fmt], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    got = out.read_bytes()
    assert got == described(eng, c, jp2=fmt == "jp2", mct=True)
    if fmt == "jp2":
        assert split(got)[0][:-8] == c.prefix()
    else:
        assert got == eng.encode(c.src, c.prec, params=params(mct=False))


def test_grk_api_raw_codestream_ignores_the_colour_space(eng, tool):
    """A colour space the JP2 writer refuses (CIELab) does not touch a raw codestream: today's bytes."""
    exe, d = tool
    c = CASES["sycc"]
    raw, out = d / "cie.raw", d / "cie.j2k"
    np.ascontiguousarray(c.src, dtype=np.int32).tofile(raw)
    _, h, w = c.src.shape
    r = subprocess.run([exe, str(raw), str(w), str(h), str(out), "cie", "j2k"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert out.read_bytes() == eng.encode(c.src, c.prec, params=params(mct=True))
    r = subprocess.run([exe, str(raw), str(w), str(h), str(d / "cie.jp2"), "cie", "jp2"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "colour_space" in r.stderr
