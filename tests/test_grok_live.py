"""The oracle against Grok 9.2.0's own binaries, run live (tests/grok_ref.py; built by
`make -C oracle ref GROK_SRC=...`, which __graft_entry__.build() calls where a source tree is at
hand).  CPU only: the binaries run as child processes on temporary PNM / PGX files.

  * encode: oracle.encode(img, bits, **parse_flags(flags)) == grk_compress's bytes, over
    tests/grok_cases.py::ENCODE (every CLI option family, the parameters of the GPU suites'
    offset / odd-tile / mode-switch / progression / tile-part / rate-control / SOP cases, 8 / 10 /
    12 / 16 bits, 1 and 3 components, signed input through PGX);
  * decode: oracle.decode == grk_decompress, plain and with -l, -r, -d, -t, on Grok's streams,
    which the encode test shows to be the oracle's streams too; equality, 9/7 included;
  * streams Grok's encoder never writes but its decoder reads: COC, QCC and scalar-derived
    quantisation, PPM / PPT, tile-part COD / COC / QCD / QCC / RGN, whole-component RGN,
    subsampled components, as the oracle writes them (the generators of test_coc.py, test_qcc.py,
    test_ppx.py, tile_coding.py, subsampling_cases.py).

What Grok gets wrong or refuses in these families (C.MIXED_CODERS_* among them) is named case by case in
tests/test_grok_defects.py; nothing here is skipped for differing.  Without
the binaries every test here skips with the reason; tests/test_grok_fixtures.py then still holds
the oracle to their recorded output.
"""
import numpy as np
import pytest

import oracle as O
import grok_cases as C
import display_ref
import grok_ref
import subsampling_cases
import test_coc
import test_ppx
import tile_coding
from qcc_cases import CASES as QCC_CASES


@pytest.fixture(autouse=True)
def _binaries():
    grok_ref.need()


_streams = {}


def grok_stream(case):
    if case not in _streams:
        _streams[case] = C.grok_encode(*case)
    return _streams[case]


@pytest.mark.parametrize("case", C.ENCODE, ids=[C.case_id(c) for c in C.ENCODE])
def test_encode_equals_grok(case):
    assert C.oracle_encode(*case) == grok_stream(case)


@pytest.mark.parametrize("case,dflags", C.DECODE, ids=[C.decode_id(d) for d in C.DECODE])
def test_decode_equals_grok(case, dflags):
    cs = grok_stream(case)
    want, meta = grok_ref.decompress(cs, dflags, info=True)
    got = C.oracle_decode(cs, dflags, case[1])
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    _, _, bits, signed = C.image(case[0])
    assert meta == [(bits, signed)] * len(want)


def test_every_option_family_is_covered():
    # the matrix the cases promise: each CLI option, each decode option, each depth, signed
    flags = " ".join(f for _, f in C.ENCODE).split()
    for opt in "-n -b -c -I -r -M -t -X -S -E -q -p -d -T -P -L -u".split():
        assert opt in flags, opt
    for sty in "1 2 4 8 16 32 63 64".split():
        assert any(("-M " + sty) in f.replace(",", " ") + " " for _, f in C.ENCODE), sty
    for div in "RLC":
        assert any(("-u " + div) in f for _, f in C.ENCODE)
    keys = {k for k, _ in C.ENCODE}
    assert {"m8", "m10", "m12", "m16", "rgb", "rgb10", "rgb12", "rgb16", "thin", "one", "p:m12", "s:m16"} <= keys
    dflags = " ".join(d for _, d in C.DECODE).split()
    for opt in "-l -r -d -t".split():
        assert opt in dflags, opt


# ---------------------------------------------------------------- streams only the oracle writes
def _same(got, want):
    """Component by component (a list where the components differ in size)."""
    got = list(got) if not isinstance(got, list) else got
    want = list(want) if not isinstance(want, list) else want
    assert len(got) == len(want)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(np.asarray(g), np.asarray(w))


@pytest.mark.parametrize("name", sorted(set(test_coc.CASES) - set(C.MIXED_CODERS_COC)))
def test_grok_decodes_coc(name):
    cs = test_coc.stream(name)
    assert b"\xff\x53" in cs
    got, meta = grok_ref.decompress(cs, info=True)
    _same(got, O.decode(cs)[0])
    assert [m[0] for m in meta] == test_coc._precs(name)


@pytest.mark.parametrize("name,shape,bits,kw", QCC_CASES, ids=[c[0] for c in QCC_CASES])
def test_grok_decodes_qcc(name, shape, bits, kw):
    from test_qcc import _img
    cs = O.encode(_img(shape, bits, 5), bits, **kw)
    assert b"\xff\x5d" in cs or kw.get("qderived")
    _same(grok_ref.decompress(cs), O.decode(cs)[0])


@pytest.mark.parametrize("kind", ["ppt", "ppm"])
@pytest.mark.parametrize("name", sorted(test_ppx.CASES))
def test_grok_decodes_packed_headers(name, kind):
    cs = test_ppx.stream(name, kind)
    _same(grok_ref.decompress(cs), O.decode(cs)[0])


@pytest.mark.parametrize("name", sorted(set(tile_coding.CASES) - set(C.MIXED_CODERS_TILE)))
def test_grok_decodes_tile_coding(name):
    cs = tile_coding.stream(name)
    want = tile_coding.expected(name)
    _same(O.decode(cs)[0], want)
    _same(grok_ref.decompress(cs), want)


@pytest.mark.parametrize("roi,kw", [((0, 4), {}), ((1, 9), dict(numres=4)), ((2, 3), dict(irreversible=True)),
                                    ((0, 7), dict(tiles=(32, 32), layer_rate=[20.0, 0.0]))])
def test_grok_decodes_whole_component_rgn(roi, kw):
    img, _, bits, _ = C.image("rgb")
    cs = O.encode(img, bits, roi=roi, **kw)
    assert b"\xff\x5e" in cs
    _same(grok_ref.decompress(cs), O.decode(cs)[0])


@pytest.mark.parametrize("dflags,upsample", [("", False), ("-u", True)])
@pytest.mark.parametrize("name", sorted(subsampling_cases.CASES))
def test_grok_decodes_subsampled(name, dflags, upsample):
    # the CLI's display stage follows the decode: three components with subsampled chroma are taken
    # for sYCC and come back as RGB, -u brings every other component to the image grid; the
    # oracle's planes go through the restatement of that stage (tests/display_ref.py)
    W, H, sub, prec, kw = subsampling_cases.CASES[name]
    cs = O.encode(subsampling_cases.planes(name), prec, size=(W, H), **subsampling_cases.oracle_kw(name))
    ox, oy = kw.get("origin") or kw.get("tile_origin") or (0, 0)
    planes = O.decode(cs)[0]
    np.testing.assert_equal([p.shape for p in planes],
                            [subsampling_cases.comp_shape(W, H, dx, dy, (ox, oy)) for dx, dy in sub])
    want = display_ref.post_process(planes, [(dx, dy, prec, False) for dx, dy in sub], 0,
                                    (ox, oy, ox + W, oy + H), rgb=True, upsample=upsample)[0]
    _same(grok_ref.decompress(cs, dflags), want)
