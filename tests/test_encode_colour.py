"""JP2 colour boxes on encode, without a GPU: grok_amd.jp2_boxes (gk_jp2_boxes) writes, for every
case of tests/encode_colour_cases.py, the bytes tests/jp2_boxes.py builds by hand in Grok's
write_jp2h order; the engine's header probes read the description back from the file; OpenJPEG
reads the same colour space, profile, alpha flags and palette-expanded planes; and everything the
issue lists as refused raises ValueError naming its box or field."""
import numpy as np
import pytest

import grok_amd as G
import jp2_boxes as J
import oracle as O
import encode_colour_cases as E

CASES = E.cases()
NAMES = sorted(CASES)


@pytest.fixture(scope="module")
def streams():
    """name -> oracle-encoded lossless codestream of the case's components."""
    return {n: O.encode(c.src, c.prec, mct=False, numres=3) for n, c in CASES.items()}


@pytest.mark.parametrize("name", NAMES)
def test_boxes_equal_the_hand_built_file(name, streams):
    c, cs = CASES[name], streams[name]
    got = G.jp2_boxes(c.src.shape, c.prec, len(cs), **c.kw) + cs
    assert got == c.file(cs)


@pytest.mark.parametrize("name", NAMES)
def test_probes_return_the_description(name, streams):
    c, cs = CASES[name], streams[name]
    data = G.jp2_boxes(c.src.shape, c.prec, len(cs), **c.kw) + cs
    want, typ = c.expected()
    ci = G.probe_colour(data)
    grk, enumcs = E.SPACE[c.space]
    assert (ci.colour_space, ci.enumcs, ci.meth) == (grk, enumcs, 2 if c.space == "icc" else 1)
    assert ci.icc_len == (len(c.icc) if c.icc is not None else 0)
    assert G.probe_icc(data) == (c.icc or b"")
    assert bool(ci.has_palette) == (c.palette is not None) and bool(ci.has_cdef) == (c.cdef is not None)
    if c.palette is not None:
        assert (ci.palette_entries, ci.palette_columns) == c.lut.shape
    assert ci.num_comps == c.src.shape[0] and ci.num_channels == want.shape[0]
    assert [t for t, _ in ci.channels()] == typ
    if c.cdef is not None:   # each channel's Typ / Asoc as written (no case reorders its channels)
        assert ci.channels() == [(t, a) for _, t, a in c.cdef]
    precs = c.precs if c.palette is not None else [c.prec] * c.src.shape[0]
    assert G.probe_components(data, precision=True) == [(1, 1, p, False) for p in precs]


@pytest.mark.skipif(not J.opj_available(), reason="libopenjp2 (Pillow) not present")
@pytest.mark.parametrize("name", NAMES)
def test_openjpeg_reads_the_same(name, streams):
    c, cs = CASES[name], streams[name]
    got = J.opj_decode_jp2(G.jp2_boxes(c.src.shape, c.prec, len(cs), **c.kw) + cs)
    want, typ = c.expected()
    np.testing.assert_array_equal(got["planes"], want)
    enumcs = E.SPACE[c.space][1]
    if enumcs in J.OPJ_CLRSPC:
        assert got["color_space"] == J.OPJ_CLRSPC[enumcs]
    assert got["icc"] == (c.icc or b"")
    if c.cdef is not None:   # OpenJPEG keeps the cdef Typ of each channel in `alpha`
        assert got["alpha"] == typ
    else:
        assert not any(got["alpha"])


def test_xlbox_geometry_with_cdef():
    c, want = E.xl_prefix()
    assert G.jp2_boxes(E.XL_SHAPE, 8, E.XL_CS_LEN, **c.kw) == want


def test_forced_leading_entries():
    """initCompress :850-857: the first color_channels entries are (i, 0, i + 1) whatever the image says."""
    got = G.jp2_boxes((4, 8, 8), 8, 100, space="srgb", channels=[(1, 0), (0, 3), (0, 1), (1, 0)])
    assert got == G.jp2_boxes((4, 8, 8), 8, 100, space="srgb", channels=E.RGBA)
    assert J.cdef([(0, 0, 1), (1, 0, 2), (2, 0, 3), (3, 1, 0)]) in got


def test_no_colour_arguments_write_todays_bytes():
    for nc, h, w, prec, signed, n in ((1, 16, 16, 8, False, 1000), (3, 33, 47, 12, True, 70000), (4, 20000, 20000, 8, False, 5 << 30)):
        assert G.jp2_boxes((nc, h, w), prec, n, signed=signed) == O.jp2_header(w, h, nc, prec, n, signed=signed)


def test_all_colour_types_write_no_cdef():
    assert G.jp2_boxes((3, 8, 8), 8, 100, space="srgb", channels=[(0, 1), (0, 2), (0, 3)]) == G.jp2_boxes((3, 8, 8), 8, 100)
    assert G.jp2_boxes((1, 8, 8), 8, 100, space="grey") == G.jp2_boxes((1, 8, 8), 8, 100)


REFUSALS = E.refusals()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_name_the_box_or_field(name):
    shape, prec, signed, kw, what = REFUSALS[name]
    with pytest.raises(ValueError) as e:
        G.jp2_boxes(shape, prec, 1000, signed=signed, **kw)
    assert what in str(e.value), str(e.value)


def test_encode_colour_layout_matches_header(tmp_path):
    """The ctypes mirror of gk_encode_colour / gk_cmap_entry has the header's layout."""
    import ctypes
    import os
    import subprocess
    from conftest import ROOT
    src = tmp_path / "layout.c"
    src.write_text('#include "grok_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(gk_encode_colour), offsetof(gk_encode_colour, icc_len),\n'
                   '  offsetof(gk_encode_colour, asoc), offsetof(gk_encode_colour, palette_columns), offsetof(gk_encode_colour, cmap),\n'
                   '  sizeof(gk_cmap_entry)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    T = G.EncodeColour
    assert got == [ctypes.sizeof(T), T.icc_len.offset, T.asoc.offset, T.palette_columns.offset, T.cmap.offset,
                   ctypes.sizeof(G.CmapEntry)]
