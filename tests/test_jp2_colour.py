"""JP2 colour boxes without a GPU: the numpy restatement of Grok's palette / channel-definition
rules (tests/jp2_boxes.py) is pinned to OpenJPEG's JP2 decode, and the engine's header probes
report the output channels, colour space, ICC profile and cdef types of every case file and
refuse every malformed one by the name of the box at fault."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import grok_amd as G
import jp2_boxes as J
from conftest import ROOT

CASES = J.cases()
NAMES = sorted(CASES)


@pytest.mark.skipif(not J.opj_available(), reason="libopenjp2 (Pillow) not present")
@pytest.mark.parametrize("name", NAMES)
def test_expected_equals_openjpeg(name):
    c = CASES[name]
    got = J.opj_decode_jp2(c.file)
    np.testing.assert_array_equal(got["planes"], c.want)
    assert got["prec"] == c.out_prec
    if c.cdef is not None:   # OpenJPEG keeps the cdef Typ of each channel in `alpha`
        assert got["alpha"] == c.typ[:len(got["alpha"])]
    if c.enumcs in J.OPJ_CLRSPC:
        assert got["color_space"] == J.OPJ_CLRSPC[c.enumcs]
    if c.icc is not None:
        assert got["icc"] == c.icc


@pytest.mark.parametrize("name", NAMES)
def test_probes_report_output_channels(name):
    c = CASES[name]
    nch, h, w = c.want.shape
    info = G.probe_header(c.file)
    assert (info.numcomps, info.w, info.h, info.prec) == (nch, w, h, max(c.out_prec))
    comps = G.probe_components(c.file, precision=True)
    assert comps == [(1, 1, p, False) for p in c.out_prec]
    ci = G.probe_colour(c.file)
    assert ci.num_channels == nch and ci.num_comps == c.src.shape[0]
    assert ci.colour_space == c.colour_space
    assert ci.enumcs == (c.enumcs or 0) and ci.meth == (2 if c.icc is not None else 1)
    assert bool(ci.has_palette) == (c.lut is not None) and bool(ci.has_cdef) == (c.cdef is not None)
    if c.lut is not None:
        assert (ci.palette_entries, ci.palette_columns) == c.lut.shape
    assert [t for t, _ in ci.channels()] == c.typ
    if c.cdef is not None:   # position asoc - 1 holds the colour channel with that association
        want = {a - 1: a for _, t, a in c.cdef if t == 0 and a}
        for k, a in want.items():
            assert ci.channels()[k] == (0, a)
        assert ci.channels()[3] == (1, 0)   # (both cdef cases: a whole-image opacity last)
    assert ci.icc_len == (len(c.icc) if c.icc is not None else 0)


def test_icc_profile_bytes():
    c = CASES["c7_icc"]
    assert G.probe_icc(c.file) == c.icc
    assert G.probe_icc(CASES["c7_sycc"].file) == b""
    assert G.probe_icc(c.cs) == b""   # a raw codestream


def test_raw_codestream_reports_components():
    c = CASES["c5_direct_cdef"]
    assert G.probe_header(c.cs).numcomps == 2
    ci = G.probe_colour(c.cs)
    assert (ci.num_comps, ci.num_channels, ci.has_palette, ci.has_cdef, ci.colour_space) == (2, 2, 0, 0, 0)


MALFORMED = J.malformed()


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_boxes_are_refused_by_name(name):
    data, boxname = MALFORMED[name]
    for probe in (G.probe_colour, G.probe_header, G.probe_components):
        with pytest.raises(ValueError) as e:
            probe(data)
        assert boxname in str(e.value), str(e.value)
    if name == "prec_above_ne":
        assert "Grok" in str(e.value)


def test_pclr_without_cmap_is_dropped():
    data, src = J.pclr_without_cmap()
    info = G.probe_header(data)
    assert (info.numcomps, info.prec) == (1, 8)
    ci = G.probe_colour(data)
    assert (ci.num_channels, ci.has_palette, ci.colour_space) == (1, 0, 3)
    assert G.probe_components(data, precision=True) == [(1, 1, 8, False)]
    if J.opj_available():
        np.testing.assert_array_equal(J.opj_decode_jp2(data)["planes"], src)


def test_colour_info_layout_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include "grok_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void){printf("%zu %zu %zu %zu %d\\n", sizeof(gk_colour_info), offsetof(gk_colour_info, num_channels),'
                   ' offsetof(gk_colour_info, typ), offsetof(gk_colour_info, asoc), GK_MAX_CHANNELS);return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(G.ColourInfo), G.ColourInfo.num_channels.offset, G.ColourInfo.typ.offset,
                   G.ColourInfo.asoc.offset, G.GK_MAX_CHANNELS]
