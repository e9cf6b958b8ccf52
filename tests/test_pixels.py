"""The output stage without a GPU: the restatement (tests/pixels_ref.py) against answers worked out
by hand from the C, and grok_amd.probe_output, which resolves from the header alone what a decode
under Engine.set_decode_display(force_rgb=...) and set_decode_precision returns, or why it is
refused."""
import os
import re
import subprocess

import numpy as np
import pytest

import grok_amd as G
import oracle as O
import display_ref as R
import display_cases as C
import pixels_ref as P

W, H = 34, 18


def _stream(w, h, sub, prec=8, signed=False, seed=3):
    planes = C.random_planes(w, h, sub, prec, (0, 0), seed, signed)
    kw = dict(mct=False, numres=C.numres_for(w, h, sub))
    if all(d == (1, 1) for d in sub):
        return O.encode(np.stack(planes), prec, signed=signed, **kw)
    return O.encode(planes, prec, signed=signed, size=(w, h), subsampling=sub, **kw)


@pytest.fixture(scope="module")
def streams():
    return {"grey": _stream(W, H, [(1, 1)]), "ga": _stream(W, H, [(1, 1)] * 2), "rgb": _stream(W, H, C.S444),
            "rgb12": _stream(W, H, C.S444, prec=12), "420": _stream(W, H, C.S420)}


# ---------------------------------------------------------------- 1. known answers
def _s(v, old, new, sgnd=False):
    return [int(x) for x in P.scale_component(np.array(v), old, new, sgnd)]


def test_scale_up_is_one_float32_product():
    # 65535 / 4095 = 16.003663 in float32; 1229 * that = 19668.50 just below the tie: exact 19669
    assert _s([1229, 4095], 12, 16) == [19668, 65535]
    # 8191 / 4095 in float32 is 2.00024414..: 2048 * it = 4096.5 exactly in float32: to even
    assert _s([2048, 2049], 12, 13) == [4096, 4098]
    assert _s([340], 9, 16) == [43604]
    v = np.arange(256)
    assert _s(v, 8, 16) == [257 * int(x) for x in v]
    assert _s([-128, -1, 127], 8, 12, sgnd=True) == [-2048, -16, 2032]


def test_scale_down_truncates_toward_zero():
    assert _s([4095, 15], 12, 8) == [255, 0]
    assert _s([-5, -16, -17], 8, 4, sgnd=True) == [0, -1, -1]
    assert _s([7, 300], 12, 12) == [7, 300]


def test_clip_to_the_forced_range():
    assert [int(x) for x in P.clip_component([300, 7], 8, False)] == [255, 7]
    assert [int(x) for x in P.clip_component([-200, 200, -128, 127], 8, True)] == [-128, 127, -128, 127]


def test_gray_to_rgb_and_pack():
    g, a = np.array([[1, 2]]), np.array([[9, 8]])
    planes, comps, cs, rep = P.gray_to_rgb([g, a], [(1, 1, 8, 0), (1, 1, 4, 0)], R.CS_GRAY)
    assert (len(planes), comps, cs, rep) == (4, [(1, 1, 8, 0)] * 3 + [(1, 1, 4, 0)], R.CS_SRGB, True)
    assert P.pack(planes).tolist() == [[[1, 1, 1, 9], [2, 2, 2, 8]]]
    with pytest.raises(ValueError):
        P.gray_to_rgb([g] * 3, [(1, 1, 8, 0)] * 3, R.CS_UNKNOWN)
    planes, comps = P.force_precision([g, a], [(1, 1, 8, 0), (1, 1, 4, 0)], "16S,0C")
    assert planes[0].tolist() == [[257, 514]] and planes[1].tolist() == [[9, 8]]
    assert [c[2] for c in comps] == [16, 4]


def test_parse_precision():
    assert G.parse_precision("8S") == [(8, "S")]
    assert G.parse_precision("8S,12C,0S") == [(8, "S"), (12, "C"), (0, "S")]
    assert G.parse_precision("10") == [(10, "C")] and G.parse_precision("32S") == [(32, "S")]
    assert G.parse_precision(None) == [] and G.parse_precision([]) == []
    assert G.parse_precision([(8, "S"), (0, "C")]) == [(8, "S"), (0, "C")]
    for bad in ("33", "8X", "S", "8s", "8S;9S"):
        with pytest.raises(ValueError):
            G.parse_precision(bad)


def test_kernel_builds_for_gfx950_without_scratch_or_lds(tmp_path):
    src = os.path.join(os.path.dirname(G.__file__), "csrc", "gk_pixels.hip")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "gk_pixels.out")],
                       capture_output=True, text=True, check=True)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    # 3 source types x 3 destination types x (C = 1..4 and the generic kernel)
    assert len(names) == 45 and sum("k_pixels_any" in n for n in names) == 9
    assert len(scratch) == 45 and not any(scratch) and len(lds) == 45 and not any(lds)


# ---------------------------------------------------------------- 2. probe_output
def _refused(data, needle, **kw):
    with pytest.raises(ValueError) as e:
        G.probe_output(data, **kw)
    assert needle in str(e.value), str(e.value)


def test_probe_grey_force_rgb(streams):
    d = G.probe_output(streams["grey"], force_rgb=True)
    assert (d.shapes, d.precisions, d.colour_space) == ([(H, W)] * 3, [8] * 3, R.CS_SRGB)
    assert d.colour.display_applied & 4 and d.replicated and d.info.numcomps == 3
    assert d.colour.num_comps == 1 and d.colour.num_channels == 3
    d = G.probe_output(streams["ga"], force_rgb=True)
    assert (len(d.shapes), d.colour_space, d.colour.display_applied) == (4, R.CS_SRGB, 4)
    # rgb alone names the image grey and leaves it
    d = G.probe_output(streams["grey"], rgb=True)
    assert (len(d.shapes), d.colour_space, d.colour.display_applied) == (1, R.CS_GRAY, 0)


def test_probe_force_rgb_other_colour_spaces(streams):
    _refused(streams["rgb"], "unknown", force_rgb=True)          # a raw 3-component codestream
    f = C.wrap(streams["rgb"], W, H, 3, 8, C.SRGB)
    d = G.probe_output(f, force_rgb=True)                        # sRGB: nothing to do
    assert (len(d.shapes), d.colour_space, d.colour.display_applied) == (3, R.CS_SRGB, 0)
    _refused(C.wrap(streams["rgb"], W, H, 3, 8, C.EYCC), "e-sYCC", force_rgb=True)
    f = C.wrap(streams["420"], W, H, 3, 8, C.SYCC)
    _refused(f, "GK_DISPLAY_RGB", force_rgb=True)
    _refused(streams["420"], "GK_DISPLAY_RGB", force_rgb=True)   # (subsampled chroma counts as sYCC)
    d = G.probe_output(f, rgb=True, force_rgb=True)
    assert (d.shapes, d.colour_space, d.colour.display_applied) == ([(H, W)] * 3, R.CS_SRGB, 1)


def test_probe_precision_list(streams):
    d = G.probe_output(streams["rgb12"], precision="8S")
    assert d.precisions == [8, 8, 8] and d.info.prec == 8
    d = G.probe_output(streams["rgb12"], precision="8S,16C")     # the last entry repeats
    assert d.precisions == [8, 16, 16] and d.info.prec == 16
    d = G.probe_output(streams["rgb12"], precision=[(8, "S"), (0, "C"), (10, "S")])
    assert d.precisions == [8, 12, 10]
    # channels are counted after grey to RGB
    d = G.probe_output(streams["ga"], force_rgb=True, precision="4S,5S,6S,7S")
    assert d.precisions == [4, 5, 6, 7]
    _refused(streams["rgb12"], "17", precision="8S,17S")
    wide = C.set_ssiz(streams["rgb12"], 1, 20)
    _refused(wide, "channel 1", precision="8S")
    assert G.probe_output(wide, precision="8S,0S,8S").precisions == [8, 20, 8]


def test_nothing_set_is_probe_display(streams):
    files = list(streams.values()) + [C.wrap(streams["420"], W, H, 3, 8, C.SYCC)]
    for f in files:
        for kw in (dict(), dict(rgb=True), dict(upsample=True)):
            a, b = G.probe_output(f, **kw), G.probe_display(f, **kw)
            assert (a.shapes, a.precisions, a.signed, a.channels, a.colour_space) == \
                (b.shapes, b.precisions, b.signed, b.channels, b.colour_space)
            for name, _ in G.ColourInfo._fields_:
                x, y = getattr(a.colour, name), getattr(b.colour, name)
                assert (list(x) == list(y)) if hasattr(x, "__len__") else x == y, name
            for name, _ in G.ImageInfo._fields_:
                assert getattr(a.info, name) == getattr(b.info, name), name
