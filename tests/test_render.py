"""The render stage without a GPU: the rule restated in numpy (tests/render_ref.py) against answers
worked out by hand, Levels.window on hand-written histograms, grok_amd.probe_render (its answers
and every refusal, from the header of committed fixtures) and the C ABI of the new calls."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, FIXTURES
import grok_amd as G
import oracle as O
import render_ref as R

FX = {f.name: f for f in FIXTURES}
MONO16, RGB12, RGB8 = FX["mono16_noise"].cs, FX["rgb12_97"].cs, FX["rgb8_tiny"].cs


def _l(v, lo, hi):
    return R.level(np.array(v), lo, hi).tolist()


# ---------------------------------------------------------------- 1. the rule, by hand
def test_window_known_answers():
    # (0, 4095): t = floor((510 v + 4095) / 8190)
    # v = 2048: (1044480 + 4095) / 8190 = 128.03 -> 128;  v = 8: 8175 / 8190 -> 0;  v = 9: 8685 / 8190 -> 1
    assert _l([2048, 8, 9, 4095, 0], 0, 4095) == [128, 0, 1, 255, 0]
    # clamping: below lo and above hi
    assert _l([-5, 5000, 70000], 0, 4095) == [0, 255, 255]
    # (100, 355): span 255, t = floor((510 (v - 100) + 255) / 510) = v - 100 (the half never carries)
    assert _l([100, 101, 227, 354, 355], 100, 355) == [0, 1, 127, 254, 255]
    # (0, 2): v = 1 -> (510 + 2) / 4 = 128
    assert _l([0, 1, 2], 0, 2) == [0, 128, 255]


def test_window_of_width_one():
    # hi - lo = 1: (510 (u - lo) + 1) / 2 -> 0 and 255
    assert _l([6, 7, 8, 9], 7, 8) == [0, 0, 255, 255]
    assert _l([-3, -2], -3, -2) == [0, 255]


def test_full_int32_window():
    lo, hi = -2 ** 31, 2 ** 31 - 1
    # span = 2^32 - 1; v = lo -> 0, v = hi -> 255, v = 0: (510 * 2^31 + 2^32 - 1) / (2^33 - 2) = 128.0..: 128
    # v = -1: (510 (2^31 - 1) + 2^32 - 1) / (2^33 - 2) = 127.99999997 -> 127
    assert _l([lo, hi, 0, -1], lo, hi) == [0, 255, 128, 127]
    assert R.level(np.array([hi], np.int32), lo, hi).dtype == np.int64


def test_inverted_window():
    # lo > hi: 255 - level(v; hi, lo)
    assert _l([2048, 8, 9, 4095, 0, 9000], 4095, 0) == [127, 255, 254, 0, 255, 0]
    assert _l([7, 8], 8, 7) == [255, 0]
    with pytest.raises(ValueError):
        R.level(np.array([1]), 5, 5)


def test_signed_window():
    # (-1000, 1000): span 2000; v = 0 -> (510000 + 2000) / 4000 = 128; v = -1000 -> 0; v = -996: (2040 + 2000) / 4000 -> 1
    assert _l([0, -1000, -996, -997, 1000, -32768], -1000, 1000) == [128, 0, 1, 0, 255, 0]


def test_curve_and_channel_entries():
    pix = np.array([[[0, 4095, 2048]]])                    # one pixel, three channels
    inv = np.arange(255, -1, -1).astype(np.uint8)
    assert R.render(pix, "window", [(0, 4095)]).tolist() == [[[0, 255, 128]]]          # entry 0 serves every channel
    assert R.render(pix, "window", [(0, 4095), (4095, 0)]).tolist() == [[[0, 0, 127]]]   # entry 1 serves channels 1 and 2
    assert R.render(pix, "window", [(0, 4095)], curve=inv).tolist() == [[[255, 0, 127]]]
    g = R.gamma_curve(2.0)                                 # round(255 sqrt(t / 255)): 64 -> 127.75 -> 128
    assert (g[0], g[255], g[64]) == (0, 255, 128) and (G.gamma_curve(2.0) == g).all()
    assert (R.gamma_curve(1.0) == np.arange(256)).all()


def test_map_through_a_ramp_table():
    ramp = np.stack([np.arange(256), 255 - np.arange(256), np.full(256, 7)], axis=1).astype(np.uint8)
    pix = np.array([[[0], [2048], [4095]]])
    assert R.render(pix, "map", [(0, 4095)], map=ramp).tolist() == [[[0, 255, 7], [128, 127, 7], [255, 0, 7]]]
    with pytest.raises(AssertionError):
        R.render(np.zeros((1, 1, 2), int), "map", [(0, 1)], map=ramp)


def test_blend_grey_composite_and_saturation():
    # one channel tinted white: (2 * 255 t + 255) / 510 = t
    pix = np.array([[[0], [9], [2048], [4095]]])
    out = R.render(pix, "blend", [(0, 4095)], tints=[(255, 255, 255)])
    assert out[0, :, 0].tolist() == [0, 1, 128, 255] and (out[:, :, 0] == out[:, :, 1]).all() and (out[:, :, 1] == out[:, :, 2]).all()
    # red + green on two channels: t = (255, 128) -> R = 255, G = 128, B = 0
    pix = np.array([[[4095, 2048]]])
    assert R.render(pix, "blend", [(0, 4095)], tints=[(255, 0, 0), (0, 255, 0)]).tolist() == [[[255, 128, 0]]]
    # two channels on the same colour saturate: (2 (255 * 200 + 255 * 200) + 255) / 510 = 400 -> 255
    assert R.render(pix, "blend", [(0, 1)], tints=[(200, 0, 0)]).tolist() == [[[255, 0, 0]]]
    # a half tint rounds half up: t = 255, tint 1 -> (510 + 255) / 510 = 1;  t = 127, tint 1 -> (254 + 255) / 510 = 0
    assert R.render(np.array([[[1]]]), "blend", [(0, 1)], tints=[(1, 0, 0)]).tolist() == [[[1, 0, 0]]]
    # a zero tint leaves its channel out
    assert R.render(pix, "blend", [(0, 4095)], tints=[(0, 0, 0), (0, 0, 255)]).tolist() == [[[0, 0, 128]]]


def test_bin_rule():
    v = np.array([-7, -5, -4, -1, 0, 3, 4, 100])
    # origin -4, shift 2 (bins of 4): floor((v + 4) / 4) = -1, -1, 0, 0, 1, 1, 2, 26 -> clamped into 0 .. 3
    assert R.bin_of(v, -4, 2, 4).tolist() == [0, 0, 0, 0, 1, 1, 2, 3]
    assert R.bin_of(v, 0, 0, 1).tolist() == [0] * 8
    s = R.stats(v.reshape(2, 4, 1), bins=4, entries=[(-4, 2)])[0]
    assert (s["min"], s["max"], s["sum"], s["count"], s["hist"].tolist()) == (-7, 100, 90, 8, [4, 2, 1, 1])
    assert R.auto_bins(10, 10 + 4095, 4096) == (10, 0) and R.auto_bins(10, 10 + 4096, 4096) == (10, 1)
    assert R.auto_bins(-32768, 32767, 4096) == (-32768, 4)


# ---------------------------------------------------------------- 2. Levels.window
def _levels(hist, origin=0, shift=0):
    hist = np.array(hist, np.uint64).reshape(1, -1)
    n = int(hist.sum())
    st = [G.ChannelLevels(0, 0, 0, n)]
    return G.Levels(st, hist, [origin], [shift], None)


def test_levels_window_by_hand():
    h = [0, 10, 20, 30, 40, 0]                         # N = 100, cumulative 0 10 30 60 100 100
    lv = _levels(h, origin=100, shift=0)
    assert lv.window(0, 1000) == [(101, 104)]          # first non-empty bin .. the bin that reaches 100
    assert lv.window(100, 900) == [(101, 104)]         # reaches 10 in bin 1; 90 in bin 4
    assert lv.window(101, 600) == [(102, 103)]         # 11 -> bin 2; 60 -> bin 3
    assert lv.window(500, 500, per=1000) == [(103, 104)]   # both in bin 3: they meet, hi = lo + 1
    lv = _levels(h, origin=-50, shift=3)               # bins of 8 from -50
    assert lv.window(0, 1000) == [(-42, -11)]          # bin 1 starts at -42; bin 4 ends at -50 + 40 - 1
    assert lv.window(300, 300) == [(-34, -27)]         # bin 2: -34 .. -27
    for args in ((0, 1000), (100, 900), (101, 600), (500, 500), (0, 0), (1000, 1000)):
        for origin, shift in ((100, 0), (-50, 3)):
            assert _levels(h, origin, shift).window(*args) == [R.percentile_window(h, origin, shift, *args)]


def test_levels_window_all_mass_in_one_bin():
    lv = _levels([0, 0, 77, 0], origin=5)
    assert lv.window(0, 1000) == [(7, 8)] and lv.window(20, 980) == [(7, 8)]
    lv = _levels([0, 0, 77, 0], origin=5, shift=4)     # bin 2: 37 .. 52
    assert lv.window(0, 1000) == [(37, 52)]
    # low = 0 asks for at least one pixel; high = 0 asks for none and meets lo
    assert _levels([0, 3, 0, 9]).window(0, 0) == [(1, 2)]
    assert _levels([0, 3, 0, 9]).window(1000, 1000) == [(3, 4)]
    with pytest.raises(ValueError):
        lv.window(600, 400)


# ---------------------------------------------------------------- 3. probe_render
def _t(r):
    return (r.channels, r.prec, r.sgnd, r.colour_space)


RAMP = np.stack([np.arange(256)] * 3, axis=1).astype(np.uint8)


def test_probe_render_answers():
    assert _t(G.probe_render(MONO16)) == (1, 16, 0, 0)                          # no render: the output as it is (a raw codestream: unknown)
    assert _t(G.probe_render(RGB12)) == (3, 12, 0, 0)
    assert _t(G.probe_render(RGB12, precision="8S")) == (3, 8, 0, 0)
    assert _t(G.probe_render(MONO16, "window", [(0, 3000)])) == (1, 8, 0, 0)
    assert _t(G.probe_render(RGB12, "window", [(0, 4095)])) == (3, 8, 0, 0)
    assert _t(G.probe_render(RGB12, "window", [(0, 4095), (9, 1), (-5, 5)], gamma=2.2)) == (3, 8, 0, 0)
    assert _t(G.probe_render(MONO16, "map", [(65535, 0)], map=RAMP)) == (3, 8, 0, 2)
    assert _t(G.probe_render(MONO16, "blend", [(0, 3000)], tints=[(0, 255, 0)])) == (3, 8, 0, 2)
    assert _t(G.probe_render(RGB12, "blend", [(0, 4095)], tints=[(255, 0, 0), (0, 255, 0), (0, 0, 255)])) == (3, 8, 0, 2)
    assert _t(G.probe_render(MONO16, "window", [(0, 255)], force_rgb=True)) == (3, 8, 0, 2)   # grey to RGB, then windowed
    assert _t(G.probe_render(MONO16, "window", [(-2 ** 31, 2 ** 31 - 1)])) == (1, 8, 0, 0)


def _refused(data, needle, *a, **kw):
    with pytest.raises(ValueError) as e:
        G.probe_render(data, *a, **kw)
    assert needle in str(e.value), str(e.value)


def _raw(mode, n, ch=None, curve=None, map=None):
    """gk_probe_render with a description the Python side would not build."""
    lib = G.load_library()
    arr = (G.RenderChannel * 17)()
    for k, (lo, hi, tint) in enumerate(ch or []):
        arr[k] = G.RenderChannel(lo, hi, (ctypes.c_uint8 * 3)(*tint))
    r = G.Render(mode, n, arr if ch is not None else None, None, None)
    if map is not None:
        r.map = map.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    b = np.frombuffer(MONO16, np.uint8)
    msg = ctypes.create_string_buffer(512)
    res = G.RenderResult()
    rc = lib.gk_probe_render(b.ctypes.data, len(b), 0, None, 0, ctypes.byref(r), ctypes.byref(res), msg, 512)
    return rc, msg.value.decode()


def test_probe_render_refusals():
    assert _raw(4, 1, [(0, 1, (0, 0, 0))]) == (-1, "render: mode 4 (1 window, 2 map, 3 blend)")
    assert _raw(1, 0, [(0, 1, (0, 0, 0))]) == (-1, "render: 0 channel entries (1 .. 16)")
    assert _raw(1, 17, [(0, 1, (0, 0, 0))] * 17) == (-1, "render: 17 channel entries (1 .. 16)")
    assert _raw(1, 1, None) == (-1, "render: no channel entries")
    assert _raw(1, 3, [(0, 1, (0, 0, 0)), (4, 9, (0, 0, 0)), (7, 7, (0, 0, 0))]) == \
        (-1, "render: entry 2 has lo == hi (7): an empty window")
    assert _raw(2, 1, [(0, 1, (0, 0, 0))]) == (-1, "render: map mode without a 256 x 3 table")
    assert _raw(3, 2, [(0, 1, (0, 0, 0))] * 2) == (-1, "render: blend mode with every tint zero")
    assert _raw(0, 0)[0] == 0 and _raw(1, 1, [(0, 1, (0, 0, 0))])[0] == 0
    _refused(MONO16, "entry 0 has lo == hi (12)", "window", [(12, 12)])
    _refused(RGB12, "map mode on 3 output channels (it takes exactly one)", "map", [(0, 4095)], map=RAMP)
    _refused(MONO16, "map mode on 3 output channels", "map", [(0, 4095)], map=RAMP, force_rgb=True)
    # tints that exist only past the image's channels: entry 1 never serves a one-channel image
    _refused(MONO16, "every tint of the image's 1 channels zero", "blend", [(0, 9)], tints=[(0, 0, 0), (255, 0, 0)])
    c17 = O.encode(np.zeros((17, 7, 9), np.int32), 8, mct=False, numres=2)
    _refused(c17, "17 output channels (at most 16)", "blend", [(0, 255)], tints=[(1, 1, 1)])
    _refused(c17, "17 output channels (at most 16)", "window", [(0, 255)])
    _refused(RGB12, "17", "window", [(0, 255)], precision="8S,17S")           # what the pixel calls refuse from the header
    _refused(MONO16[:40], "", "window", [(0, 255)])
    for bad in (dict(mode="tint"), dict(mode="window", windows=[(0, 2 ** 31)]), dict(mode="blend", windows=[(0, 1)], tints=[(256, 0, 0)]),
                dict(mode="window", windows=[(0, 1)], curve=np.zeros(255, np.uint8)),
                dict(mode="map", windows=[(0, 1)], map=np.zeros((256, 4), np.uint8)),
                dict(mode="window", windows=[(0, 1)], curve=np.zeros(256, np.uint8), gamma=2.0)):
        with pytest.raises(ValueError):
            G.probe_render(MONO16, **bad)


# ---------------------------------------------------------------- 4. the ABI and the kernels
def test_abi_declared_exported_and_listed(tmp_path):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "grok_amd.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", G.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for sym in ("gk_set_decode_render", "gk_probe_render", "gk_decode_levels"):
        assert re.search(r"^int %s\s*\(" % sym, txt, flags=re.M), sym
        assert sym in exported and sym in G.EXPORTS
    src = tmp_path / "layout.c"
    src.write_text('#include "grok_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %u %u %u %u %u\\n", sizeof(gk_render_channel),'
                   ' sizeof(gk_render), sizeof(gk_render_result), sizeof(gk_levels_bins), sizeof(gk_channel_levels),'
                   ' offsetof(gk_render_channel, tint), offsetof(gk_render, curve), offsetof(gk_render, map),'
                   ' offsetof(gk_channel_levels, count), GK_RENDER_WINDOW, GK_RENDER_MAP, GK_RENDER_BLEND,'
                   ' GK_RENDER_MAX_CHANNELS, GK_LEVELS_MAX_BINS);return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(G.RenderChannel), ctypes.sizeof(G.Render), ctypes.sizeof(G.RenderResult),
                   ctypes.sizeof(G.LevelsBins), ctypes.sizeof(G.ChannelLevels), G.RenderChannel.tint.offset,
                   G.Render.curve.offset, G.Render.map.offset, G.ChannelLevels.count.offset, G.GK_RENDER_WINDOW,
                   G.GK_RENDER_MAP, G.GK_RENDER_BLEND, G.GK_RENDER_MAX_CHANNELS, G.GK_LEVELS_MAX_BINS]


def test_kernels_build_for_gfx950_without_scratch(tmp_path):
    csrc = os.path.join(os.path.dirname(G.__file__), "csrc")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, "gk_render.hip"), "-o",
                        str(tmp_path / "gk_render.out")], capture_output=True, text=True, check=True)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == 2 and "k_render" in names[0] and "k_levels" in names[1]
    assert scratch == [0, 0]
    assert lds == [1024, 0]   # k_render: the curve and the map; k_levels: the histogram is sized by the launch
    assert "gk_render.hip" in open(os.path.join(os.path.dirname(G.__file__), "build.py")).read()
    # one definition of the area average: the header, included by both
    for f in ("gk_view.hip", "gk_render.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "gk_area.h"' in text and "round_div(int64_t" not in text
