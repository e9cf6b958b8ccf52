"""Views without a GPU: the resampling rule restated in numpy (tests/view_ref.py) against answers
worked out by hand, grok_amd.probe_view (the engine's own size / reduce resolution and its
refusals, from the header alone), grok_amd.parse_iiif, and the C ABI of the two new calls."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import grok_amd as G
import oracle as O
import display_cases as C
import view_ref as V


def _img(w, h, nc=3, prec=8, seed=5, signed=False):
    return np.stack(C.random_planes(w, h, [(1, 1)] * nc, prec, seed=seed, signed=signed))


@pytest.fixture(scope="module")
def streams():
    sub = C.random_planes(34, 18, C.S420, 8, seed=2)
    return {
        "rgb": O.encode(_img(53, 37), 8, mct=False, numres=3),
        "tiled": O.encode(_img(64, 48), 8, mct=False, numres=3, tiles=(32, 32)),
        "one": O.encode(_img(64, 48, nc=1), 8, mct=False, numres=1),
        "deep": O.encode(_img(200, 120, nc=1), 8, mct=False, numres=6),
        "rgb12": O.encode(_img(34, 18, prec=12), 12, mct=False, numres=3),
        "420": O.encode(sub, 8, size=(34, 18), subsampling=C.S420, mct=False, numres=C.numres_for(34, 18, C.S420)),
        "c17": O.encode(_img(9, 7, nc=17), 8, mct=False, numres=2),
        "origin": O.encode(_img(40, 30, nc=1), 8, mct=False, numres=3, origin=(5, 3)),
    }


# ---------------------------------------------------------------- 1. the rule, by hand
def _r(a, ow, oh):
    a = np.asarray(a)
    return V.resample(a[:, :, None] if a.ndim == 2 else a, ow, oh)


def test_halves_round_up():
    assert _r([[1, 2], [2, 2]], 1, 1).tolist() == [[[2]]]           # sum 7, mean 1.75
    assert _r([[1, 2]], 1, 1).tolist() == [[[2]]]                   # 1.5 rounds up
    assert _r([[0, 1]], 1, 1).tolist() == [[[1]]]                   # 0.5 rounds up


def test_signed_floor_division():
    assert _r([[-1, -2], [-2, -2]], 1, 1).tolist() == [[[-2]]]      # sum -7, mean -1.75
    assert _r([[-1, -2]], 1, 1).tolist() == [[[-1]]]                # -1.5 rounds up, to -1
    assert _r([[-1, 0]], 1, 1).tolist() == [[[0]]]                  # -0.5 rounds up, to 0


def test_three_to_two_columns():
    assert V.weights(3, 2).tolist() == [[2, 1, 0], [0, 1, 2]]
    # (2 * 10 + 1 * 20) / 3 = 13.33, (20 + 2 * 60) / 3 = 46.67
    assert _r([[10, 20, 60]], 2, 1).tolist() == [[[13], [47]]]


def test_identity_constant_and_block_mean():
    a = _img(7, 5, prec=12, signed=True).transpose(1, 2, 0)
    np.testing.assert_array_equal(V.resample(a, 7, 5), a)
    c = np.full((9, 11, 2), -37)
    for ow, oh in ((11, 9), (7, 4), (1, 1), (10, 8), (3, 9)):
        assert (V.resample(c, ow, oh) == -37).all()
    a = _img(12, 8, prec=10, signed=True, seed=9).transpose(1, 2, 0).astype(np.int64)
    for fx, fy in ((2, 2), (3, 4), (4, 1), (12, 8)):
        blocks = a.reshape(8 // fy, fy, 12 // fx, fx, 3).sum(axis=(1, 3))
        n = fx * fy
        np.testing.assert_array_equal(V.resample(a, 12 // fx, 8 // fy), (2 * blocks + n) // (2 * n))


def test_weights_sum_to_the_source_size():
    for rn in range(1, 41):
        for on in range(1, rn + 1):
            w = V.weights(rn, on)
            assert (w.sum(axis=1) == rn).all() and (w.sum(axis=0) == on).all() and (w >= 0).all()


def test_orientation():
    a = np.arange(6).reshape(2, 3, 1)
    assert V.orient(a, 90)[:, :, 0].tolist() == [[3, 0], [4, 1], [5, 2]]
    assert V.orient(a, 180)[:, :, 0].tolist() == [[5, 4, 3], [2, 1, 0]]
    assert V.orient(a, 270)[:, :, 0].tolist() == [[2, 5], [1, 4], [0, 3]]
    assert V.orient(a, 0, True)[:, :, 0].tolist() == [[2, 1, 0], [5, 4, 3]]
    assert V.orient(a, 90, True)[:, :, 0].tolist() == [[5, 2], [4, 1], [3, 0]]


def test_pillow_box_at_integer_ratios():
    Image = pytest.importorskip("PIL.Image")
    a = np.random.RandomState(4).randint(0, 256, (64, 64, 3)).astype(np.uint8)
    for ow, oh in ((32, 32), (16, 32), (8, 8)):
        pil = np.asarray(Image.fromarray(a).resize((ow, oh), Image.BOX)).astype(np.int64)
        # Pillow rounds to 8 bits between its horizontal and its vertical pass
        assert np.abs(pil - V.resample(a, ow, oh)).max() <= 1


# ---------------------------------------------------------------- 2. probe_view
def _t(r):
    return (r.reduce, (r.rx0, r.ry0, r.rx1, r.ry1), (r.out_w, r.out_h), (r.pix_w, r.pix_h))


def test_probe_size_forms(streams):
    s = streams["rgb"]   # 53 x 37
    assert _t(G.probe_view(s, size=(29, 17))) == (0, (0, 0, 53, 37), (29, 17), (29, 17))
    assert _t(G.probe_view(s, size=(53, 37))) == (0, (0, 0, 53, 37), (53, 37), (53, 37))
    assert _t(G.probe_view(s, width=26)) == (1, (0, 0, 27, 19), (26, 18), (26, 18))       # 26 * 37 / 53 = 18.15
    assert _t(G.probe_view(s, height=9)) == (2, (0, 0, 14, 10), (13, 9), (13, 9))         # 9 * 53 / 37 = 12.89
    assert _t(G.probe_view(s, size=(20, 20), fit=True))[2] == (20, 14)                    # 20 * 37 / 53 = 13.96
    assert _t(G.probe_view(s, size=(40, 10), fit=True))[2] == (14, 10)                    # 10 * 53 / 37 = 14.32
    assert _t(G.probe_view(s, size=(1, 1))) == (2, (0, 0, 14, 10), (1, 1), (1, 1))
    assert _t(G.probe_view(s, width=1))[2] == (1, 1)                                      # 37 / 53 rounds to 1
    assert _t(G.probe_view(streams["deep"], height=1))[2] == (2, 1)                       # 200 / 120 = 1.67
    assert _t(G.probe_view(streams["deep"], region=(0, 0, 200, 1), width=2))[2] == (2, 1)  # the height: at least 1
    r = G.probe_view(s, size=(13, 9))
    assert (r.channels, r.prec, r.sgnd) == (3, 8, 0)
    # a region given as all 0 is the whole image, as None is
    for kw in (dict(size=(1, 5)), dict(width=26, rotate=90), dict(size=(20, 20), fit=True)):
        assert _t(G.probe_view(s, region=(0, 0, 0, 0), **kw)) == _t(G.probe_view(s, **kw))
    assert _t(G.probe_view(s, region=(0, 0, 0, 0), size=(1, 5))) == (2, (0, 0, 14, 10), (1, 5), (1, 5))
    assert G.probe_view(streams["rgb12"], size=(5, 5), precision="8S").prec == 8


def test_probe_matches_the_restatement(streams):
    rng = np.random.RandomState(11)
    for name, w, h, numres, origin in (("rgb", 53, 37, 3, (0, 0)), ("deep", 200, 120, 6, (0, 0)), ("origin", 40, 30, 3, (5, 3))):
        for _ in range(60):
            x0, y0 = rng.randint(0, w), rng.randint(0, h)
            x1, y1 = rng.randint(x0 + 1, w + 1), rng.randint(y0 + 1, h + 1)
            bw, bh = x1 - x0, y1 - y0
            form = rng.randint(4)
            kw = [dict(width=rng.randint(1, bw + 1)), dict(height=rng.randint(1, bh + 1)),
                  dict(size=(rng.randint(1, bw + 1), rng.randint(1, bh + 1))),
                  dict(size=(rng.randint(1, bw + 1), rng.randint(1, bh + 1)), fit=True)][form]
            ow, oh = kw.get("size", (kw.get("width", 0), kw.get("height", 0)))
            size = V.resolve_size(bw, bh, ow, oh, kw.get("fit", False))
            assert size == G._view_size(bw, bh, ow, oh, kw.get("fit", False))   # (the binding's, for device bytes)
            red = V.choose_reduce((x0, y0, x1, y1), size[0], size[1], numres - 1, origin)
            got = G.probe_view(streams[name], region=(x0, y0, x1, y1), rotate=90, **kw)
            assert _t(got) == (red, V.reduced((x0, y0, x1, y1), red, origin), size, size[::-1])


def test_probe_reduce_and_rectangle(streams):
    # odd region edges across the 32 x 32 tiles of a 64 x 48 image: 56 x 41 at full resolution
    s = streams["tiled"]
    assert _t(G.probe_view(s, region=(5, 3, 61, 44), size=(28, 20))) == (1, (3, 2, 31, 22), (28, 20), (28, 20))
    assert _t(G.probe_view(s, region=(5, 3, 61, 44), size=(29, 20))) == (0, (5, 3, 61, 44), (29, 20), (29, 20))
    assert _t(G.probe_view(s, region=(5, 3, 61, 44), size=(14, 10))) == (2, (2, 1, 16, 11), (14, 10), (14, 10))
    assert _t(G.probe_view(s, region=(5, 3, 61, 44), size=(3, 3)))[:2] == (2, (2, 1, 16, 11))   # 3 resolutions: no further
    # one resolution: nothing to discard, the kernel takes the whole 8 : 1
    assert _t(G.probe_view(streams["one"], size=(8, 6))) == (0, (0, 0, 64, 48), (8, 6), (8, 6))
    # six resolutions
    assert _t(G.probe_view(streams["deep"], size=(6, 3)))[:2] == (5, (0, 0, 7, 4))
    assert _t(G.probe_view(streams["deep"], size=(7, 4)))[:2] == (5, (0, 0, 7, 4))    # ceil(200 / 32) x ceil(120 / 32): a copy
    assert _t(G.probe_view(streams["deep"], size=(8, 4)))[:2] == (4, (0, 0, 13, 8))
    # an image origin: the canvas rectangle is what is reduced
    assert _t(G.probe_view(streams["origin"], size=(20, 15)))[:2] == (1, (3, 2, 23, 17))


def test_probe_swaps_for_quarter_turns(streams):
    for rot, mirror in ((0, False), (180, True)):
        assert _t(G.probe_view(streams["rgb"], size=(29, 17), rotate=rot, mirror=mirror))[2:] == ((29, 17), (29, 17))
    for rot, mirror in ((90, False), (270, True)):
        assert _t(G.probe_view(streams["rgb"], size=(29, 17), rotate=rot, mirror=mirror))[2:] == ((29, 17), (17, 29))


def test_probe_display_flags(streams):
    f = C.wrap(streams["420"], 34, 18, 3, 8, C.SYCC)
    r = G.probe_view(f, size=(8, 4), rgb=True, upsample=True)
    assert _t(r) == (0, (0, 0, 34, 18), (8, 4), (8, 4)) and r.channels == 3   # upsampling: no reduction
    g = O.encode(_img(34, 18, nc=1), 8, mct=False, numres=3)
    assert G.probe_view(g, size=(8, 4), force_rgb=True).channels == 3


def _refused(data, needle, **kw):
    with pytest.raises(ValueError) as e:
        G.probe_view(data, **kw)
    assert needle in str(e.value), str(e.value)


def _huge(cs, side):
    """The raw codestream with the image and its one tile `side` samples wide and high (header probes only)."""
    b = bytearray(cs)
    assert b[:4] == b"\xff\x4f\xff\x51"
    for off in (8, 12, 24, 28):   # Xsiz, Ysiz, XTsiz, YTsiz
        b[off:off + 4] = int(side).to_bytes(4, "big")
    return bytes(b)


def test_probe_refusals(streams):
    s = streams["rgb"]
    _refused(s, "rotate 45", size=(5, 5), rotate=45)
    _refused(s, "mirror must be 0 or 1", size=(5, 5), mirror=2)
    _refused(s, "fit must be 0 or 1", size=(5, 5), fit=2)
    _refused(s, "empty or leaves the image", region=(5, 5, 5, 9), size=(1, 1))
    _refused(s, "empty or leaves the image", region=(9, 5, 5, 9), size=(1, 1))
    _refused(s, "empty or leaves the image", region=(0, 0, 54, 37), size=(1, 1))
    _refused(s, "empty or leaves the image", region=(0, 0, 53, 38), size=(1, 1))
    _refused(s, "empty or leaves the image", region=(0, 0, 0, 5), size=(1, 1))
    _refused(s, "upscaling", size=(54, 37))
    _refused(s, "upscaling", size=(53, 38))
    _refused(s, "upscaling", width=54)
    _refused(s, "upscaling", region=(0, 0, 10, 10), size=(11, 5))
    _refused(s, "upscaling", size=(60, 60), fit=True)
    _refused(s, "both 0")
    _refused(s, "both 0", size=(0, 0), fit=True)
    # whatever the pixel calls refuse
    _refused(streams["420"], "GK_DISPLAY_UPSAMPLE", size=(8, 4))
    _refused(streams["c17"], "17 output channels", size=(3, 3))
    _refused(streams["rgb12"], "17", size=(3, 3), precision="8S,17S")
    _refused(s[:40], "", size=(3, 3))
    # the accumulator: 2^31 x 2^31 samples of 8 bits in a stream of one resolution
    _refused(_huge(streams["one"], 1 << 31), "overflows the 64-bit accumulator", size=(1, 1))
    assert G.probe_view(_huge(streams["one"], 1 << 26), size=(1, 1)).reduce == 0   # 2^52 << 8 fits
    with pytest.raises(ValueError):
        G.probe_view(s, size=(5, 5), width=5)
    with pytest.raises(ValueError):
        G.probe_view(s, size=(-1, 5))


# ---------------------------------------------------------------- 3. parse_iiif
def test_parse_iiif_regions():
    p = lambda *a: G.parse_iiif(100, 80, *a)
    assert p("full", "max", "0") == dict(region=None, width=100, height=80, fit=False, rotate=0, mirror=False)
    assert p("square", "max", "0")["region"] == (10, 0, 90, 80)
    assert G.parse_iiif(80, 101, "square")["region"] == (0, 10, 80, 90)
    assert p("10,20,30,40", "max", "0") == dict(region=(10, 20, 40, 60), width=30, height=40, fit=False, rotate=0, mirror=False)
    assert p("90,70,30,40", "max", "0")["region"] == (90, 70, 100, 80)           # cut at the image's edges
    assert p("0,0,100,80", "max", "0")["region"] is None
    assert p("pct:10,10,50,50", "max", "0")["region"] == (10, 8, 60, 48)
    assert p("pct:12.5,0,25,100", "max", "0")["region"] == (13, 0, 38, 80)       # 12.5 and 37.5 round half up
    for bad in ("100,0,5,5", "0,80,5,5", "0,0,0,5", "pct:100,0,5,5", "1,2,3", "a,b,c,d", "-1,0,5,5", "1.5,0,5,5", "sq", ""):
        with pytest.raises(ValueError):
            p(bad, "max", "0")


def test_parse_iiif_sizes():
    p = lambda size, region="full": G.parse_iiif(100, 80, region, size, "0")
    assert (p("50,")["width"], p("50,")["height"]) == (50, None)
    assert (p(",40")["width"], p(",40")["height"]) == (None, 40)
    assert (p("50,20")["width"], p("50,20")["height"], p("50,20")["fit"]) == (50, 20, False)
    assert (p("!50,50")["width"], p("!50,50")["height"], p("!50,50")["fit"]) == (50, 50, True)
    assert (p("!500,50")["width"], p("!500,50")["height"]) == (100, 50)          # held to the region
    assert (p("pct:50")["width"], p("pct:50")["height"]) == (50, 40)
    assert (p("pct:0.1")["width"], p("pct:0.1")["height"]) == (1, 1)
    assert (p("pct:100", "10,20,30,40")["width"], p("max", "10,20,30,40")["height"]) == (30, 40)
    for bad in ("^max", "^200,", "^!50,50", "101,", ",81", "100,81", "pct:101", "31,", "0,", ",0", "0,5", "x,", "5", "1,2,3", ""):
        with pytest.raises(ValueError):
            p(bad, "10,20,30,40" if bad == "31," else "full")


def test_parse_iiif_rotations():
    p = lambda rot: G.parse_iiif(100, 80, "full", "max", rot)
    assert [(p(r)["rotate"], p(r)["mirror"]) for r in ("0", "90", "180", "270", "!0", "!270", "90.0")] == \
        [(0, False), (90, False), (180, False), (270, False), (0, True), (270, True), (90, False)]
    for bad in ("45", "360", "-90", "!22.5", "x", "", "!"):
        with pytest.raises(ValueError):
            p(bad)


def test_parse_iiif_feeds_probe_view(streams):
    kw = G.parse_iiif(53, 37, "square", "!20,20", "!90")
    r = G.probe_view(streams["rgb"], **kw)
    assert ((r.out_w, r.out_h), (r.pix_w, r.pix_h), r.reduce) == ((20, 20), (20, 20), 0)
    r = G.probe_view(streams["rgb"], **G.parse_iiif(53, 37, "full", "pct:25", "270"))
    assert ((r.out_w, r.out_h), (r.pix_w, r.pix_h), r.reduce) == ((13, 9), (9, 13), 2)


# ---------------------------------------------------------------- 4. the ABI and the kernel
def test_abi_declared_exported_and_listed(tmp_path):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "grok_amd.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", G.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for sym in ("gk_probe_view", "gk_decode_view_pixels"):
        assert re.search(r"^int %s\s*\(" % sym, txt, flags=re.M), sym
        assert sym in exported and sym in G.EXPORTS
    src = tmp_path / "layout.c"
    src.write_text('#include "grok_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(gk_view), sizeof(gk_view_result),'
                   ' offsetof(gk_view, rotate), offsetof(gk_view_result, pix_w), offsetof(gk_view_result, sgnd));'
                   'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(G.View), ctypes.sizeof(G.ViewResult), G.View.rotate.offset, G.ViewResult.pix_w.offset,
                   G.ViewResult.sgnd.offset]


def test_kernel_builds_for_gfx950_without_scratch_or_lds(tmp_path):
    src = os.path.join(os.path.dirname(G.__file__), "csrc", "gk_view.hip")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "gk_view.out")],
                       capture_output=True, text=True, check=True)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == 3 and all("k_view" in n for n in names)   # u8, u16 and int32 pixels
    assert len(scratch) == 3 and not any(scratch) and len(lds) == 3 and not any(lds)
    assert "gk_view.hip" in open(os.path.join(os.path.dirname(G.__file__), "build.py")).read()
