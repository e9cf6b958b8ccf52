"""RGB to sYCC on encode, without a GPU: the arithmetic's restatement (tests/ycc_ref.py) against hand
computed answers and against the restated inverses of tests/display_ref.py, the no-device probe
(gk_probe_encode_convert) and the pipeline the GPU tests compare with (oracle encode of the restated
planes, OpenJPEG decode, display_ref back to RGB).

The round-trip bounds are a property of the defined forward arithmetic and of Grok's inverse
constants (three decimals in sycc_to_rgb), a restatement against a restatement: the kernel gets no
tolerance anywhere, it must equal ycc_ref bit for bit (tests/test_gpu_ycc_encode.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import grok_amd as G
import display_cases as C
import display_ref as D
import openjpeg as OPJ
import oracle as O
import ycc_ref as Y
from conftest import ROOT

# maximum |R' - R|, |G' - G|, |B' - B| of inverse(forward(rgb)): every 8-bit colour; at 12 and 16
# bits sample_colours() (measured with the two restatements alone)
ROUND_TRIP = {
    8: ((2, 2, 2), (1, 1, 1)),          # (sycc_to_rgb, color_esycc_to_rgb)
    12: ((2, 2, 2), (1, 2, 2)),
    16: ((2, 8, 3), (3, 20, 13)),
}


def test_known_answers_at_8_bits():
    for rgb, want, raw in [((255, 255, 255), (255, 128, 128), (128, 128)),
                           ((255, 0, 0), (76, 85, 255), (85, 256)),
                           ((0, 255, 0), (150, 44, 21), (44, 21)),
                           ((0, 0, 255), (29, 255, 107), (256, 107))]:
        got = Y.rgb_to_ycc(np.array(rgb).reshape(1, 1, 3), 8)
        assert tuple(int(p[0, 0]) for p in got) == want, rgb
        assert tuple(int(v) for v in Y.chroma(*rgb, 1, 8, clamp=False)) == raw, rgb   # (before the clamp)


@pytest.mark.parametrize("prec", [1, 8, 12, 16])
@pytest.mark.parametrize("sub", [Y.S444, Y.S422, Y.S420])
def test_grey_stays_grey(prec, sub):
    ramp = np.arange(1 << prec, dtype=np.int64)
    img = np.repeat(ramp.reshape(2, -1)[:, :, None], 3, axis=2)
    # (a box of different greys averages them; keep each box one grey)
    img = np.repeat(np.repeat(img, sub[1], axis=0), sub[0], axis=1)
    y, cb, cr = Y.rgb_to_ycc(img, prec, sub)
    assert (y == img[:, :, 0]).all()
    assert (cb == 1 << (prec - 1)).all() and (cr == 1 << (prec - 1)).all()


def sample_colours(prec, seed=7, n=1 << 20):
    """(1, N, 3): a fixed-seed sample of the colour cube plus its corners and edges."""
    rng = np.random.RandomState(seed)
    top = (1 << prec) - 1
    pts = [rng.randint(0, top + 1, (n, 3))]
    ramp = np.arange(top + 1)
    for a in (0, top):
        for b in (0, top):
            for ax in range(3):
                e = np.empty((top + 1, 3), np.int64)
                o = [k for k in range(3) if k != ax]
                e[:, ax], e[:, o[0]], e[:, o[1]] = ramp, a, b
                pts.append(e)
    return np.concatenate(pts)[None, :, :]


def round_trip_errors(rgb, prec):
    y, cb, cr = Y.rgb_to_ycc(rgb, prec)
    back = D.sycc_to_rgb(1 << (prec - 1), (1 << prec) - 1, y, cb, cr)
    eback = D.color_esycc_to_rgb([y, cb, cr], [(1, 1, prec, 0)] * 3)
    err = lambda out: tuple(int(np.abs(out[k].astype(np.int64) - rgb[:, :, k]).max()) for k in range(3))
    return err(back), err(eback)


def test_round_trip_of_every_8_bit_colour():
    g = np.arange(256)
    rgb = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(1, -1, 3)
    sycc, esycc = round_trip_errors(rgb, 8)
    print("8 bits: sYCC", sycc, "e-sYCC", esycc)
    assert max(sycc) <= 2 and max(esycc) <= 1
    assert (sycc, esycc) == ROUND_TRIP[8]


@pytest.mark.parametrize("prec", [12, 16])
def test_round_trip_at_12_and_16_bits(prec):
    sycc, esycc = round_trip_errors(sample_colours(prec), prec)
    print("%d bits: sYCC" % prec, sycc, "e-sYCC", esycc)
    assert (sycc, esycc) == ROUND_TRIP[prec]


# ---------------------------------------------------------------- the probe
@pytest.mark.parametrize("origin", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("size", [(1, 1), (2, 2), (3, 5), (17, 9)])
@pytest.mark.parametrize("sub", [Y.S444, Y.S422, Y.S420])
def test_probe_shapes(origin, size, sub):
    w, h = size
    grids, shapes = G.probe_encode_convert((h, w, 3), 8, "sycc", sub, origin=origin)
    assert grids == Y.subsampling(sub)
    assert shapes == [G.comp_shape(w, h, dx, dy, origin) for dx, dy in grids]
    assert shapes[1] == Y.chroma_shape(w, h, sub, origin) == shapes[2]
    assert [p.shape for p in Y.rgb_to_ycc(np.zeros((h, w, 3), np.int64), 8, sub, origin)] == shapes


def test_probe_esycc_is_444():
    grids, shapes = G.probe_encode_convert((9, 17, 3), 12, "esycc", (1, 1), origin=(1, 1), sample_bytes=2)
    assert grids == [(1, 1)] * 3 and shapes == [(9, 17)] * 3


@pytest.mark.parametrize("kw,name", [
    (dict(shape=(4, 4, 4)), "4 channels"),
    (dict(shape=(4, 4, 1)), "1 channels"),
    (dict(signed=True), "signed"),
    (dict(prec=17), "precision 17"),
    (dict(prec=0), "precision 0"),
    (dict(chroma=(1, 2)), "chroma subsampling 1 x 2"),
    (dict(chroma=(4, 1)), "chroma subsampling 4 x 1"),
    (dict(chroma=(2, 4)), "chroma subsampling 2 x 4"),
    (dict(chroma=(0, 0)), "chroma subsampling 0 x 0"),
    (dict(space="esycc", chroma=(2, 1)), "e-sYCC with subsampled chroma"),
    (dict(space="esycc", chroma=(2, 2)), "e-sYCC with subsampled chroma"),
    (dict(space="srgb"), "colour space 2"),
    (dict(space=0), "colour space 0"),
    (dict(prec=12, sample_bytes=1), "sample_bytes"),
    (dict(shape=(0, 4, 3)), "empty image"),
])
def test_probe_refusals_name_the_cause(kw, name):
    args = dict(shape=(4, 4, 3), prec=8, space="sycc", chroma=(2, 2))
    args.update(kw)
    with pytest.raises(ValueError, match=re.escape(name)):
        G.probe_encode_convert(**args)


def test_entry_points_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "grok_amd.h")).read()
    lib = G.load_library()
    for name in ("gk_set_encode_convert", "gk_probe_encode_convert"):
        assert name in G.EXPORTS and hasattr(lib, name)
        assert re.search(r"\bint %s\(" % name, header)
    assert hasattr(G.Engine, "set_encode_convert")


def test_kernel_builds_for_gfx950_without_scratch_or_lds(tmp_path):
    src = os.path.join(os.path.dirname(G.__file__), "csrc", "gk_rgbycc.hip")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "gk_rgbycc.out")],
                       capture_output=True, text=True, check=True)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    # 3 sample sizes x 3 layouts x (packed, planar)
    assert len(names) == 18 and all("k_rgb_ycc" in n for n in names)
    assert len(scratch) == 18 and not any(scratch) and len(lds) == 18 and not any(lds)


# ---------------------------------------------------------------- the pipeline the GPU tests compare with
def test_oracle_and_openjpeg_carry_the_restated_planes():
    if not OPJ.available():
        pytest.skip("libopenjp2 not found")
    w, h, prec = 33, 21, 8
    src = Y.box_constant(np.random.RandomState(3), w, h, prec, Y.S420)
    planes = Y.rgb_to_ycc(src, prec, Y.S420)
    sub = Y.subsampling(Y.S420)
    cs = O.encode(planes, prec, size=(w, h), subsampling=sub, mct=False, numres=C.numres_for(w, h, sub))
    dec = OPJ.decode(cs)
    assert [(dx, dy) for dx, dy, _ in dec] == sub
    for (_, _, got), want in zip(dec, planes):
        np.testing.assert_array_equal(got, want)
    comps = [(dx, dy, prec, 0) for dx, dy in sub]
    rgb, _ = D.color_sycc_to_rgb([p for _, _, p in dec], comps, 0, 0)
    for k in range(3):
        err = int(np.abs(rgb[k].astype(np.int64) - src[:, :, k]).max())
        print("channel", k, "max error", err)
        assert err <= ROUND_TRIP[8][0][k]
