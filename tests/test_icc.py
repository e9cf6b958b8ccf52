"""Colour management without a GPU: the float64 restatement (tests/icc_ref.py) against lcms2 called
as Grok's CLI calls it, the header probes under GK_DISPLAY_ICC, and the profile reader under
AddressSanitizer / UBSan in a stand-alone program (tools/icc_check.cpp).

Figures of the lcms2 comparison on this case list (lcms2 2.18, Pillow's wheel): the largest
difference is 1 level for every profile at 8 bits (flags 0), at 16 bits with cmsFLAGS_NOOPTIMIZE and
for CIELab; with flags 0 at 16 bits lcms2 is between 3,700 and 8,600 of 65,535 away (R-BUG-12).
A `curv` table is read as lcms2 reads it (16-bit fixed-point interpolation): with exact linear
interpolation the restatement was up to 17 of 65,535 from lcms2 unoptimised."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import grok_amd as G
import icc_profiles as P
import icc_ref as R
import jp2_boxes as J
import lcms
import oracle as O
from conftest import ROOT

needs_lcms = pytest.mark.skipif(not lcms.available(), reason="needs lcms2 (Pillow's pillow.libs)")
LIB = os.path.join(ROOT, "grok_amd", "libgrok_amd.so")
ACCEPTED = sorted(P.accepted())
RGB_PROFILES = [n for n in ACCEPTED if not P.accepted()[n][1]]
GREY_PROFILES = [n for n in ACCEPTED if P.accepted()[n][1]]


def lattice(bits, n=17):
    v = np.round(np.linspace(0, (1 << bits) - 1, n)).astype(np.int64)
    return np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=-1).reshape(-1, 3)


def triples(bits, seed):
    return np.concatenate([lattice(bits), np.random.RandomState(seed).randint(0, 1 << bits, (1 << 16, 3))])


# ---------------------------------------------------------------- 1. the restatement against lcms2
@needs_lcms
@pytest.mark.parametrize("name", RGB_PROFILES)
def test_ref_matches_lcms_rgb8(name):
    prof = P.accepted()[name][0]
    s = triples(8, 1)
    got = lcms.apply_profile(prof, s, 8).astype(np.int64)
    _, want = R.apply_profile(prof, s, 8)
    d = int(np.abs(got - want).max())
    print(name, "max difference", d, "differing", float(np.mean(got != want)))
    assert d <= 1


@needs_lcms
@pytest.mark.parametrize("name", GREY_PROFILES)
def test_ref_matches_lcms_grey8(name):
    prof = P.accepted()[name][0]
    v = np.arange(256)
    got = lcms.apply_profile(prof, v, 8).astype(np.int64)
    _, want = R.apply_profile(prof, v, 8)
    assert (got[:, 0] == got[:, 1]).all() and (got[:, 0] == got[:, 2]).all()
    assert int(np.abs(got[:, 0] - want).max()) <= 1


def lab_samples(seed):
    rng = np.random.RandomState(seed)
    rnd = np.stack([rng.uniform(0, 100, 1 << 16), rng.uniform(-128, 128, 1 << 16), rng.uniform(-128, 128, 1 << 16)], axis=-1)
    lat = lattice(8).astype(np.float64) / 255.0 * np.array([100.0, 255.0, 255.0]) - np.array([0.0, 127.5, 127.5])
    return np.concatenate([lat, rnd])


@needs_lcms
def test_ref_matches_lcms_lab():
    lab = lab_samples(3)
    got = lcms.lab_to_rgb16(lab).astype(np.int64)
    _, want = R.lab_to_rgb(lab)
    assert int(np.abs(got - want).max()) <= 1
    # the integer samples of both boxes, through Grok's ranges and offsets
    rng = np.random.RandomState(4)
    for bits, custom in ((8, None), (16, (100, 0, 180, 1 << 15, 180, 1 << 15, P.CIE_D50))):
        s = rng.randint(0, 1 << bits, (1 << 14, 3))
        vals = R.lab_values(s, bits, P.lab_words(custom))
        _, want = R.lab_to_rgb(vals)
        assert int(np.abs(lcms.lab_to_rgb16(vals).astype(np.int64) - want).max()) <= 1


# ---------------------------------------------------------------- 2. 16 bits: unoptimised lcms2, and R-BUG-12
@needs_lcms
@pytest.mark.parametrize("name", RGB_PROFILES)
def test_ref_matches_unoptimised_lcms_rgb16(name):
    prof = P.accepted()[name][0]
    s = triples(16, 2)
    got = lcms.apply_profile(prof, s, 16, lcms.FLAGS_NOOPTIMIZE).astype(np.int64)
    _, want = R.apply_profile(prof, s, 16)
    assert int(np.abs(got - want).max()) <= 1


@needs_lcms
def test_optimised_lcms_is_off_at_16_bits():
    """R-BUG-12: with flags 0, which is how Grok calls it, lcms2 resamples the transform into a 3-D
    table; on the input where the unoptimised transform agrees with the restatement it does not."""
    prof = P.accepted()["adobe_g22"][0]
    s = triples(16, 2)
    _, want = R.apply_profile(prof, s, 16)
    assert int(np.abs(lcms.apply_profile(prof, s, 16, lcms.FLAGS_NOOPTIMIZE).astype(np.int64) - want).max()) <= 1
    d = int(np.abs(lcms.apply_profile(prof, s, 16, 0).astype(np.int64) - want).max())
    print("flags 0 at 16 bits: max difference", d)
    assert d > 1


# ---------------------------------------------------------------- 3. the illuminant word
@needs_lcms
def test_lab_illuminant_has_no_effect():
    lab = lab_samples(5)
    d50 = lcms.lab_to_rgb16(lab)
    np.testing.assert_array_equal(lcms.lab_to_rgb16(lab, 6504), d50)     # GRK_CIE_D65
    np.testing.assert_array_equal(lcms.lab_to_rgb16(lab, 2856), d50)     # GRK_CIE_SA: cmsWhitePointFromTemp fails


# ---------------------------------------------------------------- 4. header probes
def image(nc, prec, seed=0, h=16, w=16, signed=False):
    rng = np.random.RandomState(seed)
    lo = -(1 << (prec - 1)) if signed else 0
    return rng.randint(lo, lo + (1 << prec), (nc, h, w)).astype(np.int32)


def stream(nc, prec, signed=False, **kw):
    return O.encode(image(nc, prec, signed=signed), prec, signed=signed, mct=False, numres=2, **kw)


def rgb_file(profile, nc=3, prec=8, cdef=None, extra=(), signed=False):
    return P.jp2(stream(nc, prec, signed), 16, 16, nc, prec, P.colr_profile(profile), cdef, extra, signed)


ADOBE = P.accepted()["adobe_g22"][0]
GREY = P.accepted()["grey_g22"][0]
CUSTOM = (100, 0, 180, 1 << 15, 180, 1 << 15, P.CIE_D65)


def describe(d):
    return (len(d.precisions), d.precisions, d.colour_space, d.colour.display_applied)


def test_probe_describes_every_accepted_case():
    for name in ACCEPTED:
        prof, grey = P.accepted()[name]
        d = G.probe_output(rgb_file(prof, 1 if grey else 3), icc=True)
        assert describe(d) == ((1, [8], 3, 8) if grey else (3, [8] * 3, 2, 8)), name
    for prec in (1, 5, 12, 16):
        assert describe(G.probe_output(rgb_file(ADOBE, prec=prec), icc=True)) == (3, [prec] * 3, 2, 8)
    rgba = rgb_file(ADOBE, 4, cdef=P.RGBA_CDEF)
    for force in (False, True):
        d = G.probe_output(rgba, icc=True, force_rgb=force)
        assert describe(d) == (4, [8] * 4, 2, 8)
        assert list(d.colour.typ[:4]) == [0, 0, 0, 1] and d.managed and not d.replicated
        assert describe(G.probe_output(rgb_file(ADOBE), icc=True, force_rgb=force)) == (3, [8] * 3, 2, 8)
    grey, greya = rgb_file(GREY, 1), rgb_file(GREY, 2, cdef=P.GREYA_CDEF)
    assert describe(G.probe_output(grey, icc=True)) == (1, [8], 3, 8)
    assert describe(G.probe_output(grey, icc=True, force_rgb=True)) == (3, [8] * 3, 2, 12)
    assert describe(G.probe_output(greya, icc=True)) == (2, [8, 8], 3, 8)
    d = G.probe_output(greya, icc=True, force_rgb=True)
    assert describe(d) == (4, [8] * 4, 2, 12) and list(d.colour.typ[:4]) == [0, 0, 0, 1]
    # the flag off: the profile is only reported
    d = G.probe_output(rgb_file(ADOBE))
    assert describe(d) == (3, [8] * 3, 9, 0) and G.probe_icc(rgb_file(ADOBE)) == ADOBE
    # a forced precision follows the conversion
    assert describe(G.probe_output(rgb_file(ADOBE, prec=12), icc=True, precision="8S")) == (3, [8] * 3, 2, 8)


def lab_file(prec, custom=None, nc=3, cdef=None, **kw):
    return P.jp2(stream(nc, prec, **kw), 16, 16, nc, prec, P.colr_lab(custom), cdef)


def test_probe_describes_cielab():
    for prec, custom, space in ((8, None, 7), (16, CUSTOM, 8), (12, None, 7)):
        f = lab_file(prec, custom)
        assert G.probe_colour(f).colour_space == space and G.probe_colour(f).enumcs == 14
        assert G.probe_cielab(f) == P.lab_words(custom)
        assert describe(G.probe_output(f)) == (3, [prec] * 3, space, 0)       # decodes to its L*, a*, b* planes
        assert describe(G.probe_output(f, icc=True)) == (3, [16] * 3, 2, 8)
        assert G.probe_output(f, icc=True).info.prec == 16
    # a colr box of another size is the default space (Grok's warning path)
    odd = struct.pack(">I4s", 8 + 11, b"colr") + struct.pack(">BBBI", 1, 0, 0, 14) + b"\0" * 4
    f = P.jp2(stream(3, 8), 16, 16, 3, 8, odd)
    assert G.probe_cielab(f) == [14, P.GRK_DEFAULT_CIELAB_SPACE] and G.probe_colour(f).colour_space == 7
    # L*a*b* + opacity: the fourth channel keeps its precision
    assert describe(G.probe_output(lab_file(8, None, 4, P.RGBA_CDEF), icc=True)) == (4, [16, 16, 16, 8], 2, 8)
    assert G.probe_cielab(rgb_file(ADOBE)) == []
    with pytest.raises(ValueError, match="CIELab"):   # without the flag grey to RGB still refuses the space
        G.probe_output(lab_file(8), force_rgb=True)


def test_probe_leaves_other_files_alone():
    cs = stream(3, 8)
    srgb = P.jp2(cs, 16, 16, 3, 8, J.colr_enum(16))
    for f in (srgb, cs, P.jp2(stream(1, 8), 16, 16, 1, 8, J.colr_enum(17))):
        a, b = G.probe_output(f), G.probe_output(f, icc=True)
        assert describe(a) == describe(b) and b.colour.display_applied == 0
        assert bytes(a.colour) == bytes(b.colour) and bytes(a.info) == bytes(b.info)


def patch_siz(f, comp, ssiz=None, xrsiz=None):
    """The file with one component's Ssiz / XRsiz rewritten in the SIZ marker."""
    b = bytearray(f)
    at = b.index(b"\xff\x4f\xff\x51") + 4 + 2 + 2 + 32 + 2 + 3 * comp
    if ssiz is not None:
        b[at] = ssiz
    if xrsiz is not None:
        b[at + 1] = xrsiz
    return bytes(b)


def test_probe_leaves_unlike_channels_unconverted():
    """color.cpp:469-485: the first min(nc, 4) channels of an RGB-profile image must be alike."""
    for f in (patch_siz(rgb_file(ADOBE), 1, ssiz=6), patch_siz(rgb_file(ADOBE), 2, xrsiz=2),
              patch_siz(rgb_file(ADOBE, 4, cdef=P.RGBA_CDEF), 3, ssiz=3), patch_siz(rgb_file(ADOBE), 1, ssiz=0x87)):
        d = G.probe_output(f, icc=True)
        assert d.colour_space == 9 and d.colour.display_applied == 0
        assert describe(d)[:2] == describe(G.probe_output(f))[:2]


@pytest.mark.parametrize("name", sorted(P.refused()))
def test_probe_refuses_profile(name):
    prof, words = P.refused()[name]
    f = rgb_file(prof, 1 if name.startswith("grey") else 3)
    with pytest.raises(ValueError, match="display: ICC: .*" + words):
        G.probe_output(f, icc=True)
    assert G.probe_output(f).colour_space == 9        # without the flag it decodes as before


def test_probe_refuses_images():
    pal = [J.pclr(np.arange(256 * 3).reshape(256, 3) % 256, [8, 8, 8]), J.cmap([(0, 1, 0), (0, 1, 1), (0, 1, 2)])]
    sub = O.encode([image(1, 8)[0], image(1, 8, h=16, w=8)[0], image(1, 8, h=16, w=8)[0]], 8, size=(16, 16), mct=False, numres=2,
                   subsampling=[(1, 1), (2, 1), (2, 1)])
    sub1 = O.encode([image(1, 8, h=16, w=8)[0]], 8, size=(16, 16), mct=False, numres=2, subsampling=[(2, 1)])
    cases = [
        (rgb_file(ADOBE, signed=True), "signed"),
        (lab_file(8, signed=True), "signed"),
        (rgb_file(GREY, 1, signed=True), "signed"),
        (patch_siz(patch_siz(patch_siz(rgb_file(ADOBE, prec=16), 0, ssiz=16), 1, ssiz=16), 2, ssiz=16), "17 bits"),
        (rgb_file(ADOBE, 2), "RGB profile on an image of 2 channels"),
        (rgb_file(ADOBE, 1), "RGB profile on an image of 1 channels"),
        (rgb_file(GREY, 3), "grey profile on an image of 3 channels"),
        (lab_file(8, nc=2), "CIELab: an image of 2 channels"),
        (P.jp2(sub1, 16, 16, 1, 8, P.colr_profile(GREY)), "subsampled"),
        (P.jp2(patch_siz(patch_siz(patch_siz(stream(3, 8), 0, xrsiz=2), 1, xrsiz=2), 2, xrsiz=2), 16, 16, 3, 8, P.colr_profile(ADOBE)),
         "subsampled"),
        (P.jp2(sub, 16, 16, 3, 8, P.colr_lab()), "subsampled"),
        (rgb_file(ADOBE, 1, extra=pal), "palette"),
    ]
    for f, words in cases:
        with pytest.raises(ValueError, match="display: .*" + words):
            G.probe_output(f, icc=True)
        G.probe_output(f)
    with pytest.raises(ValueError, match="subsampled"):     # ... also when the CLI's rule takes the image as sYCC first
        G.probe_output(P.jp2(sub, 16, 16, 3, 8, P.colr_lab()), icc=True, rgb=True)


# ---------------------------------------------------------------- 5. the reader under the sanitizers
def _host_compiler():
    for c in ("g++", "clang++", "hipcc"):
        if shutil.which(c):
            return c
    return None


@pytest.mark.skipif(_host_compiler() is None, reason="needs a C++ compiler")
def test_reader_under_sanitizers(tmp_path):
    exe = str(tmp_path / "icc_check")
    subprocess.check_call([_host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "icc_check.cpp"), "-o", exe])
    files, want = [], {}
    for name in ACCEPTED:
        files.append(str(tmp_path / name)); want[files[-1]] = None
        open(files[-1], "wb").write(P.accepted()[name][0])
    for name, (prof, words) in P.refused().items():
        files.append(str(tmp_path / ("bad_" + name))); want[files[-1]] = words
        open(files[-1], "wb").write(prof)
    good = P.accepted()["adobe_three_curves"][0]
    for n in (0, 1, 127, 128, 131, 132, 140, 200, len(good) - 1):       # every truncation is a refusal, not a read past the end
        files.append(str(tmp_path / ("cut_%d" % n))); want[files[-1]] = "not a profile"
        open(files[-1], "wb").write(good[:n])
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(l.split(": ", 1) for l in r.stdout.splitlines())
    assert len(lines) == len(files)
    for f, words in want.items():
        if words is None:
            assert lines[f].startswith("ok: "), lines[f]
        else:
            assert lines[f].startswith("refused: ") and words in lines[f], lines[f]
    assert "curve0 para(g=2.199219" in lines[str(tmp_path / "adobe_g22")]
    assert "curve1 table(1024)" in lines[str(tmp_path / "adobe_three_curves")]
    assert "grey" in lines[str(tmp_path / "grey_g22")]
