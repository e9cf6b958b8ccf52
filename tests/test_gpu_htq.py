"""HT 9/7 quantisation control on the GPU: Engine.set_encode_quant(step | max_bytes | psnr).

References: the oracle's encoder at the default step (byte identity), tests/htq_ref.py for the QCD
of any step and for the known answer of a numres = 1 encode, the oracle's decoder (and OpenJPEG's)
for what the streams mean.  Shapes are the smallest at which the kernels can go wrong: one sample,
an image below one quad row, odd sizes, ICT, ragged edge tiles, 16-bit and signed samples, 1 / 3 / 6
resolutions.
"""
import ctypes
import math

import numpy as np
import pytest

import htq_ref as R
import openjpeg
import oracle as O
from test_gpu_ht97 import _img, _psnr

pytestmark = pytest.mark.gpu

# PSNR mode: the achieved PSNR (oracle decode against the source) may fall below the target by at
# most this much.  It is the largest measured est_psnr - achieved of the PSNR cases below plus
# 0.1 dB for platform float differences; per case (dB; negative: the estimate was pessimistic):
#   line    30 / 36 / 42:  0.061 -0.036 -0.114      rgb     30 / 36 / 42:  0.157 -0.698 -0.565
#   tiles   30 / 36 / 42: -0.503 -0.697 -0.512      tiles1  30 / 36 / 42:  0.044 -0.027 -0.103
#   mono12  40 / 50:      -0.156 -0.117             s12     40 / 50:       0.003 -0.002
#   one     30 / 36 / 42:  2.341 (notch 43 each time; achieved 42.11 dB, above every target)
# The largest is 0.157 dB wherever the image has more than one sample.  The one-sample image is
# the exception and no bias of the estimate: its estimate is pinned to err^2 + 1/12 by
# test_distortion_estimate, 1/12 being the mean of a rounding error whose single realisation here
# is (1.5 + 0.5)^2 - 1.5^2; it is asserted like the others and is not what the bar is taken from.
# This departs from the issue in one point, on the stricter side: the issue takes the bar from the
# largest shortfall of exactly these cases (2.341 + 0.1) and calls an estimator with more than 1 dB
# wrong; here the bar is 0.257 dB for every case, the 1 x 1 image included.
PSNR_MARGIN = 0.157 + 0.1

CASES = {
    "one": dict(seed=11, c=1, h=1, w=1, bits=8, numres=1),
    "line": dict(seed=12, c=1, h=3, w=5, bits=8, numres=1),
    "mono12": dict(seed=13, c=1, h=129, w=67, bits=12, numres=3),
    "rgb": dict(seed=14, c=3, h=88, w=72, bits=8, numres=6),
    "tiles": dict(seed=15, c=3, h=170, w=150, bits=8, numres=3, tiles=(64, 64)),
    "tiles1": dict(seed=16, c=3, h=170, w=150, bits=8, numres=1, tiles=(64, 64), mct=False),
    "mono16": dict(seed=17, c=1, h=160, w=96, bits=16, numres=6),
    "s12": dict(seed=18, c=1, h=77, w=90, bits=12, numres=1, signed=True),
}
FLAT = ("one", "line", "tiles1", "s12")   # numres = 1 without MCT: coefficient = sample - dc


@pytest.fixture(scope="module")
def eng():
    import grok_amd as G
    e = G.Engine(0)
    yield e
    e.set_encode_quant()
    e.close()


_memo = {}


def _case(name):
    """(image, engine params kwargs, oracle kwargs, bits, signed), the image built once."""
    if name not in _memo:
        k = CASES[name]
        sg = k.get("signed", False)
        img = _img(k["seed"], k["c"], k["h"], k["w"], k["bits"], sg)
        kw = dict(numresolution=k["numres"], cblk_sty=0x40, irreversible=True, mct=k.get("mct", True))
        okw = dict(numres=k["numres"], cblk_sty=0x40, irreversible=True, mct=k.get("mct", True))
        if "tiles" in k:
            kw["tiles"] = okw["tiles"] = k["tiles"]
        img.setflags(write=False)
        _memo[name] = (img, kw, okw, k["bits"], sg)
    return _memo[name]


def _encode(eng, name, **extra):
    import grok_amd as G
    img, kw, _, bits, sg = _case(name)
    return eng.encode(img, bits, signed=sg, params=G.default_params(**dict(kw, **extra)))


def _steps(bits, sg):
    """The STEP values of check 2: notches 8 and 24 and one value between two notches."""
    return [R.ladder_step(bits, sg, 8), R.ladder_step(bits, sg, 24), R.ladder_step(bits, sg, 13) * 1.03]


@pytest.mark.parametrize("name", list(CASES))
def test_step_default_is_todays_stream(eng, name):
    img, kw, okw, bits, sg = _case(name)
    eng.set_encode_quant()
    plain = _encode(eng, name)
    eng.set_encode_quant(step=R.ladder_step(bits, sg, 0))
    cs = _encode(eng, name)
    r = eng.encode_quant()
    eng.set_encode_quant()
    assert cs == plain == O.encode(img, bits, signed=sg, **okw)
    assert (r["mode"], r["notch"], r["t1_passes"], r["bytes"]) == (1, 0, 1, len(cs))


@pytest.mark.parametrize("name", list(CASES))
def test_step_streams(eng, name):
    img, kw, okw, bits, sg = _case(name)
    lens, psnrs = [], []
    for i, step in enumerate([R.ladder_step(bits, sg, 0)] + _steps(bits, sg)):
        eng.set_encode_quant(step=step)
        cs = _encode(eng, name)
        r = eng.encode_quant()
        eng.set_encode_quant()
        assert r["base_step"] == pytest.approx(step, rel=1e-12) and r["t1_passes"] == 1
        assert R.find_qcd(cs) == R.qcd_body(step, kw["numresolution"])
        ref = O.decode(cs)[0]
        np.testing.assert_array_equal(eng.decode(cs), ref)
        if name in FLAT:
            e, m = R.band_quant(step, 1)[0]
            np.testing.assert_array_equal(ref, R.known_answer(img, bits, sg, R.band_step(e, m, bits)))
        if i < 3:   # notches 0, 8, 24
            lens.append(len(cs))
            psnrs.append(_psnr(ref, img, bits))
    print(name, "lengths", lens, "psnr", ["%.2f" % p for p in psnrs])
    assert lens[0] >= lens[1] >= lens[2]
    assert psnrs[0] >= psnrs[1] >= psnrs[2]


@pytest.mark.parametrize("name,jp2", [("mono12", False), ("rgb", False), ("rgb", True), ("tiles", False), ("mono16", False),
                                      ("s12", False)])
def test_bytes_target(eng, name, jp2):
    img, kw, okw, bits, sg = _case(name)
    extra = dict(jp2=True) if jp2 else {}
    eng.set_encode_quant(step=R.ladder_step(bits, sg, 0))
    full = len(_encode(eng, name, **extra))
    launches = eng.timings().dwt_launches
    notches = R.notches(bits)
    for frac in (2, 4):
        target = full // frac
        eng.set_encode_quant(max_bytes=target)
        cs = _encode(eng, name, **extra)
        r = eng.encode_quant()
        assert eng.timings().dwt_launches == launches
        print(name, "target", target, "got", len(cs), "notch", r["notch"], "passes", r["t1_passes"])
        assert len(cs) <= target and r["bytes"] == len(cs) and r["mode"] == 2
        assert r["t1_passes"] <= 2 + math.ceil(math.log2(notches))
        assert r["base_step"] == R.ladder_step(bits, sg, r["notch"])
        if not jp2:
            np.testing.assert_array_equal(eng.decode(cs), O.decode(cs)[0])
        if r["notch"] > 0:
            eng.set_encode_quant(step=R.ladder_step(bits, sg, r["notch"] - 1))
            assert len(_encode(eng, name, **extra)) > target
        # the same call again, after other work on the engine: the same bytes
        eng.set_encode_quant(max_bytes=target)
        assert _encode(eng, name, **extra) == cs
    eng.set_encode_quant()


def test_bytes_target_below_the_ladder(eng):
    for name, target in (("one", 40), ("rgb", 300)):
        eng.set_encode_quant(max_bytes=target)
        with pytest.raises(RuntimeError, match="quant: max_bytes %d is below what the coarsest notch" % target):
            _encode(eng, name)
    eng.set_encode_quant()
    img, kw, okw, bits, sg = _case("rgb")
    assert _encode(eng, "rgb") == O.encode(img, bits, **okw)


@pytest.mark.parametrize("name", FLAT)
def test_distortion_estimate(eng, name):
    """k_htq_dist against numpy where the coefficients are known without a DWT: est_mse is the
    float64 sum of htq_ref's squared errors over the samples, plus 1/12.  The bound of 1e-5 covers
    float32 partial sums
    over at most 25,500 samples; measured: 0 in all twelve cases (the coefficients are integers and the
    steps short dyadic fractions, so the float32 sums are exact), hence the tighter 1e-6 asserted."""
    img, kw, okw, bits, sg = _case(name)
    x = img.astype(np.int64) - (0 if sg else 1 << (bits - 1))
    for n in (0, 8, 24):
        step = R.ladder_step(bits, sg, n)
        eng.set_encode_quant(step=step)
        _encode(eng, name)
        r = eng.encode_quant()
        e, m = R.band_quant(step, 1)[0]
        want = R.band_error(x, R.band_step(e, m, bits)) / x.size + 1.0 / 12.0
        print(name, n, "est_mse", r["est_mse"], "numpy", want, "rel", abs(r["est_mse"] - want) / want)
        assert r["stats_passes"] == 1
        assert r["est_mse"] == pytest.approx(want, rel=1e-6)
        assert r["est_psnr"] == pytest.approx(10 * math.log10(((1 << bits) - 1) ** 2 / want), abs=1e-4)
    eng.set_encode_quant()


PSNR_CASES = [(n, t) for n in ("one", "line", "rgb", "tiles", "tiles1") for t in (30, 36, 42)] + \
             [(n, t) for n in ("mono12", "s12") for t in (40, 50)]


@pytest.mark.parametrize("name,target", PSNR_CASES)
def test_psnr_target(eng, name, target):
    img, kw, okw, bits, sg = _case(name)
    eng.set_encode_quant(psnr=target)
    cs = _encode(eng, name)
    r = eng.encode_quant()
    eng.set_encode_quant()
    got = _psnr(O.decode(cs)[0], img, bits)
    print(name, target, "notch", r["notch"], "est %.3f next %.3f achieved %.3f shortfall %.3f" %
          (r["est_psnr"], r["est_psnr_next"], got, r["est_psnr"] - got))
    assert (r["mode"], r["t1_passes"], r["stats_passes"]) == (3, 1, 1)
    assert r["est_psnr_next"] < target <= r["est_psnr"]
    assert R.find_qcd(cs) == R.qcd_body(R.ladder_step(bits, sg, r["notch"]), kw["numresolution"])
    assert got >= target - PSNR_MARGIN


def test_history(eng):
    """STEP, BYTES, PSNR, STEP on one engine: a result does not depend on the calls before it."""
    img, kw, okw, bits, sg = _case("rgb")
    step = R.ladder_step(bits, sg, 11)
    eng.set_encode_quant(step=step)
    first = _encode(eng, "rgb")
    eng.set_encode_quant(max_bytes=len(first) // 3)
    b = _encode(eng, "rgb")
    eng.decode(O.encode(img, bits, **okw))   # a decode applies its stream's QCD to the cached plan
    eng.set_encode_quant(psnr=33)
    c = _encode(eng, "rgb")
    eng.set_encode_quant(step=step)
    assert _encode(eng, "rgb") == first
    eng.set_encode_quant(max_bytes=len(first) // 3)
    assert _encode(eng, "rgb") == b
    eng.set_encode_quant(psnr=33)
    assert _encode(eng, "rgb") == c
    eng.set_encode_quant()
    assert _encode(eng, "rgb") == O.encode(img, bits, **okw)
    assert eng.encode_quant()["mode"] == 0


def test_refusals_on_the_engine(eng):
    import grok_amd as G
    img, kw, okw, bits, sg = _case("tiles")
    eng.set_encode_quant(step=R.ladder_step(bits, sg, 8))
    try:
        with pytest.raises(RuntimeError, match="quant: .*Part-1"):
            eng.encode(img, bits, params=G.default_params(irreversible=True))
        with pytest.raises(RuntimeError, match="quant: .*reversible"):
            eng.encode(img, bits, params=G.default_params(cblk_sty=0x40))
        with pytest.raises(RuntimeError, match="quant: numlayers"):
            _encode(eng, "tiles", numlayers=2)
        with pytest.raises(RuntimeError, match="quant: layer_rate"):
            _encode(eng, "tiles", layer_rate=[20])
        one = np.ascontiguousarray(img[:, :64, :64])   # (gk_encode_blocks takes single-tile images)
        info = G.ImageInfo(64, 64, 3, bits, 0, 0)
        ptrs = (ctypes.c_void_p * 3)(*[one[k].ctypes.data for k in range(3)])
        pb = G.default_params(numresolution=3, cblk_sty=0x40, irreversible=True)
        rc = eng.lib.gk_encode_blocks(ctypes.c_void_p(eng.ctx), ctypes.byref(info), ptrs, (ctypes.c_uint32 * 3)(64, 64, 64), 0,
                                      ctypes.byref(pb), None, None, None, None)
        assert rc == -1 and "quant: gk_encode_blocks while gk_set_encode_quant is set" in eng.lib.gk_last_error(eng.ctx).decode()
        # STEP mode shards: header + tile parts + EOC is the whole-image stream
        p = G.default_params(**kw)
        whole = eng.encode(img, bits, params=p)
        hdr = eng.main_header(img.shape, bits, params=p)[0]
        parts = eng.encode_tiles(img, bits, 0, 9, params=p)[0]
        assert hdr + parts + b"\xff\xd9" == whole
        eng.set_encode_quant(psnr=40)
        with pytest.raises(RuntimeError, match="quant: GK_QUANT_BYTES / GK_QUANT_PSNR with gk_encode_tiles"):
            eng.encode_tiles(img, bits, 0, 9, params=p)
        with pytest.raises(ValueError, match="quant: unknown mode|finite and positive"):
            eng.set_encode_quant(step=-1.0)
    finally:
        eng.set_encode_quant()


def test_composition(eng):
    import grok_amd as G
    import torch
    img, kw, okw, bits, sg = _case("rgb")
    step = R.ladder_step(bits, sg, 8)
    qcd = R.qcd_body(step, kw["numresolution"])
    p = G.default_params(**kw)
    try:
        eng.set_encode_quant(step=step)
        cs = eng.encode(img, bits, params=p)
        # packed pixels, host and device
        pix = np.ascontiguousarray(img.transpose(1, 2, 0)).astype(np.uint8)
        assert eng.encode_pixels(pix, bits, params=p) == cs
        # a device-resident input with out=
        out = torch.zeros(len(cs) + 4096, dtype=torch.uint8, device="cuda")
        n = eng.encode(torch.from_numpy(np.array(img)).cuda(), bits, params=p, out=out)
        assert bytes(out[:n].cpu().numpy()) == cs
        # transcode keeps the QCD: to Part-1 and back is the same stream
        p1 = eng.transcode(cs, "part1")
        assert R.find_qcd(p1) == qcd
        assert eng.transcode(p1, "ht") == cs
        # TLM + PLT under a byte target
        eng.set_encode_quant(max_bytes=len(cs) // 2)
        t = eng.encode(img, bits, params=G.default_params(tlm=True, plt=True, **kw))
        assert len(t) <= len(cs) // 2 and b"\xff\x55" in t[:200] and b"\xff\x58" in t
        np.testing.assert_array_equal(eng.decode(t), O.decode(t)[0])
        # RGB to sYCC 4:2:0 in front of the encode
        eng.set_encode_quant(step=step)
        eng.set_encode_convert("sycc", (2, 2))
        y = eng.encode_pixels(pix, bits, params=p)
        eng.set_encode_convert()
        assert R.find_qcd(y) == qcd and len(y) < len(cs)
        got, ref = eng.decode(y), O.decode(y)[0]
        assert len(got) == len(ref) == 3 and ref[1].shape == (44, 36)
        for a, b in zip(got, ref):
            np.testing.assert_array_equal(a, b)
        # a maxshift region (three resolutions: the shift on top of the bands' bit-planes stays
        # within the 25 the ROI check allows)
        eng.set_encode_roi(rects=[(8, 8, 40, 48)])
        roi = _encode(eng, "tiles")
        eng.set_encode_roi()
        assert R.find_qcd(roi) == R.qcd_body(step, 3) and b"\xff\x5e" in roi[:200]
        np.testing.assert_array_equal(eng.decode(roi), O.decode(roi)[0])
    finally:
        eng.set_encode_quant()
        eng.set_encode_convert()
        eng.set_encode_roi()


@pytest.mark.skipif(not openjpeg.available(), reason="libopenjp2 not found")
@pytest.mark.parametrize("name", ["mono12", "rgb", "tiles", "mono16"])
def test_openjpeg_decodes(eng, name):
    """OpenJPEG is another decoder with its own arithmetic (it rebuilds at the bin's centre, as Grok, the
    oracle and the engine do; the bar dates from the oracle's earlier lower-edge rule and holds), so the
    samples may differ; its PSNR against the source is not more than 1 dB below the oracle decode's."""
    img, kw, okw, bits, sg = _case(name)
    for n in (8, 24):
        eng.set_encode_quant(step=R.ladder_step(bits, sg, n))
        cs = _encode(eng, name)
        eng.set_encode_quant()
        opj = np.stack([pl for _, _, pl in openjpeg.decode(cs)])
        a, b = _psnr(opj, img, bits), _psnr(O.decode(cs)[0], img, bits)
        print(name, "notch", n, "openjpeg %.2f dB, oracle %.2f dB" % (a, b))
        assert a >= b - 1.0
