"""HT 9/7 quantisation control (gk_set_encode_quant): what needs no GPU.

The interface is declared and exported; the reference rule of tests/htq_ref.py gives the QCD the
oracle writes at the default step; the decode half of its known answer (the sample a decoder
returns for a non-zero index q under the step a QCD's (exponent, mantissa) pair represents is
rint((q + 1/2) * step) + dc, the centre of the bin, as Grok's decoder rebuilds it) holds against
the oracle's decoder on oracle-written
numres = 1 streams whose mantissa is rewritten; the probe reports the ladder and every refusal.
"""
import os
import re

import numpy as np
import pytest

import htq_ref as R
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gk_set_encode_quant", "gk_probe_encode_quant", "gk_get_encode_quant")
HT97 = dict(cblk_sty=0x40, irreversible=True)


def test_exports_declared():
    import grok_amd as G
    with open(os.path.join(ROOT, "include", "grok_amd.h")) as f:
        hdr = f.read()
    lib = G.load_library()
    for n in NAMES:
        assert n in G.EXPORTS
        assert re.search(r"\bint %s\(" % n, hdr), n
        assert hasattr(lib, n)
    for n, v in (("GK_QUANT_STEP", 1), ("GK_QUANT_BYTES", 2), ("GK_QUANT_PSNR", 3)):
        assert re.search(r"#define %s\s+%du" % (n, v), hdr)
        assert getattr(G, n) == v


def _img(seed, prec, signed, h=20, w=16):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << prec, size=(1, h, w)).astype(np.int32)
    return a - (1 << (prec - 1)) if signed else a


@pytest.mark.parametrize("numres", [1, 3, 6])
@pytest.mark.parametrize("prec,signed", [(8, False), (12, False), (12, True), (16, False)])
def test_default_qcd_is_the_oracles(prec, signed, numres):
    cs = O.encode(_img(numres, prec, signed), prec, signed=signed, numres=numres, **HT97)
    assert R.find_qcd(cs) == R.qcd_body(R.ladder_step(prec, signed, 0), numres)


@pytest.mark.parametrize("mant", [300, 1024, 2047])
@pytest.mark.parametrize("prec,signed", [(8, False), (12, False), (12, True)])
def test_lower_edge_reconstruction(prec, signed, mant):
    """An oracle-written numres = 1 stream codes the indices sample - dc at step 1 (signed: 1/2, the
    indices doubled).  With only the QCD mantissa rewritten, the oracle's decoder must return
    rint((index + 1/2) * step') + dc for the step' the new pair represents (dc for index 0): the
    centre of the bin, where Grok's decoder rebuilds (the test keeps its name from the time the
    oracle rebuilt at the lower edge, which Grok's own binaries showed to be a misreading)."""
    img = _img(7 + mant, prec, signed)
    cs = bytearray(O.encode(img, prec, signed=signed, numres=1, **HT97))
    i = cs.find(b"\xff\x5c")
    expn = int.from_bytes(cs[i + 5:i + 7], "big") >> 11
    old = R.band_step(expn, int.from_bytes(cs[i + 5:i + 7], "big") & 0x7ff, prec)
    cs[i + 5:i + 7] = ((expn << 11) | mant).to_bytes(2, "big")
    new = R.band_step(expn, mant, prec)
    dc = 0 if signed else 1 << (prec - 1)
    x = img.astype(np.int64) - dc
    q = np.sign(x) * R.indices(x, old)
    lo, hi = (-(1 << (prec - 1)), (1 << (prec - 1)) - 1) if signed else (0, (1 << prec) - 1)
    want = np.clip(np.rint(np.sign(q) * R.reconstruct(np.abs(q), new)).astype(np.int64) + dc, lo, hi)
    np.testing.assert_array_equal(O.decode(bytes(cs))[0], want)


def test_known_answer_at_the_default_step():
    """The whole rule at the step the oracle's encoder uses: its stream decodes to htq_ref's answer."""
    for prec, signed in ((8, False), (12, True)):
        img = _img(3, prec, signed)
        cs = O.encode(img, prec, signed=signed, numres=1, **HT97)
        e, m = R.band_quant(R.ladder_step(prec, signed, 0), 1)[0]
        np.testing.assert_array_equal(O.decode(cs)[0], R.known_answer(img, prec, signed, R.band_step(e, m, prec)))


@pytest.mark.parametrize("prec", [8, 12, 16])
@pytest.mark.parametrize("signed", [False, True])
def test_probe_ladder(prec, signed):
    import grok_amd as G
    lo, hi, n = G.probe_encode_quant((1, 64, 64), prec, G.default_params(**HT97), signed=signed)
    assert n == 8 * (prec - 1) + 1 == R.notches(prec)
    assert lo == 2.0 ** -(prec + signed) == R.ladder(prec, signed)[0]
    assert hi == 2.0 ** -(1 + signed) == R.ladder(prec, signed)[-1]
    # every notch is accepted, and at the top no band has lost its last bit-plane
    for s in R.ladder(prec, signed):
        G.probe_encode_quant((1, 64, 64), prec, G.default_params(**HT97), step=s, signed=signed)
    assert min(e for e, _ in R.band_quant(hi, 6)) >= 1


REFUSALS = [
    (dict(step=2.0 ** -7), "encode", dict(), "Part-1"),
    (dict(step=2.0 ** -7), "encode", dict(cblk_sty=0x40), "reversible"),
    (dict(psnr=40), "encode", dict(numlayers=2, **HT97), "numlayers"),
    (dict(max_bytes=4000), "encode", dict(layer_rate=[20], **HT97), "layer_rate"),
    (dict(step=2.0 ** -7), "encode", dict(quality=[40], **HT97), "allocationByQuality"),
    (dict(max_bytes=4000), "encode_tiles", dict(tiles=(32, 32), **HT97), "gk_encode_tiles"),
    (dict(psnr=40), "encode_tiles", dict(tiles=(32, 32), **HT97), "gk_encode_tiles"),
    (dict(step=2.0 ** -7), "encode_blocks", dict(**HT97), "gk_encode_blocks"),
    (dict(max_bytes=60), "encode", dict(**HT97), "coarsest notch"),
    (dict(step=2.0 ** -9), "encode", dict(**HT97), "outside"),
    (dict(step=0.75), "encode", dict(**HT97), "outside"),
    (dict(psnr=float("nan")), "encode", dict(**HT97), "finite"),
]


@pytest.mark.parametrize("quant,call,params,name", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_probe_refusals(quant, call, params, name):
    import grok_amd as G
    with pytest.raises(ValueError, match="quant: .*" + re.escape(name)):
        G.probe_encode_quant((1, 64, 64), 8, G.default_params(**params), call=call, **quant)


def test_probe_accepts():
    import grok_amd as G
    G.probe_encode_quant((1, 64, 64), 8, G.default_params(tiles=(32, 32), **HT97), step=2.0 ** -6, call="encode_tiles")
    G.probe_encode_quant((3, 64, 64), 8, G.default_params(tlm=True, plt=True, jp2=True, **HT97), max_bytes=4000)
    G.probe_encode_quant((3, 64, 64), 8, G.default_params(**HT97), psnr=36.5)
    with pytest.raises(ValueError, match="exactly one"):
        G.probe_encode_quant((1, 64, 64), 8, G.default_params(**HT97), step=0.01, psnr=40)
