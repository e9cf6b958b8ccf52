"""HTJ2K with the 9/7 transform on the HIP path vs the oracle.

Grok's own HT 9/7 encoder is R-BUG-2 (T1HT.cpp:88-104 reads the 9/7 float
coefficients through an int32, ~16 dB); this build implements the standard-correct
behaviour (quantisation index trunc(x / stepsize) with the HT irreversible QCD of
param_qcd::set_irrev_quant, HTParams.cpp:273-317) and decodes with Grok's own
ScaleHTFilter rule (PostDecompressFilters.h:161-176), so a stream from this encoder decodes
the same in Grok.  Bar: encode byte-identical to the oracle, decode sample-identical to the
oracle, and the round trip close to the source (tolerance: PSNR >= 45 dB at the default
step sizes).  Grok's encoder writes no sound HT 9/7 stream to compare with; its decoder on these
streams is held live (tests/test_grok_defects.py R-BUG-2 cases, tests/test_gpu_grok_live.py), which
is where the reconstruction point, the centre of the bin, comes from.
"""
import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import grok_amd as G
    e = G.Engine(0)
    yield e
    e.close()


def _img(seed, c, h, w, bits, signed=False):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (np.sin(xx / 11.0 + seed) * np.cos(yy / 6.0) + 1) * (1 << (bits - 2))
    img = base[None].repeat(c, 0) + rng.integers(0, 1 << max(bits - 4, 1), size=(c, h, w))
    img = np.clip(img, 0, (1 << bits) - 1)
    if signed:
        img = img - (1 << (bits - 1))
    return img.astype(np.int32)


def _psnr(a, b, bits):
    mse = np.mean((a.astype(np.float64) - b) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(((1 << bits) - 1) ** 2 / mse)


CASES = [
    dict(seed=1, c=3, h=200, w=230, bits=8, numres=6),
    dict(seed=2, c=1, h=129, w=67, bits=12, numres=4),
    dict(seed=3, c=1, h=96, w=160, bits=16, numres=5),
    dict(seed=4, c=3, h=64, w=64, bits=10, numres=1),
    dict(seed=5, c=1, h=77, w=90, bits=12, numres=3, signed=True),
    dict(seed=6, c=3, h=150, w=170, bits=8, numres=4, tiles=(64, 64)),
]


@pytest.mark.parametrize("case", CASES, ids=[str(i) for i in range(len(CASES))])
def test_ht97_vs_oracle(eng, case):
    import grok_amd as G
    k = dict(case)
    img = _img(k["seed"], k["c"], k["h"], k["w"], k["bits"], k.get("signed", False))
    kw = dict(numresolution=k["numres"], cblk_sty=0x40, irreversible=True)
    okw = dict(numres=k["numres"], cblk_sty=0x40, irreversible=True)
    if "tiles" in k:
        kw["tiles"] = okw["tiles"] = k["tiles"]
    cs = eng.encode(img, k["bits"], signed=k.get("signed", False), params=G.default_params(**kw))
    ref = O.encode(img, k["bits"], signed=k.get("signed", False), **okw)
    assert cs == ref
    dec = eng.decode(ref)
    np.testing.assert_array_equal(dec, O.decode(ref)[0])
    assert _psnr(dec, img, k["bits"]) >= 45.0


def test_ht97_rate_control(eng):
    """HT 9/7 with PCRD layers: HT blocks enter rate control as one pass without a
    distortion record, so every layer-0 block is taken whole (as for HT 5/3)."""
    import grok_amd as G
    img = _img(9, 3, 128, 128, 8)
    cs = eng.encode(img, 8, params=G.default_params(numresolution=5, cblk_sty=0x40, irreversible=True,
                                                     layer_rate=[20, 10], numlayers=2))
    ref = O.encode(img, 8, numres=5, cblk_sty=0x40, irreversible=True, layer_rate=[20, 10])
    assert cs == ref
    np.testing.assert_array_equal(eng.decode(cs), O.decode(ref)[0])
