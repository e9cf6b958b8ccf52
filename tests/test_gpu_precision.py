"""Every sample precision on the GPU: the HIP engine against the oracle (which test_precision.py
pins against the source and OpenJPEG) from 1 bit to the highest precision each coding accepts,
its refusal of every precision above, the inverse clamp, and the 1/2/4-byte sample containers.
Precision sets the DC shift and clamp bounds of the DC / MCT / fused level-1 kernels, the sample
container and its vector paths, every band's exponent, bit-planes and step, the HT MAGBp code and
decode scalings, and how close the T1 magnitudes come to the top of their 32 bits."""
import functools

import numpy as np
import pytest
import torch

import grok_amd as G
import oracle as O
import precision_cases as PC

ident = PC.ident

pytestmark = pytest.mark.gpu

REV = [c for c in PC.CODINGS if not c[1]]
IRREV = [c for c in PC.CODINGS if c[1]]


@pytest.fixture(scope="module")
def eng():
    e = G.Engine(0)
    yield e
    e.close()


def gk_encode(eng, img, p, signed, ht, irrev, numres, tiled=False, layer_rate=None, out=None):
    kw, origin = PC.engine_kw(ht, irrev, numres, tiled, layer_rate)
    return eng.encode(img, p, signed=signed, params=G.default_params(**kw), origin=origin, out=out)


def images(p, signed, nc, top):
    out = [("rand", PC.rand(p, signed, nc)), ("chk", PC.chk(p, signed, nc))]
    if p in PC.ENDS_PRECISIONS or p == top:
        out += [("ends%d" % k, a) for k, a in enumerate(PC.ends(p, signed, nc))]
    return out


@functools.lru_cache(maxsize=None)
def eight_bit():
    img = PC.rand(8, False, 3)
    return img, O.encode(img, 8, **PC.oracle_kw(False, False, 3))


@pytest.mark.parametrize("coding", REV, ids=ident)
def test_53_encode_bytes_and_lossless_decode(eng, coding):
    ht, irrev, nc, numres = coding
    top = PC.top(*coding)
    bad = []
    for p in range(1, top + 1):
        for signed in (False, True):
            for name, img in images(p, signed, nc, top):
                ref = O.encode(img, p, signed=signed, **PC.oracle_kw(ht, irrev, numres))
                if gk_encode(eng, img, p, signed, ht, irrev, numres) != ref:
                    bad.append((p, signed, name, "encode"))
                if not np.array_equal(eng.decode(ref), img):
                    bad.append((p, signed, name, "decode"))
    assert not bad


@pytest.mark.parametrize("coding", IRREV, ids=ident)
def test_97_encode_bytes_and_decode(eng, coding):
    ht, irrev, nc, numres = coding
    top = PC.top(*coding)
    bad, worst = [], {}
    for p in range(1, top + 1):
        for signed in (False, True):
            for name, img in images(p, signed, nc, top):
                if nc == 1:   # mono 9/7: the engine's own stream, decoded by both (test_mono_97_quality)
                    cs = gk_encode(eng, img, p, signed, ht, irrev, numres)
                else:
                    cs = O.encode(img, p, signed=signed, **PC.oracle_kw(ht, irrev, numres))
                    if gk_encode(eng, img, p, signed, ht, irrev, numres) != cs:
                        bad.append((p, signed, name, "encode"))
                err = int(np.abs(eng.decode(cs).astype(np.int64) - O.decode(cs)[0]).max())
                worst[p] = max(worst.get(p, 0), err)
                if err > PC.tol97(p):
                    bad.append((p, signed, name, "decode", err, PC.tol97(p)))
    print("9/7 decode, engine against oracle, %s: max per precision %s" % (ident(coding), worst))
    assert not bad


@pytest.mark.parametrize("irrev", [False, True], ids=["53", "97"])
@pytest.mark.parametrize("ht", [False, True], ids=["p1", "ht"])
def test_tiled_offset(eng, ht, irrev):
    # 32 x 32 tiles on an image at canvas (1, 1): odd tile-component origins, the parity-general DWT
    for p in PC.TILED_PRECISIONS:
        for signed in (False, True):
            for nc in (1, 3):
                img = PC.rand(p, signed, nc)
                cs = gk_encode(eng, img, p, signed, ht, irrev, 3, tiled=True)
                if not (irrev and nc == 1):
                    assert cs == O.encode(img, p, signed=signed, **PC.oracle_kw(ht, irrev, 3, tiled=True)), (p, signed, nc)
                dec, dref = eng.decode(cs), O.decode(cs)[0]
                if irrev:
                    assert np.abs(dec.astype(np.int64) - dref).max() <= PC.tol97(p), (p, signed, nc)
                else:
                    assert np.array_equal(dec, img) and np.array_equal(dref, img), (p, signed, nc)


@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("signed", [False, True], ids=["unsigned", "signed"])
@pytest.mark.parametrize("p", PC.CLAMP_PRECISIONS)
def test_inverse_clamp(eng, p, signed, nc):
    # a rate-limited 9/7 stream of full-range noise decodes past both ends of the range: the
    # clamp bounds come from the precision, in the int32 and in the 1- and 2-byte egress
    img = PC.rand(p, signed, nc)
    cs = O.encode(img, p, signed=signed, **PC.oracle_kw(False, True, 3, layer_rate=PC.clamp_rate(p, nc)))
    dref = O.decode(cs)[0]
    lo, hi = PC.sample_range(p, signed)
    assert dref.min() == lo and dref.max() == hi, "the stream does not reach both range ends"
    dec = eng.decode(cs)
    assert dec.min() >= lo and dec.max() <= hi
    assert np.abs(dec.astype(np.int64) - dref).max() <= PC.tol97(p)
    if p <= 16:
        small = eng.decode(cs, sample_bytes=(p + 7) // 8)
        assert small.dtype.itemsize == (p + 7) // 8
        np.testing.assert_array_equal(small.astype(np.int64), dec)


@pytest.mark.parametrize("signed", [False, True], ids=["unsigned", "signed"])
@pytest.mark.parametrize("p", range(1, 17))
def test_sample_containers(eng, p, signed):
    # planar (p + 7) // 8-byte samples in and out, on the host and on the device, against int32
    for nc in (1, 3):
        img = PC.rand(p, signed, nc)
        nb = (p + 7) // 8
        dt = {(1, False): np.uint8, (1, True): np.int8, (2, False): np.uint16, (2, True): np.int16}[(nb, signed)]
        tdt = {np.uint8: torch.uint8, np.int8: torch.int8, np.uint16: torch.int16, np.int16: torch.int16}[dt]
        small = img.astype(dt)
        ref = gk_encode(eng, img, p, signed, False, False, 3)
        assert ref == O.encode(img, p, signed=signed, **PC.oracle_kw(False, False, 3))
        assert gk_encode(eng, small, p, signed, False, False, 3) == ref
        x = torch.from_numpy(small.view(np.int16) if dt == np.uint16 else small).cuda()
        out = torch.empty(small.nbytes * 2 + 4096, dtype=torch.uint8, device="cuda")
        n = gk_encode(eng, x, p, signed, False, False, 3, out=out)
        assert out[:n].cpu().numpy().tobytes() == ref
        dec = eng.decode(ref, sample_bytes=nb)
        assert dec.dtype == dt
        np.testing.assert_array_equal(dec, small)
        np.testing.assert_array_equal(eng.decode(ref), img)
        y = torch.empty(x.shape, dtype=tdt, device="cuda")
        eng.decode(out, length=n, out=y)
        np.testing.assert_array_equal(y.cpu().numpy().view(dt), small)


def test_mode_switch_coder_holds_one_bit_less(eng):
    # the lane-per-block coder of mode switches keeps magnitude << 6 signed: 25 bits.  At 24
    # bits the checkerboard's HH (2^25 - 2) fills it; 25 bits is refused for it alone
    kw = dict(numresolution=2, cblk=PC.CBLK, cblk_sty=2)   # RESET
    img = PC.chk(24, False, 1)
    ref = O.encode(img, 24, numres=2, cblk=PC.CBLK, cblk_sty=2)
    assert eng.encode(img, 24, params=G.default_params(**kw)) == ref
    np.testing.assert_array_equal(eng.decode(ref), img)
    with pytest.raises(RuntimeError, match=r"precision 25\b.*holds 25"):
        eng.encode(PC.chk(25, False, 1), 25, params=G.default_params(**kw))
    assert gk_encode(eng, PC.chk(25, False, 1), 25, False, False, False, 2) == \
        O.encode(PC.chk(25, False, 1), 25, **PC.oracle_kw(False, False, 2))


@pytest.mark.parametrize("coding", PC.CODINGS, ids=ident)
def test_refused_above_the_top(eng, coding):
    # refused on the host, before any launch, with the precision in the message; the engine then
    # encodes as before
    ht, irrev, nc, numres = coding
    img8, ref8 = eight_bit()
    zero = np.zeros((nc, PC.H, PC.W), np.int32)
    for p in range(PC.top(*coding) + 1, 32):
        for signed in (False, True):
            with pytest.raises(RuntimeError, match=r"precision %d\b" % p):
                gk_encode(eng, zero, p, signed, ht, irrev, numres)
            assert gk_encode(eng, img8, 8, False, False, False, 3) == ref8
