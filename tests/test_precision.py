"""Every sample precision on the CPU: the oracle (the GPU tests' reference, test_gpu_precision.py)
against the source and against OpenJPEG 2.5.4, from 1 bit to the highest precision each coding
accepts, and its refusal of every precision above."""
import numpy as np
import pytest

import openjpeg as OJ
import oracle as O
import precision_cases as PC

needs_openjpeg = pytest.mark.skipif(not OJ.available(), reason="libopenjp2 (Pillow's pillow.libs) not found")

# 9/7 HT, oracle against OpenJPEG: the largest difference measured per precision over every case
# below; the tests allow one LSB more for case-to-case variation.  9/7 Part 1: 0,
# the two decoders run the same float operations in the same order.
HT97_MEASURED = {1: 1, 2: 1, 3: 2, 21: 4, 22: 3, 23: 5, 24: 12, 25: 16}   # 4..20: 3


def ht97_bound(p):
    return HT97_MEASURED.get(p, 3) + 1


def images(p, signed, nc):
    return [("rand", PC.rand(p, signed, nc)), ("chk", PC.chk(p, signed, nc))] + \
        [("ends%d" % k, a) for k, a in enumerate(PC.ends(p, signed, nc))]


def openjpeg_planes(cs):
    return np.stack([a for _, _, a in OJ.decode(cs)])


ident = PC.ident
REV = [c for c in PC.CODINGS if not c[1]]
IRREV = [c for c in PC.CODINGS if c[1]]


@needs_openjpeg
@pytest.mark.parametrize("coding", REV, ids=ident)
def test_53_lossless_in_both_decoders(coding):
    ht, irrev, nc, numres = coding
    bad = []
    for p in range(1, PC.top(*coding) + 1):
        for signed in (False, True):
            for name, img in images(p, signed, nc):
                cs = O.encode(img, p, signed=signed, **PC.oracle_kw(ht, irrev, numres))
                dec, prec = O.decode(cs)
                if prec != p or not np.array_equal(dec, img):
                    bad.append((p, signed, name, "oracle"))
                if not np.array_equal(openjpeg_planes(cs), img):
                    bad.append((p, signed, name, "openjpeg"))
    assert not bad


@needs_openjpeg
@pytest.mark.parametrize("ht", [False, True], ids=["p1", "ht"])
def test_53_tiled_offset_lossless(ht):
    for p in PC.TILED_PRECISIONS:
        for signed in (False, True):
            for nc in (1, 3):
                img = PC.rand(p, signed, nc)
                cs = O.encode(img, p, signed=signed, **PC.oracle_kw(ht, False, 3, tiled=True))
                np.testing.assert_array_equal(O.decode(cs)[0], img)
                np.testing.assert_array_equal(openjpeg_planes(cs), img)


@needs_openjpeg
@pytest.mark.parametrize("coding", IRREV, ids=ident)
def test_97_oracle_matches_openjpeg(coding):
    ht, irrev, nc, numres = coding
    bad = []
    for p in range(1, PC.top(*coding) + 1):
        bound = ht97_bound(p) if ht else 0
        for signed in (False, True):
            lo, hi = PC.sample_range(p, signed)
            for name, img in images(p, signed, nc):
                cs = O.encode(img, p, signed=signed, **PC.oracle_kw(ht, irrev, numres))
                dec = O.decode(cs)[0].astype(np.int64)
                err = int(np.abs(dec - openjpeg_planes(cs)).max())
                if err > bound or dec.min() < lo or dec.max() > hi:
                    bad.append((p, signed, name, err, bound))
    assert not bad


@pytest.mark.parametrize("coding", PC.CODINGS, ids=ident)
def test_refused_above_the_top(coding):
    ht, irrev, nc, numres = coding
    img = np.zeros((nc, PC.H, PC.W), np.int32)
    for p in range(PC.top(*coding) + 1, 32):
        for signed in (False, True):
            with pytest.raises(RuntimeError, match=r"precision %d\b" % p):
                O.encode(img, p, signed=signed, **PC.oracle_kw(ht, irrev, numres))
    O.encode(img, PC.top(*coding), **PC.oracle_kw(ht, irrev, numres))   # the top itself is accepted


@pytest.mark.parametrize("nc,numres,p", [(3, 3, 24), (3, 6, 24), (1, 3, 25)])
def test_second_level_overflow_is_refused(nc, numres, p):
    """Part-1 5/3 one bit above the top: the rand / chk / ends images round-trip, an image laid
    out along the second level's high-pass filter does not fit 26 magnitude bits (it decoded
    with errors of 2^24 before the refusal).  One bit lower the same image is lossless."""
    with pytest.raises(RuntimeError, match=r"precision %d\b" % p):
        O.encode(PC.worst_hl(p, nc), p, **PC.oracle_kw(False, False, numres))
    img = PC.worst_hl(p - 1, nc)
    cs = O.encode(img, p - 1, **PC.oracle_kw(False, False, numres))
    np.testing.assert_array_equal(O.decode(cs)[0], img)


def test_tile_part_encode_refuses_too():
    img = np.zeros((1, PC.H, PC.W), np.int32)
    with pytest.raises(RuntimeError, match=r"precision 26\b"):
        O.encode_tile_parts(img, 0, (PC.H, PC.W), 26, 0, 1, **PC.oracle_kw(False, False, 3))
