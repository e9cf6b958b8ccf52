"""Reference rule of the HT 9/7 quantisation control (gk_set_encode_quant), restated in numpy.

* the notch ladder: base_step(n) = 2^-(prec + signed) * 2^(n / 8), n = 0 .. 8 (prec - 1);
* the QCD a base step gives: band b takes base_step / (gl gh), the band's 9/7 synthesis gain, as an
  (exponent, mantissa) pair; float32 arithmetic, as param_qcd::set_irrev_quant computes it;
* the step that pair represents, in sample levels (what the encoder divides by and every decoder
  multiplies with);
* the known answer of a numres = 1 encode without MCT: the only band is LL with gain 1, its
  coefficient is sample - dc, the index trunc(|x| * (1 / step)) in float32 (the encoder multiplies
  by the reciprocal step) and the decoded sample clip(rint((index + 1/2) * step) + dc) for a
  non-zero index, dc for index 0: the centre of the bin, which the HT block decoder Grok uses puts
  one bit under the magnitude and Grok's ScaleHTFilter scales with it (grk_decompress on these
  streams: tests/test_grok_live.py);
* the squared quantisation error of coefficients at a step (k_htq_dist's sum), in float64.
"""
import numpy as np

# sqrt of the 9/7 synthesis energy gains by decomposition level (constant data of the filter bank)
L97 = np.array([1.0000e+00, 1.4021e+00, 2.0304e+00, 2.9012e+00, 4.1153e+00, 5.8245e+00, 8.2388e+00, 1.1652e+01,
                1.6479e+01, 2.3304e+01, 3.2957e+01, 4.6609e+01, 6.5915e+01, 9.3217e+01, 1.3183e+02, 1.8643e+02,
                2.6366e+02, 3.7287e+02, 5.2732e+02, 7.4574e+02, 1.0546e+03, 1.4915e+03, 2.1093e+03, 2.9830e+03,
                4.2185e+03, 5.9659e+03, 8.4371e+03, 1.1932e+04, 1.6874e+04, 2.3864e+04, 3.3748e+04, 4.7727e+04,
                6.7496e+04, 9.5454e+04], dtype=np.float32)
H97 = np.array([1.4425e+00, 1.9669e+00, 2.8839e+00, 4.1475e+00, 5.8946e+00, 8.3472e+00, 1.1809e+01, 1.6701e+01,
                2.3620e+01, 3.3403e+01, 4.7240e+01, 6.6807e+01, 9.4479e+01, 1.3361e+02, 1.8896e+02, 2.6723e+02,
                3.7792e+02, 5.3446e+02, 7.5583e+02, 1.0689e+03, 1.5117e+03, 2.1378e+03, 3.0233e+03, 4.2756e+03,
                6.0467e+03, 8.5513e+03, 1.2093e+04, 1.7103e+04, 2.4187e+04, 3.4205e+04, 4.8373e+04, 6.8410e+04,
                9.6747e+04, 1.3682e+05], dtype=np.float32)
# 2^(k / 8), k = 0 .. 7
_FRAC = (1.0, 1.0905077326652577, 1.189207115002721, 1.2968395546510096, 1.4142135623730951, 1.5422108254079407,
         1.681792830507429, 1.8340080864093424)


def notches(prec):
    return 8 * (prec - 1) + 1


def ladder_step(prec, signed, n):
    """Base step of notch n (float64)."""
    return float(np.ldexp(_FRAC[n & 7], (n >> 3) - (prec + (1 if signed else 0))))


def ladder(prec, signed=False):
    return [ladder_step(prec, signed, n) for n in range(notches(prec))]


def bands(numres):
    """(resolution, orientation) of the bands in QCD order: LL, then HL, LH, HH per resolution."""
    return [(0, 0)] + [(r, o) for r in range(1, numres) for o in (1, 2, 3)]


def gain(numres, r, orient):
    """gl * gh of a band (float32)."""
    nd = numres - 1
    if r == 0:
        return np.float32(L97[nd] * L97[nd])
    d = nd - r
    return np.float32((H97[d] if orient == 3 else L97[d + 1]) * H97[d])


def band_quant(step, numres):
    """[(exponent, mantissa)] of the bands for the base step, in QCD order."""
    out = []
    for r, o in bands(numres):
        delta = np.float32(np.float32(step) / gain(numres, r, o))
        e = 0
        while delta < np.float32(1.0):
            e += 1
            delta = np.float32(delta * np.float32(2.0))
        m = int(np.floor(np.float64(delta) * 2048.0 + 0.5)) - 2048
        out.append((e, m if m < 2048 else 0x7ff))
    return out


def qcd_body(step, numres, guard=1):
    """The QCD marker's body (Sqcd, SPqcd): scalar expounded."""
    b = bytes([(guard << 5) | 2])
    for e, m in band_quant(step, numres):
        b += int((e << 11) | m).to_bytes(2, "big")
    return b


def find_qcd(cs):
    """The body of the first QCD marker of a codestream (or of the codestream inside a JP2 file)."""
    cs = bytes(cs)
    i = cs.find(b"\xff\x4f\xff\x51")
    assert i >= 0, "no codestream"
    i += 2
    while cs[i:i + 2] != b"\xff\x90":
        n = int.from_bytes(cs[i + 2:i + 4], "big")
        if cs[i:i + 2] == b"\xff\x5c":
            return cs[i + 4:i + 2 + n]
        i += 2 + n
    raise AssertionError("no QCD marker")


def band_step(expn, mant, prec, orient=0):
    """The step an (exponent, mantissa) pair represents, in sample levels (float32; exact)."""
    lg = (0, 1, 1, 2)[orient]
    return np.float32((1.0 + mant / 2048.0) * 2.0 ** (prec + lg - expn))


def indices(x, delta):
    """The encoder's index magnitudes of coefficients x at step delta: trunc(|x| * (1 / delta)), float32."""
    a = np.abs(np.asarray(x, dtype=np.float32))
    inv = np.float32(1.0) / np.float32(delta)
    return np.trunc(a * inv).astype(np.float32)


def reconstruct(q, delta):
    """The coefficient magnitude a decoder rebuilds from index magnitude q at step delta: the centre
    of the bin, (2 q + 1) * (delta / 2) in float32 (one rounding: the halving is exact), 0 for q = 0."""
    q = np.asarray(q, dtype=np.float32)
    return np.where(q > 0, (2 * q + 1) * (np.float32(delta) * np.float32(0.5)), np.float32(0)).astype(np.float32)


def known_answer(img, prec, signed, delta):
    """Decoded samples of a numres = 1 encode without MCT at LL step delta (sample levels)."""
    dc = 0 if signed else 1 << (prec - 1)
    x = np.asarray(img, dtype=np.int64) - dc
    rec = np.sign(x).astype(np.float32) * reconstruct(indices(x, delta), delta)
    lo, hi = (-(1 << (prec - 1)), (1 << (prec - 1)) - 1) if signed else (0, (1 << prec) - 1)
    return np.clip(np.rint(rec).astype(np.int64) + dc, lo, hi).astype(np.int32)


def band_error(x, delta):
    """Sum of (|x| - index * delta)^2 over coefficients x, in float64."""
    a = np.abs(np.asarray(x, dtype=np.float32)).astype(np.float64)
    return float(np.sum((a - indices(x, delta).astype(np.float64) * float(np.float32(delta))) ** 2))
