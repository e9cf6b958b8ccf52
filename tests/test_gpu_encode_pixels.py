"""Encode from packed pixels on the GPU (k_unpixels, gk_unpixels.hip) through Engine.encode_pixels.

Truth: the same engine's planar encode of the same samples, byte for byte
(encode(np.ascontiguousarray(np.moveaxis(pix, 2, 0)))); four cases are also held to oracle.encode of
the planes.  Random pixels carry a per-channel offset, so a swapped channel cannot pass.

The shapes walk every path of the kernel: the tail group (widths 1, 7, 9), one whole lane (8), the
second workgroup in x (2049), a partial row group (5 rows), the register-resident template (1..4
channels) and the channel-at-a-time variant (5, 16), 16- / 8- / 4-byte loads and the realigned
dwords of rows that start 1..3 bytes past a dword boundary (tight odd-width u8 RGB, device slices)."""
import ctypes

import numpy as np
import pytest
import torch

import grok_amd as G
import display_cases as C
import oracle as O

pytestmark = pytest.mark.gpu

# kind: (numpy dtype, torch dtype, precision, signed)
KINDS = {
    "u8": (np.uint8, torch.uint8, 8, False),
    "u16p12": (np.uint16, torch.int16, 12, False),
    "u16p16": (np.uint16, torch.int16, 16, False),
    "i16p12": (np.int16, torch.int16, 12, True),
    "i32p8": (np.int32, torch.int32, 8, False),
    "i32p20": (np.int32, torch.int32, 20, False),
}


@pytest.fixture(scope="module")
def eng():
    e = G.Engine(0)
    yield e
    e.close()


def pixels(w, h, c, kind, seed=0):
    """(h, w, c) random samples of the kind's dtype; channel k sits in its own band of the range."""
    dt, _, prec, signed = KINDS[kind]
    rng = np.random.RandomState(seed * 131 + w * 7 + h * 3 + c)
    span = (1 << prec) // (c + 1)
    lo = -(1 << (prec - 1)) if signed else 0
    x = rng.randint(0, max(span, 1), (h, w, c)).astype(np.int64) + lo + np.arange(c)[None, None, :] * span
    x[0, 0, :] = lo + np.arange(c) * span                         # (each band's floor and, below, the range's top)
    x[-1, -1, c - 1] = lo + (1 << prec) - 1
    return x.astype(dt)


def planes_of(pix):
    return np.ascontiguousarray(np.moveaxis(pix, 2, 0))


def params(w, h, **kw):
    kw.setdefault("numresolution", C.numres_for(w, h, [(1, 1)]))
    return G.default_params(**kw)


def to_dev(a, tdt):
    """The numpy array's bits as a cuda tensor of the torch type of the same size."""
    return torch.from_numpy(a.view({1: np.uint8, 2: np.int16, 4: np.int32}[a.dtype.itemsize]).copy()).to("cuda").view(tdt)


def place(pix, kind, pitch, mem):
    """The pixels as the case hands them over: a host array or device tensor whose rows lie `pitch`."""
    dt, tdt, _, _ = KINDS[kind]
    h, w, c = pix.shape
    es = pix.dtype.itemsize
    if pitch == "slice":                                          # big[2:2+h, 3:3+w, :]: rows and base off every boundary
        big = np.full((h + 3, w + 5, c), 0x55, dt)
        big[2:2 + h, 3:3 + w, :] = pix
        if mem == "host":
            return big[2:2 + h, 3:3 + w, :]
        return to_dev(big, tdt)[2:2 + h, 3:3 + w, :]
    row = {"tight": w * c, "tight+es": w * c + 1, "pad64": -(-(w * c * es) // 64) * 64 // es}[pitch]
    buf = np.full((h, row), 0x55, dt)
    buf[:, :w * c] = pix.reshape(h, w * c)
    if mem == "host":
        return buf[:, :w * c].reshape(h, w, c) if row == w * c else np.lib.stride_tricks.as_strided(
            buf, (h, w, c), (row * es, c * es, es))
    t = to_dev(buf, tdt)
    return t[:, :w * c].unflatten(1, (w, c))


# (w, h, c, kind, pitch, pixel memory, output memory): every value of every axis, every load path
CASES = [
    # u8: tight odd widths with C = 3 start rows at every byte misalignment (the alignbyte path)
    (1, 1, 1, "u8", "tight", "host", "host"),
    (7, 5, 3, "u8", "tight", "dev", "host"),
    (8, 5, 3, "u8", "tight", "dev", "dev"),
    (9, 5, 3, "u8", "tight", "dev", "host"),
    (2047, 5, 3, "u8", "tight", "dev", "host"),
    (2048, 1, 3, "u8", "tight", "host", "host"),
    (2049, 5, 3, "u8", "tight", "dev", "host"),
    (2049, 5, 3, "u8", "tight", "host", "dev"),
    (2049, 5, 3, "u8", "pad64", "dev", "host"),                   # 16-byte loads (C * 8 = 24: 8-byte loads)
    (2049, 5, 3, "u8", "tight+es", "dev", "host"),
    (2049, 5, 3, "u8", "slice", "dev", "host"),
    (2047, 5, 1, "u8", "tight", "dev", "host"),
    (2049, 5, 1, "u8", "pad64", "dev", "host"),
    (2048, 5, 2, "u8", "pad64", "dev", "host"),                   # 16-byte rows, 16-byte loads
    (9, 1, 2, "u8", "slice", "dev", "host"),
    (2049, 5, 4, "u8", "pad64", "dev", "host"),
    (2047, 5, 4, "u8", "tight+es", "dev", "host"),
    (33, 5, 4, "u8", "slice", "host", "host"),
    (2049, 5, 5, "u8", "tight", "dev", "host"),                   # channel-at-a-time
    (9, 5, 16, "u8", "tight+es", "host", "host"),
    (2048, 1, 16, "u8", "pad64", "dev", "dev"),
    # u16, precisions 12 and 16
    (1, 5, 3, "u16p12", "tight", "dev", "host"),
    (7, 1, 2, "u16p12", "tight", "host", "host"),
    (8, 5, 1, "u16p12", "tight", "dev", "host"),
    (9, 5, 3, "u16p12", "tight+es", "dev", "host"),               # rows 2 bytes off a dword: realigned
    (2047, 5, 3, "u16p12", "tight", "dev", "host"),
    (2049, 5, 3, "u16p12", "pad64", "dev", "dev"),
    (2049, 5, 3, "u16p12", "slice", "dev", "host"),
    (2048, 5, 4, "u16p12", "tight", "host", "host"),
    (2049, 1, 4, "u16p16", "slice", "dev", "host"),
    (2049, 5, 2, "u16p16", "tight+es", "dev", "host"),
    (2047, 5, 1, "u16p16", "tight", "dev", "host"),
    (33, 5, 5, "u16p16", "tight", "dev", "host"),
    (2049, 5, 16, "u16p12", "pad64", "host", "host"),
    # signed 12 in int16
    (7, 5, 3, "i16p12", "tight", "dev", "host"),
    (2049, 5, 3, "i16p12", "slice", "dev", "dev"),
    (2048, 5, 4, "i16p12", "pad64", "host", "host"),
    (9, 1, 1, "i16p12", "tight+es", "dev", "host"),
    (8, 5, 5, "i16p12", "tight", "dev", "host"),
    # int32, precisions 8 and 20
    (1, 1, 3, "i32p8", "tight", "dev", "host"),
    (7, 5, 4, "i32p8", "tight", "host", "host"),
    (9, 5, 3, "i32p8", "tight+es", "dev", "host"),                # 4-byte loads
    (2049, 5, 3, "i32p8", "pad64", "dev", "host"),                # 16-byte loads
    (2047, 5, 1, "i32p8", "slice", "dev", "host"),
    (2049, 5, 2, "i32p20", "tight+es", "dev", "dev"),             # every other row 8-byte aligned
    (2048, 5, 3, "i32p20", "tight", "dev", "host"),
    (2049, 5, 4, "i32p20", "slice", "dev", "host"),
    (2049, 1, 5, "i32p20", "tight", "host", "host"),
    (8, 5, 16, "i32p20", "slice", "dev", "host"),
]
assert len(CASES) <= 60
ORACLE = {(2049, 5, 3, "u8", "slice", "dev", "host"), (2049, 5, 3, "u16p12", "slice", "dev", "host"),
          (2049, 5, 3, "i16p12", "slice", "dev", "dev"), (2049, 5, 4, "i32p20", "slice", "dev", "host")}
assert ORACLE <= set(CASES)


def run(eng, src, prec, signed, p, out_mem, cap):
    if out_mem == "host":
        return eng.encode_pixels(src, prec, signed=signed, params=p)
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    n = eng.encode_pixels(src, prec, signed=signed, params=p, out=out)
    return out[:n].cpu().numpy().tobytes()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_unpack_matches_planar(eng, case):
    w, h, c, kind, pitch, mem, out_mem = case
    _, _, prec, signed = KINDS[kind]
    pix = pixels(w, h, c, kind)
    p = params(w, h, mct=c >= 3)
    want = eng.encode(planes_of(pix), prec, signed=signed, params=p)
    src = place(pix, kind, pitch, mem)
    got = run(eng, src, prec, signed, p, out_mem, w * h * c * 4 + (1 << 20))
    assert got == want
    if case in ORACLE:
        assert got == O.encode(planes_of(pix).astype(np.int32), prec, signed=signed, numres=p.numresolution, mct=c >= 3)


# one case each through the other front ends and coders
@pytest.mark.parametrize("name,kw,origin", [
    ("tiles64", dict(tiles=(64, 64), numresolution=3), None),
    ("odd_origin", dict(numresolution=3), (3, 5)),                # the unfused front end
    ("97_layers", dict(irreversible=True, layer_rate=[40, 20, 10], numresolution=4), None),
    ("ht", dict(cblk_sty=0x40, numresolution=4), None),
    ("numres1", dict(numresolution=1), None),
    ("jp2", dict(jp2=True, numresolution=3), None),
])
def test_coding_paths(eng, name, kw, origin):
    w, h, c = 203, 131, 3
    pix = pixels(w, h, c, "u8", seed=len(name))
    p = G.default_params(**kw)
    want = eng.encode(planes_of(pix), 8, params=p, origin=origin)
    for mem in ("host", "dev"):
        got = eng.encode_pixels(place(pix, "u8", "slice", mem), 8, params=p, origin=origin)
        assert got == want, (name, mem)


def test_device_tensor_of_floats_is_refused(eng):
    x = torch.zeros((4, 4, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="integers"):
        eng.encode_pixels(x, 8)


def test_two_dimensional_input(eng):
    pix = pixels(37, 9, 1, "u8")
    p = params(37, 9)
    assert eng.encode_pixels(pix[:, :, 0], 8, params=p) == eng.encode(planes_of(pix), 8, params=p)


def test_small_capacity_reports_the_size(eng):
    pix = pixels(64, 64, 3, "u8")
    p = params(64, 64)
    want = eng.encode(planes_of(pix), 8, params=p)
    info = G.ImageInfo(64, 64, 3, 8, 0, 1)
    buf, n = np.empty(16, np.uint8), ctypes.c_size_t()
    rc = eng.lib.gk_encode_pixels(eng.ctx, ctypes.byref(info), pix.ctypes.data, 64 * 3, 0, ctypes.byref(p),
                                  buf.ctypes.data, 16, ctypes.byref(n), 0)
    assert rc == -2 and n.value == len(want)
    assert eng.encode_pixels(pix, 8, params=p) == want


def test_round_trip_through_decode_pixels(eng):
    pix = pixels(131, 67, 4, "u8")
    cs = eng.encode_pixels(pix, 8, params=params(131, 67, mct=True, jp2=True))
    np.testing.assert_array_equal(eng.decode_pixels(cs, sample_bytes=1), pix)


# ---------------------------------------------------------------- refusals (host-side checks)
def raw(eng, info, pix, row_bytes, p):
    buf, n = np.empty(1 << 20, np.uint8), ctypes.c_size_t()
    rc = eng.lib.gk_encode_pixels(eng.ctx, ctypes.byref(info), pix.ctypes.data, row_bytes, 0, ctypes.byref(p),
                                  buf.ctypes.data, buf.size, ctypes.byref(n), 0)
    return rc, eng.lib.gk_last_error(eng.ctx).decode()


def test_refusals_name_the_cause_and_leave_the_engine_usable(eng):
    w, h, c = 40, 12, 3
    pix = pixels(w, h, c, "u16p12")
    p = params(w, h)
    want = eng.encode(planes_of(pix), 12, params=p)

    def still_good():
        assert eng.encode_pixels(pix, 12, params=p) == want

    info = G.ImageInfo(w, h, c, 12, 0, 2)
    rc, msg = raw(eng, info, pix, w * c * 2 - 2, p)               # short rows
    assert rc == -1 and "row_bytes" in msg and "below" in msg
    still_good()
    rc, msg = raw(eng, info, pix, w * c * 2 + 1, p)               # rows that split a sample
    assert rc == -1 and "row_bytes" in msg and "multiple" in msg
    still_good()
    odd = np.zeros(w * h * c * 2 + 2, np.uint8)[1:]                # a buffer one byte off its 16-bit samples
    rc, msg = raw(eng, info, odd, w * c * 2, p)
    assert rc == -1 and "aligned" in msg
    still_good()
    rc, msg = raw(eng, G.ImageInfo(w, h, c, 12, 0, 1), pix, w * c * 2, p)   # 12 bits in one byte
    assert rc == -1 and "sample_bytes" in msg
    still_good()
    wide = np.zeros((4, 4, 17), np.uint16)
    rc, msg = raw(eng, G.ImageInfo(4, 4, 17, 12, 0, 2), wide, 4 * 17 * 2, p)
    assert rc == -1 and "16 channels" in msg and "planar" in msg
    still_good()
    assert eng.lib.gk_set_subsampling(eng.ctx, 3, (ctypes.c_uint32 * 3)(1, 2, 2), (ctypes.c_uint32 * 3)(1, 2, 2)) == 0
    try:
        with pytest.raises(RuntimeError, match="subsampling"):
            eng.encode_pixels(pix, 12, params=p)
    finally:
        assert eng.lib.gk_set_subsampling(eng.ctx, 0, None, None) == 0
    still_good()
    rc, msg = raw(eng, G.ImageInfo(w, h, c, 0, 0, 0), pix, w * c * 4, p)    # what gk_encode refuses, unchanged
    assert rc == -1 and "precision" in msg
    still_good()


def test_history_refused_call_leaves_the_next_encode_unchanged(eng):
    """A fresh engine's planar encode equals this engine's after pixel encodes and a refusal."""
    pix = pixels(90, 33, 3, "u8", seed=5)
    p = params(90, 33)
    eng.encode_pixels(pixels(2049, 5, 4, "i32p20"), 20, params=params(2049, 5))
    rc, _ = raw(eng, G.ImageInfo(90, 33, 3, 8, 0, 1), pix, 10, p)
    assert rc == -1
    got = eng.encode(planes_of(pix), 8, params=p)
    fresh = G.Engine(0)
    try:
        assert fresh.encode(planes_of(pix), 8, params=p) == got
        assert fresh.encode_pixels(pix, 8, params=p) == got
    finally:
        fresh.close()
