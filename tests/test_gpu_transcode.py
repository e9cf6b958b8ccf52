"""Transcode Part-1 <-> HTJ2K on the GPU (Engine.transcode): the source coder's T1 decoders hand
quantisation indices to the target coder's T1 encoders; no DWT, MCT or sample stage runs.

Yardsticks: the corpus of OpenJPEG-written streams with its recorded samples (tests/golden/opj),
the oracle's decoder for both coders, and byte equality of round trips.  Bars: a reversible
stream, transcoded, decodes to the recording exactly, by the engine and by the oracle; a 9/7
stream taken Part-1 -> HT -> Part-1 decodes on the engine to exactly what the source decodes to
(the indices are the same, and so is every kernel behind them), and on the oracle within
TOL_97_MAXABS (1, tests/test_gpu_parity.py) of the recording; the engine's own streams come back
byte for byte.  The intermediate HT form of a 9/7 stream carries no sample bar: k_ht_dec
reconstructs an index M at M * step (Grok's ScaleHTFilter), the Part-1 decoders at (M + 1/2) * step.
"""
import ctypes
import struct

import numpy as np
import pytest

import grok_amd as G
import opj_cases as OC
import oracle as O
import encode_colour_cases as E
from grok_amd.synth import synth_image
from test_gpu_parity import TOL_97_MAXABS

pytestmark = pytest.mark.gpu

FX = OC.load()
BY_NAME = {f.name: f for f in FX}
MUST = [f for f in FX if f.expect["layers"] == 1 and not f.expect["irreversible"]]
REST = [f for f in FX if f not in MUST]
TRUNC = "transcode: truncated code-block"
# The streams of the corpus an HT target refuses, with the refusal (from gk_probe_transcode; the
# probe is asserted to give this table below).  Truncated: cut by OpenJPEG's rate control or split
# into layers that leave the last passes out.
REFUSED = {
    "mono8_layers_pterm": TRUNC, "mono8_layers_reset": TRUNC, "mono8_layers_segsym": TRUNC,
    "mono8_layers_termall": TRUNC, "mono8_layers_vsc": TRUNC,
    "rgb12_cinema4k": "transcode: progression order changes (POC) are not supported",
    "rgb8_bypass_rates_97": TRUNC, "rgb8_db_97": TRUNC, "rgb8_layers_mode63_97": TRUNC, "rgb8_rates_97": TRUNC,
    "rgb8_roi_layers_97": TRUNC, "yuv420_97_tiles": TRUNC,
}
ACCEPTED = [f for f in FX if f.name not in REFUSED]
SINGLE_97 = ["mono8_97", "mono12_signed_97", "rgb8_97", "rgb8_97_nomct", "rgb10_97", "mono8_tiles_offset_97",
             "mono8_tiles_thin_97"]


@pytest.fixture(scope="module")
def eng():
    e = G.Engine(0)
    yield e
    e.close()


def coder(cs):
    """The code-block style of a stream's COD (0x40: HT)."""
    lib = G.load_library()
    b = np.frombuffer(bytes(cs), np.uint8)
    info, cp = G.ImageInfo(), G.CParameters()
    msg = ctypes.create_string_buffer(256)
    assert lib.gk_probe_header(b.ctypes.data, len(b), ctypes.byref(info), ctypes.byref(cp), msg, 256) == 0, msg.value
    return cp.cblk_sty, cp


def ora(cs):
    return OC.planes_of(O.decode(cs)[0])


_ht = {}


def ht_of(eng, f):
    """f transcoded to HT, once per module."""
    if f.name not in _ht:
        _ht[f.name] = eng.transcode(f.cs, "ht")
    return _ht[f.name]


def exact(eng, cs, f, what):
    assert OC.maxabs(eng.decode(cs), f.planes) == 0, (f.name, what, "engine")
    assert OC.maxabs(ora(cs), f.planes) == 0, (f.name, what, "oracle")


# ------------------------------------------------------------------ 1. another encoder's streams
@pytest.mark.parametrize("f", MUST, ids=[f.name for f in MUST])
def test_openjpeg_streams_to_ht(eng, f):
    t = ht_of(eng, f)
    sty, cp = coder(t)
    assert sty == 0x40 and cp.numlayers == 1 and not (cp.csty & 6)
    exact(eng, t, f, "HT")


# ------------------------------------------------------------------ 2. the rest of the corpus
def test_refusal_table_is_the_probes():
    got = {}
    for f in FX:
        try:
            G.probe_transcode(f.cs, "ht")
        except ValueError as e:
            got[f.name] = str(e)
    assert sorted(got) == sorted(REFUSED)
    for n, why in got.items():
        assert why.startswith(REFUSED[n]), (n, why)
    assert not set(REFUSED) & {f.name for f in MUST}


@pytest.mark.parametrize("f", REST, ids=[f.name for f in REST])
def test_rest_of_the_corpus(eng, f):
    if f.name in REFUSED:
        with pytest.raises(RuntimeError) as e:
            eng.transcode(f.cs, "ht")
        assert REFUSED[f.name] in str(e.value)
        return
    t = ht_of(eng, f)
    assert coder(t)[0] == 0x40
    if f.lossless:
        exact(eng, t, f, "HT")
    else:   # (no sample bar on the HT form of a 9/7 stream: the shapes only)
        assert [p.shape for p in OC.planes_of(eng.decode(t))] == [p.shape for p in f.planes]


# ------------------------------------------------------------------ 3. Part-1 -> HT -> Part-1
@pytest.mark.parametrize("f", ACCEPTED, ids=[f.name for f in ACCEPTED])
def test_round_trip_through_ht(eng, f):
    back = eng.transcode(ht_of(eng, f), "part1")
    assert coder(back)[0] == 0
    if f.lossless:
        exact(eng, back, f, "Part-1 again")
        return
    assert OC.maxabs(eng.decode(back), eng.decode(f.cs)) == 0, f.name
    d = OC.maxabs(ora(back), f.planes)
    assert d is not None and d <= TOL_97_MAXABS, (f.name, d)


def test_the_single_layer_97_streams_are_accepted():
    assert all(n in BY_NAME and n not in REFUSED for n in SINGLE_97)


# ------------------------------------------------------------------ 4. byte-exact round trips
def _images():
    return {
        "rgb8": (synth_image(80, 96, 3, 8, 11).astype(np.int32), 8, {}, {}),
        "mono16": (synth_image(60, 75, 1, 16, 12).astype(np.int32), 16, {}, {}),
        "tiles_offset": (synth_image(70, 90, 3, 8, 13).astype(np.int32), 8, dict(tiles=(40, 32)), dict(origin=(13, 9))),
        "rgb8_97": (synth_image(72, 88, 3, 8, 14).astype(np.int32), 8, dict(irreversible=True), {}),
    }


@pytest.mark.parametrize("name", ["rgb8", "mono16", "tiles_offset", "rgb8_97"])
def test_own_streams_come_back_byte_for_byte(eng, name):
    img, prec, pkw, ekw = _images()[name]
    S = eng.encode(img, prec, params=G.default_params(**pkw), **ekw)
    H = eng.encode(img, prec, params=G.default_params(cblk_sty=0x40, **pkw), **ekw)
    assert coder(S)[0] == 0 and coder(H)[0] == 0x40
    h = eng.transcode(S, "ht")
    assert coder(h)[0] == 0x40
    assert eng.transcode(h, "part1") == S
    s = eng.transcode(H, "part1")
    assert coder(s)[0] == 0
    assert eng.transcode(s, "ht") == H
    if not pkw.get("irreversible"):
        for cs in (h, s):
            assert np.array_equal(np.asarray(eng.decode(cs)), img)
            assert np.array_equal(np.asarray(O.decode(cs)[0]), img)


ORACLE_WRITTEN = {
    "rgb8_rpcl_prc": (lambda: synth_image(66, 94, 3, 8, 21).astype(np.int32), 8,
                      dict(numres=4, cblk=(32, 32), prog_order=2, precincts=[(64, 64), (32, 32)])),
    "mono12_signed": (lambda: synth_image(50, 61, 1, 12, 22).astype(np.int32) - 2048, 12, dict(numres=3, cblk=(16, 64))),
}


@pytest.mark.parametrize("name", sorted(ORACLE_WRITTEN))
@pytest.mark.parametrize("src_ht", [False, True], ids=["part1_source", "ht_source"])
def test_oracle_written_streams(eng, name, src_ht):
    mk, prec, kw = ORACLE_WRITTEN[name]
    img = mk()
    signed = bool((img < 0).any())
    src = O.encode(img, prec, signed=signed, cblk_sty=0x40 if src_ht else 0, **kw)
    other, own = ("part1", "ht") if src_ht else ("ht", "part1")
    t = eng.transcode(src, other)
    assert coder(t)[0] == (0 if src_ht else 0x40)
    assert np.array_equal(np.asarray(eng.decode(t)), img) and np.array_equal(np.asarray(O.decode(t)[0]), img)
    back = eng.transcode(t, own)
    assert np.array_equal(np.asarray(eng.decode(back)), img) and np.array_equal(np.asarray(O.decode(back)[0]), img)
    assert back[back.index(b"\xff\x90"):] == src[src.index(b"\xff\x90"):]


# ------------------------------------------------------------------ 5. JP2
def _boxes(data):
    """[(type, offset, length, header bytes)] of a JP2 file's top-level boxes."""
    out, pos = [], 0
    while pos + 8 <= len(data):
        L, T = struct.unpack(">I4s", data[pos:pos + 8])
        hdr = 8
        if L == 1:
            L, hdr = struct.unpack(">Q", data[pos + 8:pos + 16])[0], 16
        elif L == 0:
            L = len(data) - pos
        out.append((T, pos, L, hdr))
        pos += L
    assert pos == len(data)
    return out


def test_jp2_keeps_its_boxes(eng):
    c = E.cases()["icc_opacity"]
    eng.set_encode_colour(**c.kw)
    try:
        src = eng.encode(c.src, c.prec, params=G.default_params(numresolution=3, jp2=True, mct=False))
    finally:
        eng.set_encode_colour()
    t = eng.transcode(src, "ht")
    bs, bt = _boxes(src), _boxes(t)
    assert [b[0] for b in bs] == [b[0] for b in bt] and b"jp2c" in [b[0] for b in bs]
    for (T, p0, L0, h0), (_, p1, L1, h1) in zip(bs, bt):
        if T == b"jp2c":
            assert h0 == h1 and coder(t[p1 + h1:p1 + L1])[0] == 0x40 and coder(src[p0 + h0:p0 + L0])[0] == 0
        else:   # (ftyp included: the engine writes one brand for both coders)
            assert src[p0:p0 + L0] == t[p1:p1 + L1], T
    eng.read_header(src)
    ci0, icc0 = bytes(eng.colour_info()), eng.icc_profile()
    eng.read_header(t)
    assert bytes(eng.colour_info()) == ci0 and eng.icc_profile() == icc0 == E.ICC
    assert np.array_equal(eng.decode_pixels(t, sample_bytes=1), eng.decode_pixels(src, sample_bytes=1))
    assert eng.transcode(t, "part1") == src


# ------------------------------------------------------------------ 6. memory spaces
def test_memory_spaces_and_capacity(eng):
    import torch
    f = BY_NAME["rgb8_tiles_odd"]
    want = eng.transcode(f.cs, "ht")
    dev = torch.frombuffer(bytearray(f.cs), dtype=torch.uint8).cuda()
    out = torch.zeros(len(want) + 64, dtype=torch.uint8, device="cuda")
    n = eng.transcode(dev, "ht", out=out, length=len(f.cs))
    assert n == len(want) and bytes(out[:n].cpu().numpy()) == want
    assert eng.transcode(dev, "ht", length=len(f.cs)) == want
    # too small: -2 with the size needed, and nothing stays
    b = np.frombuffer(f.cs, np.uint8)
    tp = G.TranscodeParams(G.GK_TRANSCODE_HT, 0, 0, 1)
    small = np.zeros(16, np.uint8)
    need = ctypes.c_size_t()
    rc = eng.lib.gk_transcode(eng.ctx, b.ctypes.data, len(b), 0, ctypes.byref(tp), small.ctypes.data, small.size, 0,
                              ctypes.byref(need))
    assert rc == -2 and need.value == len(want) and not small.any()
    assert eng.transcode(f.cs, "ht") == want
    assert OC.maxabs(eng.decode(f.cs), f.planes) == 0


def test_markers_follow_the_params(eng):
    f = BY_NAME["rgb8_tiles_offset"]
    plain = eng.transcode(f.cs, "ht")
    both = eng.transcode(f.cs, "ht", tlm=True, plt=True)
    head = both[:both.index(b"\xff\x90")]
    assert b"\xff\x55" in head and b"\xff\x55" not in plain[:plain.index(b"\xff\x90")]
    assert b"\xff\x58" in both and len(both) > len(plain)
    exact(eng, both, f, "HT with TLM and PLT")
    com = BY_NAME["rgb8_com"]
    kept, dropped = eng.transcode(com.cs, "ht"), eng.transcode(com.cs, "ht", com=False)
    assert b"\xff\x64" in kept[:kept.index(b"\xff\x90")] and b"\xff\x64" not in dropped[:dropped.index(b"\xff\x90")]


def test_no_transform_runs(eng):
    eng.transcode(BY_NAME["rgb8_default"].cs, "ht")
    t = eng.timings()
    assert t.dwt_ms == 0 and t.mct_ms == 0 and t.dwt_launches == 0 and t.dwt_bytes == 0
    assert t.t1_blocks > 0 and t.t1_ms > 0


# ------------------------------------------------------------------ 7. refusals and history
def test_refusals_and_history(eng):
    img = synth_image(64, 80, 3, 8, 31).astype(np.int32)
    layered = eng.encode(img, 8, params=G.default_params(numresolution=4, layer_rate=[40.0, 10.0]))
    A = BY_NAME["rgb8_tiles_offset"]
    B = BY_NAME["rgb8_mode63"]
    first = OC.planes_of(eng.decode(A.cs))                          # 1. decode A
    assert OC.maxabs(first, A.planes) == 0
    tb = eng.transcode(B.cs, "ht")                                  # 2. transcode B
    with pytest.raises(RuntimeError, match=r"truncated code-block \(tile 0, component \d+, resolution \d+, band "
                                           r"(LL|HL|LH|HH), block \d+: \d+ of \d+ passes\)"):
        eng.transcode(layered, "ht")                                # 3. refused calls
    with pytest.raises(RuntimeError, match="already coded with the target coder"):
        eng.transcode(tb, "ht")
    eng.set_decode_reduce(1)
    try:
        with pytest.raises(RuntimeError, match="gk_set_decode_reduce"):
            eng.transcode(B.cs, "ht")
    finally:
        eng.set_decode_reduce(0)
    eng.set_decode_layers(1)
    try:
        with pytest.raises(RuntimeError, match="gk_set_decode_layers"):
            eng.transcode(B.cs, "ht")
    finally:
        eng.set_decode_layers(0)
    assert eng.transcode(B.cs, "ht") == tb                           # 4. B again, and on a fresh engine
    fresh = G.Engine(0)
    try:
        assert fresh.transcode(B.cs, "ht") == tb
        want_enc = fresh.encode(img, 8)
    finally:
        fresh.close()
    assert OC.maxabs(eng.decode(A.cs), first) == 0                   # 5. decode A again
    assert eng.encode(img, 8) == want_enc                            # 6. an encode afterwards
    assert eng.encode(img, 8, params=G.default_params(cblk_sty=0x40)) == O.encode(img, 8, cblk_sty=0x40)
