"""Streams written by OpenJPEG's encoder (tests/golden/opj, tests/golden/make_opj_fixtures.py), on
the CPU: the oracle against OpenJPEG's recorded decode of every stream, the fixtures against a
fresh OpenJPEG decode, and the engine's host header probes against what the generator asked for.

The recorded planes are OpenJPEG's, so the bars come from there: exact for 5/3 (full, reduced and
layer-limited decodes), and for 9/7 the bound measured over the corpus when it was generated
(meta "oracle_maxabs_97", DESIGN.md §4: 0).  tests/test_gpu_opj_streams.py holds the engine to
the same recording.
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import grok_amd as G
import j2k_markers as M
import opj_cases as OC
import openjpeg as J
import oracle as O
from conftest import GOLDEN

FX = OC.load()
IDS = [f.name for f in FX]
PROGS = ["LRCP", "RLCP", "RPCL", "PCRL", "CPRL"]
needs_opj = pytest.mark.skipif(not J.available(), reason="libopenjp2 (Pillow) not installed")


def _oracle(cs, reduce=0, layers=0):
    O.set_decode_reduce(reduce)
    O.set_decode_layers(layers)
    try:
        return OC.planes_of(O.decode(cs)[0])
    finally:
        O.set_decode_reduce(0)
        O.set_decode_layers(0)


def test_corpus_conditions():
    """Sizes the corpus was promised to keep, and the coding features it has to contain."""
    sizes = [os.path.getsize(f.path) for f in FX]
    assert len(FX) >= 60 and max(sizes) < 100 * 1000 and sum(sizes) < 2 * 1000 * 1000
    assert all(max(f.expect["w"], f.expect["h"]) <= 200 for f in FX)
    assert len({f.meta["opj_version"] for f in FX}) == 1
    e = {f.name: f.expect for f in FX}
    by = lambda pred: [n for n, x in e.items() if pred(x)]
    for bit in (1, 2, 4, 8, 16, 32):   # each mode switch alone, and with truncated layers
        assert by(lambda x: x["mode"] == bit and x["layers"] == 1) and by(lambda x: x["mode"] == bit and x["layers"] > 1)
    assert by(lambda x: x["mode"] == 63) and by(lambda x: x["mode"] == 5) and by(lambda x: x["mode"] == 17)
    assert by(lambda x: x["mode"] & 1 and x["irreversible"] and x["layers"] > 1)
    assert by(lambda x: x["sop"] and x["eph"] and x["tiles"] and x["layers"] > 1)
    assert {tuple(map(tuple, x["sub"])) for x in e.values()} >= {((1, 1), (2, 2), (2, 2)), ((1, 1), (2, 1), (2, 1))}
    assert by(lambda x: x["comps"] == 3 and x["irreversible"] and not x["mct"])
    assert by(lambda x: x["comps"] == 1 and x["prec"] == 16 and x["signed"])
    assert by(lambda x: (x["w"], x["h"]) == (1, 1))
    assert by(lambda x: x["tiles"] and 1 <= x["w"] % x["tiles"][0] <= 3 and 1 <= x["h"] % x["tiles"][1] <= 3)
    assert {x["prog"] for x in e.values()} == set(PROGS)
    assert sum(f.meta["image"]["noise"] for f in FX) == 2
    assert sum(bool(f.meta["fields"].get("cinema")) for f in FX) == 2
    assert [f.name for f in FX if f.meta["fields"].get("roi") and f.layered]


@pytest.mark.parametrize("f", FX, ids=IDS)
def test_oracle_matches_recording(f):
    bound = 0 if f.lossless else f.meta["oracle_maxabs_97"]
    assert bound == 0   # (what the generator measured; a larger figure would be stated in DESIGN.md §4)
    assert OC.maxabs(_oracle(f.cs), f.planes) is not None and OC.maxabs(_oracle(f.cs), f.planes) <= bound
    for tag, kw in (("r1", dict(reduce=1)), ("r2", dict(reduce=2)), ("l1", dict(layers=1))):
        if tag in f.limited:
            d = OC.maxabs(_oracle(f.cs, **kw), f.limited[tag])
            assert d is not None and d <= bound, (tag, d)


@pytest.mark.parametrize("f", [f for f in FX if f.limited], ids=[f.name for f in FX if f.limited])
def test_limited_recordings_are_limited(f):
    """cp_reduce / cp_layer took effect when the fixture was recorded (they are addressed by offset
    in opj_dparameters_t): reduced planes are ceil(x / 2^n) of the component's canvas edges, and the
    one-layer decode of a layered stream is not the full decode."""
    cd = lambda a, b: -(-a // b)
    e = f.expect
    for n in (1, 2):
        for (dx, dy), p in zip(e["sub"], f.limited["r%d" % n]):
            x0, x1 = cd(e["x0"], dx), cd(e["x0"] + e["w"], dx)
            y0, y1 = cd(e["y0"], dy), cd(e["y0"] + e["h"], dy)
            assert p.shape == (cd(y1, 1 << n) - cd(y0, 1 << n), cd(x1, 1 << n) - cd(x0, 1 << n))
    same = OC.maxabs(f.limited["l1"], f.planes) == 0
    assert same == (not f.layered)


@needs_opj
@pytest.mark.parametrize("f", FX, ids=IDS)
def test_fixture_integrity(f):
    """A fresh OpenJPEG decode of the committed bytes is the committed recording."""
    if f.meta["reference"] == "source":   # (OpenJPEG's decoder loses this stream: DESIGN.md §7)
        gen = _generator()
        case = next(c for c in gen.CASES if c["name"] == f.name)
        assert OC.maxabs(gen.image(case), f.planes) == 0
        return
    assert OC.maxabs([p for _, _, p in J.decode(f.cs)], f.planes) == 0
    for tag, kw in (("r1", dict(reduce=1)), ("r2", dict(reduce=2)), ("l1", dict(layers=1))):
        if tag in f.limited:
            assert OC.maxabs([p for _, _, p in J.decode(f.cs, **kw)], f.limited[tag]) == 0, tag


def _generator():
    spec = importlib.util.spec_from_file_location("make_opj_fixtures", os.path.join(GOLDEN, "make_opj_fixtures.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@needs_opj
def test_generator_reproduces_the_corpus():
    """The generator's cases are the committed files, and the same OpenJPEG writes the same bytes."""
    if J.encoder_params() is None:
        pytest.skip("opj_cparameters_t layout not recognised")
    if J.version() != FX[0].meta["opj_version"]:
        pytest.skip("fixtures were written by OpenJPEG %s" % FX[0].meta["opj_version"])
    gen = _generator()
    assert sorted(c["name"] for c in gen.CASES) == sorted(IDS)
    by_name = {f.name: f for f in FX}
    for case in gen.CASES:
        cs, _, arrays = gen.build(case)
        f = by_name[case["name"]]
        assert cs == f.cs, case["name"]
        assert gen.expect(case) == {**f.expect, "sub": [tuple(d) for d in f.expect["sub"]]}, case["name"]


def _probe(cs):
    lib = G.load_library()
    b = np.frombuffer(cs, np.uint8)
    info, cp, msg = G.ImageInfo(), G.CParameters(), ctypes.create_string_buffer(256)
    rc = lib.gk_probe_header(b.ctypes.data, len(b), ctypes.byref(info), ctypes.byref(cp), msg, 256)
    assert rc == 0, msg.value
    return info, cp


def _tile_parts(cs):
    """[(tile, part, marker codes of the tile-part header)] of the SOT markers, walked through Psot."""
    _, i = M.main_markers(cs)
    out = []
    while cs[i:i + 2] == b"\xff\x90":
        codes, j = [], i + 12
        while cs[j:j + 2] != b"\xff\x93":
            codes.append(int.from_bytes(cs[j:j + 2], "big"))
            j += 2 + int.from_bytes(cs[j + 2:j + 4], "big")
        out.append((int.from_bytes(cs[i + 4:i + 6], "big"), cs[i + 10], codes))
        i += int.from_bytes(cs[i + 6:i + 10], "big")
    assert cs[i:i + 2] == b"\xff\xd9"
    return out


@pytest.mark.parametrize("f", FX, ids=IDS)
def test_header_probes(f):
    """gk_probe_header / gk_probe_components (host only) read from another encoder's markers what
    the generator asked that encoder for; this also pins the wrapper's parameter offsets."""
    e = f.expect
    info, cp = _probe(f.cs)
    assert (info.w, info.h, info.x0, info.y0, info.numcomps) == (e["w"], e["h"], e["x0"], e["y0"], e["comps"])
    assert (info.prec, bool(info.sgnd)) == (e["prec"], e["signed"])
    assert G.probe_components(f.cs, precision=True) == [(dx, dy, e["prec"], e["signed"]) for dx, dy in e["sub"]]
    assert cp.numresolution == e["numres"] and cp.numlayers == e["layers"]
    assert [cp.cblockw_init, cp.cblockh_init] == e["cblk"]
    assert cp.cblk_sty == e["mode"] and bool(cp.irreversible) == e["irreversible"]
    assert PROGS[cp.prog_order] == e["prog"] and bool(cp.mct) == e["mct"]
    assert cp.csty == (1 if e["precincts"] else 0) | (2 if e["sop"] else 0) | (4 if e["eph"] else 0)
    if e["tiles"]:
        assert cp.tile_size_on and [cp.t_width, cp.t_height] == e["tiles"] and [cp.tx0, cp.ty0] == e["tile_origin"]
    fields = f.meta["fields"]
    if fields.get("precincts"):
        n = len(fields["precincts"])
        assert [list(p) for p in zip(cp.prcw_init[:n], cp.prch_init[:n])] == [list(p) for p in fields["precincts"]]
    # what the probe does not report, from the markers: RGN, COM, TLM, PLT, cinema's tile parts
    marks, _ = M.main_markers(f.cs)
    codes = [m for _, m, _ in marks]
    if fields.get("roi"):
        assert M.body(f.cs, 0xff5e) == bytes([fields["roi"][0], 0, fields["roi"][1]])
    else:
        assert 0xff5e not in codes
    if fields.get("comment"):
        assert fields["comment"].encode() in [bytes(f.cs[o + 6:o + 2 + L]) for o, m, L in marks if m == 0xff64]
    assert (0xff55 in codes) == bool(fields.get("tlm") or fields.get("cinema"))
    parts = _tile_parts(f.cs)
    assert all((0xff58 in codes) == bool(fields.get("plt")) for _, _, codes in parts)
    if fields.get("cinema"):   # (Rsiz itself stays 0: OpenJPEG withdraws it from an image that is no DCI frame)
        assert len(parts) > 1 and {t for t, _, _ in parts} == {0}
