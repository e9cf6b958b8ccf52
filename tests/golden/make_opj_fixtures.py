"""Writes tests/golden/opj/*.npz: codestreams written by OpenJPEG's encoder (the libopenjp2 Pillow
ships, driven by tests/openjpeg.py) with OpenJPEG's own decode of each.  Run by hand where that
library is present; never needed at test time (tests/test_opj_streams.py,
tests/test_gpu_opj_streams.py read the files).

A fixture holds
  cs            the codestream bytes
  c0, c1, ...   OpenJPEG's full decode, one plane per component at its own size, narrowest dtype
  r1_c*, r2_c*  (marked cases) OpenJPEG's decode with cp_reduce 1 and 2
  l1_c*         (marked cases) OpenJPEG's decode with cp_layer 1
  meta          JSON: the image (synth_image arguments or "noise"), the encoder fields, what the
                header must report ("expect"), opj_version(), and for 9/7 the measured corpus bound
                of the oracle's decode against OpenJPEG's ("oracle_maxabs_97").

One stream (roi_bypass) is recorded with "reference": "source": OpenJPEG's decoder loses its own
lossless ROI + BYPASS streams, so the planes kept are the image that was coded.

Images: grok_amd.synth.synth_image and two uniform-noise cases, all seeded; sides <= 200.  Files are
written with fixed zip timestamps so that a rerun reproduces them byte for byte.
"""
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import openjpeg as J   # noqa: E402
import oracle as O   # noqa: E402
from grok_amd.synth import synth_image   # noqa: E402

OUT = os.path.join(HERE, "opj")
MAX_FILE, MAX_SET, MAX_SIDE = 100 * 1000, 2 * 1000 * 1000, 200

BYPASS, RESET, TERMALL, VSC, PTERM, SEGSYM = 1, 2, 4, 8, 16, 32
S420 = [(1, 1), (2, 2), (2, 2)]
S422 = [(1, 1), (2, 1), (2, 1)]
CINEMA_EXPECT = dict(numres=6, cblk=(32, 32), prog="CPRL", irreversible=True)


def C(name, h, w, c, bits, seed=3, signed=False, noise=False, sub=None, marked=False, reference="opj", **fields):
    return dict(name=name, h=h, w=w, c=c, bits=bits, seed=seed, signed=signed, noise=noise, sub=sub, marked=marked,
                reference=reference, fields=fields)


CASES = [
    # ---- the survey of the issue: plain coding styles
    C("rgb8_default", 72, 88, 3, 8, mct=True, marked=True),
    C("mono8", 61, 83, 1, 8, marked=True),
    C("mono16", 60, 75, 1, 16),
    C("rgb16", 40, 52, 3, 16, mct=True),
    C("rgba8", 50, 66, 4, 8, mct=True),
    C("rgb8_nomct", 64, 70, 3, 8),
    C("rgb8_97", 72, 88, 3, 8, mct=True, irreversible=True, marked=True),
    C("mono8_97", 77, 59, 1, 8, irreversible=True),
    C("rgb8_rates", 96, 112, 3, 8, mct=True, rates=[40, 20, 10, 0], marked=True),
    C("rgb8_rates_97", 96, 112, 3, 8, mct=True, irreversible=True, rates=[60, 30, 12], marked=True),
    C("rgb8_db", 80, 96, 3, 8, mct=True, dB=[30, 38, 0]),
    C("rgb8_db_97", 80, 96, 3, 8, mct=True, irreversible=True, dB=[28, 34, 42]),
    C("mono8_layers20", 128, 120, 1, 8, rates=[float(200 - 10 * i) for i in range(19)] + [0], marked=True),
    C("rgb8_tiles_odd", 70, 90, 3, 8, mct=True, tiles=(37, 29), numres=5, marked=True),
    C("rgb8_tiles_offset", 70, 90, 3, 8, mct=True, tiles=(40, 32), origin=(13, 9), tile_origin=(5, 3)),
    C("mono8_tiles_offset_97", 75, 85, 1, 8, irreversible=True, tiles=(33, 41), origin=(7, 11), tile_origin=(2, 6)),
    C("rgb8_rpcl", 70, 90, 3, 8, mct=True, prog="RPCL", tiles=(64, 48), rates=[30, 10, 0]),
    C("rgb8_pcrl", 70, 90, 3, 8, mct=True, prog="PCRL", tiles=(64, 48), rates=[30, 10, 0], precincts=[(32, 32)]),
    C("rgb8_cprl", 70, 90, 3, 8, mct=True, prog="CPRL", rates=[30, 10, 0], precincts=[(64, 64), (32, 32)]),
    C("rgb8_rlcp", 70, 90, 3, 8, mct=True, prog="RLCP", rates=[30, 10, 0]),
    C("rgb8_prc_lt_cblk", 80, 100, 3, 8, mct=True, precincts=[(32, 32)], numres=5),
    C("mono8_cblk4", 40, 44, 1, 8, cblk=(4, 4), numres=3),
    C("mono8_cblk1024x4", 24, 200, 1, 8, cblk=(1024, 4), numres=3),
    C("rgb8_plt", 70, 90, 3, 8, mct=True, plt=True, tiles=(48, 48), rates=[20, 0]),
    C("rgb8_tlm", 70, 90, 3, 8, mct=True, tlm=True, tiles=(48, 48)),
    C("rgb8_cinema2k", 54, 100, 3, 8, mct=True, cinema="cinema2k"),
    C("rgb12_cinema4k", 54, 100, 3, 12, mct=True, cinema="cinema4k"),
    C("rgb8_com", 40, 48, 3, 8, mct=True, comment="written by another encoder"),
    # ---- every mode switch alone, all six, BYPASS with TERMALL and with PTERM
    C("mono8_bypass", 70, 90, 1, 8, mode=BYPASS),
    C("mono8_reset", 70, 90, 1, 8, mode=RESET),
    C("mono8_termall", 70, 90, 1, 8, mode=TERMALL),
    C("mono8_vsc", 70, 90, 1, 8, mode=VSC),
    C("mono8_pterm", 70, 90, 1, 8, mode=PTERM),
    C("mono8_segsym", 70, 90, 1, 8, mode=SEGSYM),
    C("rgb8_mode63", 70, 90, 3, 8, mct=True, mode=63),
    C("mono8_bypass_termall", 70, 90, 1, 8, mode=BYPASS | TERMALL),
    C("mono8_bypass_pterm", 70, 90, 1, 8, mode=BYPASS | PTERM),
    C("rgb8_sop_eph", 70, 90, 3, 8, mct=True, sop=True, eph=True),
    C("rgb8_roi7", 70, 90, 3, 8, roi=(1, 7)),
    C("rgb12", 60, 76, 3, 12, mct=True),
    C("rgb12_signed", 60, 76, 3, 12, signed=True, mct=True),
    C("rgb10_97", 60, 76, 3, 10, mct=True, irreversible=True),
    C("yuv420", 66, 86, 3, 8, sub=S420, marked=True),
    # ---- combinations
    C("mono8_layers_bypass", 90, 110, 1, 8, mode=BYPASS, rates=[30, 10, 0], marked=True),
    C("mono8_layers_reset", 90, 110, 1, 8, mode=RESET, rates=[30, 10, 4]),
    C("mono8_layers_termall", 90, 110, 1, 8, mode=TERMALL, rates=[30, 10, 4]),
    C("mono8_layers_vsc", 90, 110, 1, 8, mode=VSC, rates=[30, 10, 4]),
    C("mono8_layers_pterm", 90, 110, 1, 8, mode=PTERM, rates=[30, 10, 4]),
    C("mono8_layers_segsym", 90, 110, 1, 8, mode=SEGSYM, rates=[30, 10, 4]),
    C("rgb8_layers_mode63_97", 80, 96, 3, 8, mct=True, irreversible=True, mode=63, rates=[40, 15, 6]),
    C("rgb8_bypass_rates_97", 80, 96, 3, 8, mct=True, irreversible=True, mode=BYPASS, rates=[40, 15, 6]),
    C("rgb8_roi_layers", 80, 96, 3, 8, roi=(0, 9), rates=[30, 10, 0], marked=True),
    C("rgb8_roi_layers_97", 80, 96, 3, 8, mct=True, irreversible=True, roi=(2, 11), rates=[30, 10]),
    C("rgb8_sop_eph_tiles_layers", 70, 90, 3, 8, mct=True, sop=True, eph=True, tiles=(40, 40), rates=[30, 10, 0]),
    C("yuv422", 66, 86, 3, 8, sub=S422),
    C("yuv420_97_tiles", 64, 96, 3, 8, sub=S420, irreversible=True, tiles=(48, 32), rates=[20, 5]),
    C("rgb8_97_nomct", 64, 70, 3, 8, irreversible=True),
    C("mono16_signed", 60, 75, 1, 16, signed=True),
    C("mono12_signed_97", 60, 75, 1, 12, signed=True, irreversible=True),
    C("mono8_1x1", 1, 1, 1, 8, numres=1),
    C("rgb8_tiles_thin", 66, 67, 3, 8, mct=True, tiles=(32, 32), numres=4),
    C("mono8_tiles_thin_97", 65, 97, 1, 8, irreversible=True, tiles=(32, 32), numres=3),
    C("mono8_noise", 64, 72, 1, 8, noise=True, seed=5),
    C("rgb12_noise_layers", 48, 56, 3, 12, noise=True, seed=6, mct=True, rates=[8, 3, 0]),
    C("rgb8_roi_bypass", 70, 90, 3, 8, roi=(1, 7), mode=BYPASS, reference="source"),
]


def image(case):
    h, w, c, bits = case["h"], case["w"], case["c"], case["bits"]
    if case["noise"]:
        img = np.random.default_rng(case["seed"]).integers(0, 1 << bits, (c, h, w)).astype(np.int32)
    else:
        img = synth_image(h, w, c, bits, case["seed"]).astype(np.int32)
    if case["signed"]:
        img -= 1 << (bits - 1)
    if case["sub"]:
        return [np.ascontiguousarray(img[k][::dy, ::dx]) for k, (dx, dy) in enumerate(case["sub"])]
    return img


def narrow(a):
    lo, hi = int(a.min()), int(a.max())
    for dt in (np.uint8, np.int8, np.uint16, np.int16):
        i = np.iinfo(dt)
        if i.min <= lo and hi <= i.max:
            return a.astype(dt)
    return a.astype(np.int32)


def expect(case):
    """What the stream's header must say: the fields asked for, or the profile's own for cinema."""
    f = dict(numres=6, cblk=(64, 64), mode=0, irreversible=False, prog="LRCP", mct=False, sop=False, eph=False,
             origin=(0, 0), tile_origin=(0, 0), tiles=None, precincts=None, roi=None)
    f.update(case["fields"])
    if f.get("cinema"):
        f.update(CINEMA_EXPECT)
    layers = f.get("rates") or f.get("dB") or [0]
    x0, y0 = f["origin"]
    return dict(w=case["w"], h=case["h"], x0=x0, y0=y0, comps=case["c"], prec=case["bits"], signed=case["signed"],
                sub=case["sub"] or [(1, 1)] * case["c"], numres=f["numres"], cblk=list(f["cblk"]), mode=f["mode"],
                irreversible=f["irreversible"], prog=f["prog"], layers=len(layers), mct=bool(f["mct"]),
                sop=bool(f["sop"]), eph=bool(f["eph"]), precincts=bool(f["precincts"]) or bool(f.get("cinema")),
                tiles=list(f["tiles"]) if f["tiles"] else None, tile_origin=list(f["tile_origin"]))


def write_npz(path, arrays):
    """An .npz that np.load reads, with fixed timestamps and order (np.savez stamps the clock)."""
    with zipfile.ZipFile(path, "w") as z:
        for k, a in arrays.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(a), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, b.getvalue(), compresslevel=9)


def build(case):
    img = image(case)
    kw = dict(case["fields"])
    if case["sub"]:
        kw.update(subsampling=case["sub"], size=(case["w"], case["h"]))
    cs = J.encode(img, case["bits"], signed=case["signed"], **kw)
    arrays = {"cs": np.frombuffer(cs, np.uint8)}
    if case["reference"] == "source":
        full = [np.asarray(p) for p in img]
    else:
        full = [p for _, _, p in J.decode(cs)]
    for k, p in enumerate(full):
        arrays["c%d" % k] = narrow(p)
    if case["marked"]:
        for tag, dkw in (("r1", dict(reduce=1)), ("r2", dict(reduce=2)), ("l1", dict(layers=1))):
            for k, (_, _, p) in enumerate(J.decode(cs, **dkw)):
                arrays["%s_c%d" % (tag, k)] = narrow(p)
    return cs, full, arrays


def oracle_diff(cs, arrays, tag="", reduce=0, layers=0):
    """Largest difference of the oracle's decode from the planes recorded under `tag`."""
    O.set_decode_reduce(reduce)
    O.set_decode_layers(layers)
    try:
        got, _ = O.decode(cs)
    finally:
        O.set_decode_reduce(0)
        O.set_decode_layers(0)
    d = 0
    for k, g in enumerate(got):
        want = arrays[tag + "c%d" % k]
        assert g.shape == want.shape, (tag, k, g.shape, want.shape)
        d = max(d, int(np.abs(g.astype(np.int64) - want).max()))
    return d


def main():
    assert J.available() and J.encoder_params() is not None, "libopenjp2 with the expected parameter layout needed"
    os.makedirs(OUT, exist_ok=True)
    assert len({c["name"] for c in CASES}) == len(CASES)
    built, bound97 = [], 0
    for case in CASES:
        assert max(case["h"], case["w"]) <= MAX_SIDE
        try:
            cs, full, arrays = build(case)
        except RuntimeError as e:
            raise RuntimeError("%s: %s" % (case["name"], e))
        d = oracle_diff(cs, arrays)
        if case["marked"]:
            d = max(d, oracle_diff(cs, arrays, "r1_", reduce=1), oracle_diff(cs, arrays, "r2_", reduce=2),
                    oracle_diff(cs, arrays, "l1_", layers=1))
        if case["fields"].get("irreversible") or case["fields"].get("cinema"):
            bound97 = max(bound97, d)
        else:
            assert d == 0, (case["name"], d)
        built.append((case, arrays))
    total = 0
    for case, arrays in built:
        meta = dict(name=case["name"], image={k: case[k] for k in ("h", "w", "c", "bits", "seed", "signed", "noise")},
                    subsampling=case["sub"], marked=case["marked"], reference=case["reference"],
                    fields=case["fields"], expect=expect(case), opj_version=J.version())
        if meta["expect"]["irreversible"]:
            meta["oracle_maxabs_97"] = bound97
        arrays["meta"] = np.array(json.dumps(meta, sort_keys=True))
        path = os.path.join(OUT, case["name"] + ".npz")
        write_npz(path, arrays)
        n = os.path.getsize(path)
        assert n < MAX_FILE, (case["name"], n)
        total += n
        print("%-28s cs %6d  file %6d" % (case["name"], arrays["cs"].size, n))
    assert total < MAX_SET, total
    print("%d fixtures, %d bytes; oracle vs OpenJPEG 9/7 max-abs %d" % (len(built), total, bound97))


if __name__ == "__main__":
    main()
