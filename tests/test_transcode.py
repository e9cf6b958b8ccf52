"""Transcode Part-1 <-> HTJ2K, the part that needs no GPU: gk_probe_transcode gives every refusal
of gk_transcode from the headers and packet headers alone (tests/test_gpu_transcode.py runs the
transcodes).  Over the corpus of OpenJPEG-written streams, the 33 single-layer reversible streams
must be accepted for an HT target; every other stream is accepted or refused by one of the named
refusals of include/grok_amd.h."""
import ctypes
import os
import re

import numpy as np
import pytest

import grok_amd as G
import opj_cases as OC
from conftest import FIXTURES, ROOT

FX = OC.load()
MUST = [f for f in FX if f.expect["layers"] == 1 and not f.expect["irreversible"]]
REST = [f for f in FX if f not in MUST]
# what a refusal may say (include/grok_amd.h, gk_transcode)
NAMED = ("transcode: truncated code-block", "transcode: progression order changes (POC)",
         "transcode: a COC that changes", "transcode: a tile-part COD", "transcode: HT code-block with SigProp",
         "bit-planes in the", "transcode: the source is already coded", "Part-2 (ISO 15444-2)")


def probe(cs, target="ht"):
    """None when the bytes would transcode, else the refusal."""
    try:
        G.probe_transcode(cs, target)
    except ValueError as e:
        return str(e)
    return None


def test_entry_points_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "grok_amd.h")).read()
    lib = G.load_library()
    for name in ("gk_transcode", "gk_probe_transcode"):
        assert name in G.EXPORTS and hasattr(lib, name)
        assert re.search(r"\bint %s\(" % name, header)
    assert "gk_set_default_transcode" in G.EXPORTS and re.search(r"\bvoid gk_set_default_transcode\(", header)
    assert hasattr(G.Engine, "transcode")
    p = G.TranscodeParams(9, 9, 9, 9)
    lib.gk_set_default_transcode(ctypes.byref(p))
    assert (p.target, p.tlm, p.plt, p.com) == (G.GK_TRANSCODE_HT, 0, 0, 1)


def test_the_must_accept_set():
    names = [f.name for f in MUST]
    assert len(FX) == 65 and len(MUST) == 33 and names[0] == "mono16" and names[-1] == "yuv422"
    for n in ("mono8_bypass", "mono8_bypass_pterm", "mono8_bypass_termall", "rgb8_mode63", "mono8_cblk4", "mono8_cblk1024x4",
              "mono8_1x1", "rgba8", "yuv420", "yuv422", "rgb8_tlm", "rgb8_sop_eph", "rgb8_prc_lt_cblk", "rgb8_roi7",
              "rgb8_roi_bypass"):
        assert n in names, n


@pytest.mark.parametrize("f", MUST, ids=[f.name for f in MUST])
def test_single_layer_reversible_streams_are_accepted(f):
    assert probe(f.cs) is None


@pytest.mark.parametrize("f", REST, ids=[f.name for f in REST])
def test_every_other_stream_is_accepted_or_refused_by_name(f):
    why = probe(f.cs)
    assert why is None or any(n in why for n in NAMED), why


def test_a_truncated_block_is_named():
    f = next(x for x in FX if x.name == "rgb8_rates_97")
    why = probe(f.cs)
    m = re.match(r"transcode: truncated code-block \(tile (\d+), component (\d+), resolution (\d+), band (LL|HL|LH|HH), "
                 r"block (\d+): (\d+) of (\d+) passes\)$", why)
    assert m, why
    assert int(m.group(6)) < int(m.group(7)) and (int(m.group(7)) + 2) % 3 == 0


def test_roi_blocks_coded_down_to_the_shift_are_complete():
    """OpenJPEG stops an ROI component's blocks at the plane of the shift: a region coefficient has
    no bit below it, so nothing is missing (grok_amd.h).  Both RGN streams of the corpus do this."""
    for n in ("rgb8_roi7", "rgb8_roi_bypass"):
        f = next(x for x in FX if x.name == n)
        assert f.meta["fields"].get("roi") and probe(f.cs) is None


def test_source_already_in_the_target_coder():
    part1 = next(x for x in FX if x.name == "rgb8_default")
    assert "already coded with the target coder (Part-1)" in probe(part1.cs, "part1")
    ht = next(x for x in FIXTURES if x.ht)
    assert "already coded with the target coder (HTJ2K)" in probe(ht.cs, "ht")
    assert probe(ht.cs, "part1") is None


def test_poc_is_refused():
    f = next(x for x in FX if x.name == "rgb12_cinema4k")
    assert "POC" in probe(f.cs)


def test_bad_target():
    with pytest.raises(ValueError, match="target"):
        G.probe_transcode(MUST[0].cs, "jpeg")
    lib = G.load_library()
    b = np.frombuffer(MUST[0].cs, np.uint8)
    msg = ctypes.create_string_buffer(256)
    tp = G.TranscodeParams(7, 0, 0, 1)
    assert lib.gk_probe_transcode(b.ctypes.data, len(b), ctypes.byref(tp), msg, 256) == -1
    assert b"GK_TRANSCODE_HT or GK_TRANSCODE_PART1" in msg.value


def test_bytes_that_are_no_stream_give_the_readers_messages():
    f = MUST[0]
    assert probe(b"\x00" * 64) == "not a J2K codestream (no SOC)"
    assert probe(f.cs[:20]) in ("corrupt main header (marker length)", "incomplete main header")
    assert probe(f.cs[:2] + b"\xff\x52" + f.cs[4:]) is not None
    sot = f.cs.index(b"\xff\x90")
    assert probe(f.cs[:sot]) == "incomplete main header"
    assert probe(f.cs[:sot] + b"\xff\xd9") == "incomplete main header"


def test_without_a_device_the_engine_refuses_first():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: tests/test_gpu_transcode.py runs the transcodes")
    lib = G.load_library()
    assert not lib.gk_create(0)
    with pytest.raises(RuntimeError, match="no HIP device"):
        G.Engine(0)
    # the call itself, without an engine: an error code, no crash
    b = np.frombuffer(MUST[0].cs, np.uint8)
    out = np.empty(1 << 16, np.uint8)
    n = ctypes.c_size_t()
    assert lib.gk_transcode(None, b.ctypes.data, len(b), 0, None, out.ctypes.data, out.size, 0, ctypes.byref(n)) == -1
