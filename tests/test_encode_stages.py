"""The host stages of the encode core (gk_engine.cpp: enc_range, range_blocks, weight_order,
chunk_cuts, bisect_notch, the two chain builders, layout_segments) on small plans with generated
T1 results (CPU only: the check program, tools/encode_stages_check.cpp, compiles the engine source
and makes no GPU call).

A tile range's blocks, rows and slots must equal a direct recomputation and its relocated blocks
lie inside their work planes; the weight order is a stable descending bucket sort; chunk cuts are
increasing multiples of 256; the notch search ends on an adjacent pair within its probe bound; the
serial and the by-band chain builder, and the serial and the per-packet layout, agree exactly; the
layout tiles the stream and reads every block's bytes from its slot; every stream is read back
through the engine's own reader (parse_header, the SOT walk, t2_parse_part): Psot, TLM and PLT
values, and per block its inclusion, passes, length and segment lengths.
"""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "grok_amd", "libgrok_amd.so")


@pytest.mark.skipif(shutil.which("hipcc") is None or not os.path.exists(LIB),
                    reason="needs hipcc and the built libgrok_amd.so")
def test_encode_stages(tmp_path):
    exe = str(tmp_path / "encode_stages_check")
    src = os.path.join(ROOT, "tools", "encode_stages_check.cpp")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-x", "hip", src, "-o", exe,
                           "-x", "none", LIB, "-Wl,-rpath," + os.path.dirname(LIB)],
                          cwd=os.path.join(ROOT, "tools"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "encode stages ok" in r.stdout
