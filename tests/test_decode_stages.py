"""The host stages of the decode core (gk_engine.cpp: tile_rect, blocks_needed, fill_table,
solo_split, lane_layout, output_rects) on small plans with generated packet state (CPU only: the
check program, tools/decode_stages_check.cpp, compiles the engine source and makes no GPU call).

The table fill must equal a plain serial fill byte for byte (16 tiles, one tile, BYPASS | TERMALL,
windows, a tile without a part); a window's needed blocks grow with the window; the solo split
and the lane layout keep their invariants for every lane count and plan; the output rectangles
have the sizes comp_dims gives the display stages.
"""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "grok_amd", "libgrok_amd.so")


@pytest.mark.skipif(shutil.which("hipcc") is None or not os.path.exists(LIB),
                    reason="needs hipcc and the built libgrok_amd.so")
def test_decode_stages(tmp_path):
    exe = str(tmp_path / "decode_stages_check")
    src = os.path.join(ROOT, "tools", "decode_stages_check.cpp")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-x", "hip", src, "-o", exe,
                           "-x", "none", LIB, "-Wl,-rpath," + os.path.dirname(LIB)],
                          cwd=os.path.join(ROOT, "tools"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "decode stages ok" in r.stdout
