"""Encode from packed pixels, without a GPU: the unpack kernels build for gfx950 without scratch or
LDS, and the entry point is exported and declared."""
import os
import re
import subprocess

import grok_amd as G
from conftest import ROOT


def test_kernel_builds_for_gfx950_without_scratch_or_lds(tmp_path):
    src = os.path.join(os.path.dirname(G.__file__), "csrc", "gk_unpixels.hip")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "gk_unpixels.out")],
                       capture_output=True, text=True, check=True)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    # 3 sample sizes x (C = 1..4 and the channel-at-a-time kernel)
    assert len(names) == 15 and sum("k_unpixels_any" in n for n in names) == 3
    assert len(scratch) == 15 and not any(scratch) and len(lds) == 15 and not any(lds)


def test_entry_points_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "grok_amd.h")).read()
    lib = G.load_library()
    for name in ("gk_encode_pixels", "gk_set_encode_colour", "gk_jp2_boxes"):
        assert name in G.EXPORTS and hasattr(lib, name)
        assert re.search(r"\bint %s\(" % name, header)
