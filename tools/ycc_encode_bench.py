"""Cost of the input stage of an encode under Engine.set_encode_convert (k_rgb_ycc, gk_rgbycc.hip)
beside the plain unpack (k_unpixels, gk_unpixels.hip) on one device-resident SIZE x SIZE RGB8 image
of grok_amd.synth.synth_image.

  python tools/ycc_encode_bench.py [SIZE [RUNS]]

The input stage is timed by the engine's own HIP events: gk_timings::total_ms spans the events in
front of the stage and behind the assembly, the other fields the stages after it, so the stage is
total_ms less their sum.  With device pixels it holds the one kernel and nothing else.  One JSON
line per case (after a warm-up call): every run, the median, the algorithmic bytes (every input
sample read once, every output sample written once) and their rate against the HBM peak."""
import json
import os
import statistics
import sys

HBM_PEAK = 8.0e12


def input_ms(t):
    return t.total_ms - (t.mct_ms + t.dwt_ms + t.t1_ms + t.t2_ms + t.assemble_ms)


def main(size=8192, runs=3):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import grok_amd as G
    from grok_amd.synth import synth_image
    pix = torch.from_numpy(np.ascontiguousarray(np.moveaxis(synth_image(size, size, 3, 8, 1), 0, 2)).astype(np.uint8)).cuda()
    out = torch.empty(size * size * 3 * 2, dtype=torch.uint8, device="cuda")
    p = G.default_params(numresolution=6)
    eng = G.Engine(0)
    npix = size * size
    # (case, conversion, bytes per pixel in + out)
    cases = [("k_unpixels<u8, 3>", None, 3 + 3), ("k_rgb_ycc<u8, 444, packed>", (1, 1), 3 + 3),
             ("k_rgb_ycc<u8, 420, packed>", (2, 2), 3 + 1.5)]
    try:
        for name, chroma, bpp in cases:
            eng.set_encode_convert(None if chroma is None else "sycc", chroma or (1, 1))
            ms = []
            for i in range(runs + 1):
                eng.encode_pixels(pix, 8, params=p, out=out)
                if i:
                    ms.append(input_ms(eng.timings()))
            med = statistics.median(ms)
            rate = bpp * npix / (med * 1e-3)
            print(json.dumps(dict(kernel=name, size=size, runs_ms=[round(v, 4) for v in ms], median_ms=round(med, 4),
                                  bytes=int(bpp * npix), TB_per_s=round(rate / 1e12, 3),
                                  hbm_peak_share=round(rate / HBM_PEAK, 3))), flush=True)
    finally:
        eng.set_encode_convert(None)
        eng.close()


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:]))
