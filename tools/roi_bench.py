"""Cost of a shaped region of interest (Engine.set_encode_roi) on one device-resident SIZE x SIZE
RGB8 image of grok_amd.synth.synth_image, 5/3 with RCT, default coding: the plain encode, Grok's whole-component -ROI on
component 0 with the same shift (what maxshift costs without any mask), then a centred rectangular
region of 1/16 and of 1/2 of the image.

  python tools/roi_bench.py [SIZE [RUNS]]

All times are the engine's own HIP events (gk_timings): total_ms the whole call, t1_ms the block
coders with the mask kernels in front of them (t1_cm_ms up to the last context-modelling launch,
t1_coder_ms the last MQ launch), roi_ms the mask kernels alone (k_roi_fill and one
k_roi_level launch per decomposition level and tile class; gk_roi.hip).  One JSON line per case
(after a warm-up call): every run's total, the medians, the stream size, and the mask kernels'
algorithmic bytes (each level reads and writes one byte per sample of its input) with their
rate."""
import json
import os
import statistics
import sys


def main(size=8192, runs=3):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import grok_amd as G
    from grok_amd.synth import synth_image
    img = torch.from_numpy(synth_image(size, size, 3, 8, 1).astype(np.uint8)).cuda()
    out = torch.empty(size * size * 3 * 2, dtype=torch.uint8, device="cuda")
    p = G.default_params(numresolution=6)
    eng = G.Engine(0)
    e = size // 8
    h2 = int(size * 0.5 ** 0.5) // 2
    cases = [("plain", None), ("component -ROI c=0,U=11", "comp"), ("region 1/16", (size // 2 - e, size // 2 - e, size // 2 + e, size // 2 + e)),
             ("region 1/2", (size // 2 - h2, size // 2 - h2, size // 2 + h2, size // 2 + h2))]
    # bytes of the mask kernels: the fill writes the image once, level l reads and writes 4^-(l-1) of it
    mask_bytes = size * size * (1 + 2 * sum(0.25 ** l for l in range(5)))
    try:
        for name, rect in cases:
            comp = rect == "comp"
            rect = None if comp else rect
            pp = G.default_params(numresolution=6, roi=(0, 11)) if comp else p
            eng.set_encode_roi(rects=[rect] if rect else None)
            tot, t1, cm, mq, roi, n = [], [], [], [], [], 0
            for i in range(runs + 1):
                n = eng.encode(img, 8, params=pp, out=out)
                if i:
                    t = eng.timings()
                    tot.append(t.total_ms); t1.append(t.t1_ms); roi.append(t.roi_ms)
                    cm.append(t.t1_cm_ms); mq.append(t.t1_coder_ms)
            rec = dict(case=name, size=size, runs_total_ms=[round(v, 3) for v in tot],
                       total_ms=round(statistics.median(tot), 3), t1_ms=round(statistics.median(t1), 3),
                       t1_cm_ms=round(statistics.median(cm), 3), t1_coder_ms=round(statistics.median(mq), 3),
                       roi_ms=round(statistics.median(roi), 4), stream_bytes=n)
            if rect:
                rec["region_share"] = round((rect[2] - rect[0]) * (rect[3] - rect[1]) / size ** 2, 4)
                rec["mask_bytes"] = int(mask_bytes)
                rec["mask_TB_per_s"] = round(mask_bytes / (statistics.median(roi) * 1e-3) / 1e12, 3)
            print(json.dumps(rec), flush=True)
    finally:
        eng.set_encode_roi()
        eng.close()


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:]))
