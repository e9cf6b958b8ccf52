"""Cost of a view written as a float tensor (gk_decode_view_tensor: the window decode at the chosen
reduce level, then k_tensor) beside what the engine offered before it for the same result, on the
device-resident C2 frame of bench.py (8192 x 8192 8-bit RGB, 5/3 lossless + RCT, 6 resolutions, one
tile) viewed at 2048 x 2048 into a device (3, 2048, 2048) bfloat16 tensor with per-channel mean / std.

  python tools/tensor_bench.py [RUNS]

  new:    decode_tensor(size=(2048, 2048), mean=, std=, out=bf16 tensor)
  old:    decode_view(size=(2048, 2048), sample_bytes=0, out=int32 tensor), then the torch chain
          permute -> float -> mul -> add -> bfloat16, timed with torch events
  region: set_decode_reduce(2) + decode_pixels into an int32 tensor: what both do before their last
          pass (view_region), so mct_ms(new) - mct_ms(region) is the tensor pass's own time (its two
          events) and mct_ms(old) - mct_ms(region) is k_view<int32>'s.
The three alternate in one process after a warm-up of each; total_ms / mct_ms are gk_get_timings'
(device events, read after the call's synchronise).  One JSON line: the medians of RUNS, the
spread of the totals, and whether the two results hold the same bits."""
import json
import os
import statistics
import sys


def main(runs=20):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import grok_amd as G
    from grok_amd.synth import synth_image

    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    eng = G.Engine(0)
    cs = eng.encode(synth_image(8192, 8192, 3, 8, 10).astype(np.int32), 8, params=G.default_params())
    d, n = torch.from_numpy(np.frombuffer(cs, np.uint8).copy()).cuda(), len(cs)
    scale, bias = G._tensor_affine(mean, std, None, 8, False)
    ts, tb = torch.tensor(scale, device="cuda").view(3, 1, 1), torch.tensor(bias, device="cuda").view(3, 1, 1)
    out = torch.empty((3, 2048, 2048), dtype=torch.bfloat16, device="cuda")
    pix = torch.empty((2048, 2048, 3), dtype=torch.int32, device="cuda")
    base = torch.empty((2048, 2048, 3), dtype=torch.int32, device="cuda")

    def new():
        eng.decode_tensor(d, size=(2048, 2048), mean=mean, std=std, out=out, length=n)
        t = eng.timings()
        return t.total_ms, t.mct_ms

    def old():
        eng.decode_view(d, size=(2048, 2048), sample_bytes=0, out=pix, length=n)
        t = eng.timings()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = pix.permute(2, 0, 1).float().mul(ts).add(tb).bfloat16()
        e1.record()
        torch.cuda.synchronize()
        return t.total_ms, t.mct_ms, e0.elapsed_time(e1), y

    def region():
        eng.set_decode_reduce(2)
        try:
            eng.decode_pixels(d, length=n, out=base)
        finally:
            eng.set_decode_reduce(0)
        t = eng.timings()
        return t.total_ms, t.mct_ms

    new()
    y = old()[3]
    region()
    assert eng.view_result.reduce == 2
    same = bool((out.view(torch.int16) == y.view(torch.int16)).all())
    rn, ro, rb = [], [], []
    for _ in range(runs):
        rn.append(new())
        ro.append(old()[:3])
        rb.append(region())
    eng.close()
    med = lambda v: round(statistics.median(v), 4)
    span = lambda v: [round(min(v), 3), round(max(v), 3)]
    print(json.dumps({
        "runs": runs, "equal_bits": same, "stream_bytes": n,
        "new_total_ms": med([r[0] for r in rn]), "new_total_minmax": span([r[0] for r in rn]), "new_mct_ms": med([r[1] for r in rn]),
        "old_view_total_ms": med([r[0] for r in ro]), "old_view_mct_ms": med([r[1] for r in ro]), "old_chain_ms": med([r[2] for r in ro]),
        "old_total_plus_chain_ms": med([r[0] + r[2] for r in ro]), "old_total_plus_chain_minmax": span([r[0] + r[2] for r in ro]),
        "region_total_ms": med([r[0] for r in rb]), "region_mct_ms": med([r[1] for r in rb])}))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
