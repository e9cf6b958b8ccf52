"""Cost of a view (gk_decode_view_pixels: the window decode at the chosen reduce level, then k_view)
beside decode_pixels of the same window at the same reduce level, on the device-resident C2 frame
of bench.py (8192 x 8192 8-bit RGB, 5/3 lossless + RCT, 6 resolutions, one tile).

  python tools/view_bench.py [RUNS]

Per case, A and B alternate in one process after a warm-up of both, every run between two host
clock reads with a device synchronise inside; one JSON line per case with the median and spread
(min, max, inter-quartile range) of each side, the reduce level, and the decoder's stage times
(gk_get_timings; the view pass and the output pass are both counted in mct_ms):
  A: set_decode_reduce(r), decode_pixels(window) into a device (rh, rw, 3) u8 tensor
  B: decode_view(region, size) into a device (out_h, out_w, 3) u8 tensor
B does everything A does (into the engine's int32 buffer) and then runs k_view, so B - A is the
added pass."""
import json
import os
import statistics
import sys
import time

CASES = (("whole_to_1024", None, (1024, 1024)), ("whole_to_1000", None, (1000, 1000)),
         ("region2048_to_512", (3000, 3000, 5048, 5048), (512, 512)),
         ("region2048_to_500", (3000, 3000, 5048, 5048), (500, 500)))
FIELDS = ("t2_ms", "t1_ms", "dwt_ms", "mct_ms", "total_ms")


def _stats(v):
    q = statistics.quantiles(v, n=4)
    return dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3),
                iqr_ms=round(q[2] - q[0], 3), runs=len(v))


def main(runs=16):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import grok_amd as G
    from grok_amd.synth import synth_image
    eng = G.Engine(0)
    size = 8192
    img = torch.from_numpy(synth_image(size, size, 3, 8, 10).astype(np.int32)).cuda()
    buf = torch.empty(size * size * 3 * 2, dtype=torch.uint8, device="cuda")
    n = eng.encode(img, 8, params=G.default_params(), out=buf)
    f = buf[:n].clone()
    del img, buf

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        t = eng.timings()
        return ms, [getattr(t, k) for k in FIELDS]

    for name, region, (ow, oh) in CASES:
        out_b = torch.empty((oh, ow, 3), dtype=torch.uint8, device="cuda")
        eng.decode_view(f, region=region, size=(ow, oh), out=out_b, length=n)
        vr = eng.view_result
        r, rw, rh = vr.reduce, vr.rx1 - vr.rx0, vr.ry1 - vr.ry0
        out_a = torch.empty((rh, rw, 3), dtype=torch.uint8, device="cuda")

        def a():
            eng.set_decode_reduce(r)
            try:
                eng.decode_pixels(f, length=n, out=out_a, window=region)
            finally:
                eng.set_decode_reduce(0)

        def b():
            eng.decode_view(f, region=region, size=(ow, oh), out=out_b, length=n)
        for _ in range(2):
            a()
            b()
        if (rw, rh) == (ow, oh):
            assert torch.equal(out_a, out_b), "equal sizes: the view is not a copy of A"
        ta, tb, sa, sb = [], [], [], []
        for _ in range(runs):
            ms, st = timed(a)
            ta.append(ms)
            sa.append(st)
            ms, st = timed(b)
            tb.append(ms)
            sb.append(st)
        med = lambda rows: dict(zip(FIELDS, [round(statistics.median(c), 3) for c in zip(*rows)]))
        print(json.dumps(dict(case=name, region=region, out=[ow, oh], reduce=r, source=[rw, rh], stream_bytes=n, A=_stats(ta),
                              B=_stats(tb), A_stages=med(sa), B_stages=med(sb))), flush=True)
    eng.close()


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:]))
