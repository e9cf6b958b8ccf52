"""Cost of the render stage (gk_set_decode_render: k_render in place of k_view) and of the levels
call (gk_decode_levels: k_levels) beside the nearest path the engine had before them, on one
device-resident 16-bit grey 8192 x 8192 stream (uniform noise, 5/3 lossless, 6 resolutions, one
tile) viewed whole at 1024 x 1024 (reduce 3, equal sizes: the copy branch) and at 1000 x 1000 (the
area average).

  python tools/render_bench.py [RUNS]

Every run lies between two host clock reads with a device synchronise inside, after a warm-up of
every case; the cases alternate run by run in one process.  One JSON line per size with the
median and spread (min, max, inter-quartile range) of each case and the decoder's stage times
(gk_get_timings; the view, render and levels passes are counted in mct_ms):
  p8S:     set_decode_precision("8S"), decode_view into a device (h, w, 1) u8 tensor: the existing
           way from 16 bits to 8; it reads the same source and writes the same bytes
  window:  set_decode_render("window", [(0, 65535)]), decode_view into the same tensor
  blend:   set_decode_render("blend", ..., tints=[(255, 128, 0)]), decode_view into (h, w, 3) u8
  levels:  Engine.levels(bins=4096, origin=0, shift=4) on the noise: one call, no pixels written
  levels_const: the same on a constant image of the same size: every increment of a block falls on
           one LDS counter, the worst case; `const_over_noise` is the ratio of the two medians
A library named by GROK_AMD_LIB that predates the render calls runs the p8S case alone (the parent
commit's side of the comparison)."""
import json
import os
import statistics
import sys
import time

FIELDS = ("t2_ms", "t1_ms", "dwt_ms", "mct_ms", "total_ms")


def _stats(v):
    q = statistics.quantiles(v, n=4)
    return dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3),
                iqr_ms=round(q[2] - q[0], 3), q1_ms=round(q[0], 3), q3_ms=round(q[2], 3), runs=len(v))


def main(runs=16):
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import grok_amd as G
    eng = G.Engine(0)
    new = hasattr(eng.lib, "gk_set_decode_render")
    size = 8192
    gen = torch.Generator(device="cuda").manual_seed(10)

    def stream(img):
        buf = torch.empty(size * size * 2 * 2, dtype=torch.uint8, device="cuda")
        n = eng.encode(img, 16, params=G.default_params(), out=buf)
        return buf[:n].clone(), n

    f, n = stream(torch.randint(0, 65536, (1, size, size), dtype=torch.int32, device="cuda", generator=gen))
    fc, nc = stream(torch.full((1, size, size), 1234, dtype=torch.int32, device="cuda")) if new else (None, 0)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        t = eng.timings()
        return ms, [getattr(t, k) for k in FIELDS]

    for ow, oh in ((1024, 1024), (1000, 1000)):
        out1 = torch.empty((oh, ow, 1), dtype=torch.uint8, device="cuda")
        out3 = torch.empty((oh, ow, 3), dtype=torch.uint8, device="cuda")

        def p8s():
            eng.set_decode_precision("8S")
            try:
                eng.decode_view(f, size=(ow, oh), out=out1, length=n)
            finally:
                eng.set_decode_precision(None)

        def window():
            eng.set_decode_render("window", [(0, 65535)])
            try:
                eng.decode_view(f, size=(ow, oh), out=out1, length=n)
            finally:
                eng.set_decode_render(None)

        def blend():
            eng.set_decode_render("blend", [(0, 65535)], tints=[(255, 128, 0)])
            try:
                eng.decode_view(f, size=(ow, oh), out=out3, length=n)
            finally:
                eng.set_decode_render(None)

        cases = dict(p8S=p8s)
        if new:
            cases.update(window=window, blend=blend,
                         levels=lambda: eng.levels(f, size=(ow, oh), bins=4096, origin=0, shift=4, length=n),
                         levels_const=lambda: eng.levels(fc, size=(ow, oh), bins=4096, origin=0, shift=4, length=nc))
        for _ in range(2):
            for fn in cases.values():
                fn()
        vr = eng.view_result
        times = {k: [] for k in cases}
        stages = {k: [] for k in cases}
        for _ in range(runs):
            for k, fn in cases.items():
                ms, st = timed(fn)
                times[k].append(ms)
                stages[k].append(st)
        med = lambda rows: dict(zip(FIELDS, [round(statistics.median(c), 3) for c in zip(*rows)]))
        line = dict(out=[ow, oh], reduce=vr.reduce, source=[vr.rx1 - vr.rx0, vr.ry1 - vr.ry0], stream_bytes=n,
                    library="this tree" if not os.environ.get("GROK_AMD_LIB") else os.environ["GROK_AMD_LIB"])
        for k in cases:
            line[k] = _stats(times[k])
            line[k + "_stages"] = med(stages[k])
        if new:
            line["const_over_noise"] = round(line["levels_const"]["median_ms"] / line["levels"]["median_ms"], 3)
            line["const_over_noise_pass"] = round(line["levels_const_stages"]["mct_ms"] / max(line["levels_stages"]["mct_ms"], 1e-6), 3)
            a = line["p8S"]
            for k in ("window", "blend"):
                line[k + "_inside_p8S_iqr"] = a["q1_ms"] <= line[k]["median_ms"] <= a["q3_ms"]
        print(json.dumps(line), flush=True)
    eng.close()


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:]))
