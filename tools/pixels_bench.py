"""Cost of the output stage (k_pixels, gk_pixels.hip) beside what a user does without it, on a
device-resident lossless 8192 x 8192 RGB stream of grok_amd.synth.synth_image.

  python tools/pixels_bench.py compare [SIZE [RUNS]]
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/pixels_bench.py profile
  python tools/pixels_bench.py summarise OUT/**/run_kernel_trace.csv [SIZE]

`compare` times two pairs, alternating A and B in one process after a warm-up of both, every run
between two host clock reads with a device synchronise inside, and prints one JSON line per pair
with the median and the spread (min, max, inter-quartile range) of each side:
  rgb8      A: planar u8 decode into a device tensor, then permute(1, 2, 0).contiguous()
            B: decode_pixels into a device (H, W, 3) u8 tensor
  rgb12_8S  A: planar 16-bit decode, then torch's integer arithmetic (>> 4, to u8) and the permute
            B: decode_pixels under set_decode_precision("8S") into a device u8 tensor
It also prints the decoder's stage times (gk_get_timings) of both sides.
`profile` runs B of both pairs a few times for a kernel trace; `summarise` prints k_pixels's own
time per template instance, its algorithmic bytes (es_in * C + es_out * C per pixel) over that
time, and the share of the HBM peak (8 TB/s, MI355X)."""
import csv
import json
import os
import re
import statistics
import sys
import time

SIZE = 8192
RUNS = 24
HBM_PEAK = 8.0e12
TYPE_BYTES = {"unsigned char": 1, "unsigned short": 2, "int": 4}


def _setup():
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import grok_amd as G
    from grok_amd.synth import synth_image
    return torch, G, synth_image, G.Engine(0)


def _stream(torch, G, synth_image, eng, size, prec):
    import numpy as np
    img = torch.from_numpy(synth_image(size, size, 3, prec, 1).astype(np.int32)).cuda()
    buf = torch.empty(size * size * 3 * 2, dtype=torch.uint8, device="cuda")
    n = eng.encode(img, prec, params=G.default_params(numresolution=6), out=buf)
    return buf[:n].clone(), n


def _sides(torch, eng, size, prec, f, n):
    """(A, B, precision list of B): callables that return the packed u8 device tensor."""
    pix = torch.empty((size, size, 3), dtype=torch.uint8, device="cuda")
    if prec == 8:
        planes = torch.empty((3, size, size), dtype=torch.uint8, device="cuda")

        def a():
            eng.decode(f, length=n, out=planes)
            return planes.permute(1, 2, 0).contiguous()
        spec = None
    else:
        planes = torch.empty((3, size, size), dtype=torch.int16, device="cuda")

        def a():   # (12-bit samples are positive in int16: the shift is scale_component's division)
            eng.decode(f, length=n, out=planes)
            return (planes >> (prec - 8)).to(torch.uint8).permute(1, 2, 0).contiguous()
        spec = "8S"

    def b():
        eng.decode_pixels(f, length=n, out=pix)
        return pix
    return a, b, spec


def _timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(v):
    q = statistics.quantiles(v, n=4)
    return dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3),
                iqr_ms=round(q[2] - q[0], 3), runs=len(v))


def compare(size=SIZE, runs=RUNS):
    torch, G, synth_image, eng = _setup()
    fields = ("t2_ms", "t1_ms", "dwt_ms", "mct_ms", "total_ms")
    for name, prec in (("rgb8", 8), ("rgb12_8S", 12)):
        f, n = _stream(torch, G, synth_image, eng, size, prec)
        a, b, spec = _sides(torch, eng, size, prec, f, n)

        def run_b():
            eng.set_decode_precision(spec)
            try:
                return b()
            finally:
                eng.set_decode_precision(None)
        assert torch.equal(a(), run_b()), "A and B differ"
        for _ in range(2):
            a()
            run_b()
        ta, tb, sa, sb = [], [], [], []
        for _ in range(runs):
            ta.append(_timed(torch, a))
            t = eng.timings()
            sa.append([getattr(t, k) for k in fields])
            tb.append(_timed(torch, run_b))
            t = eng.timings()
            sb.append([getattr(t, k) for k in fields])
        med = lambda rows: dict(zip(fields, [round(statistics.median(c), 3) for c in zip(*rows)]))
        print(json.dumps(dict(case=name, size=size, stream_bytes=n, A=_stats(ta), B=_stats(tb), A_stages=med(sa),
                              B_stages=med(sb))), flush=True)
    eng.close()


def profile(size=SIZE, runs=6):
    torch, G, synth_image, eng = _setup()
    for prec in (8, 12):
        f, n = _stream(torch, G, synth_image, eng, size, prec)
        _, b, spec = _sides(torch, eng, size, prec, f, n)
        eng.set_decode_precision(spec)
        for _ in range(runs):
            b()
        torch.cuda.synchronize()
        eng.set_decode_precision(None)
    eng.close()


def summarise(path, size=SIZE):
    npix = size * size
    groups = {}
    for r in csv.DictReader(open(path)):
        m = re.search(r"k_pixels<([^<>]*)>", r["Kernel_Name"])
        if not m:
            continue
        args = [a.strip() for a in m.group(1).split(",")]
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        groups.setdefault(tuple(args), []).append(us)
    for args, t in sorted(groups.items()):
        c = int(re.sub(r"\D", "", args[2]))
        nbytes = (TYPE_BYTES[args[0]] + TYPE_BYTES[args[1]]) * c * npix
        med = statistics.median(t)
        rate = nbytes / (med * 1e-6)
        print(json.dumps(dict(kernel="k_pixels<%s>" % ", ".join(args), launches=len(t), min_us=round(min(t), 1),
                              median_us=round(med, 1), max_us=round(max(t), 1), bytes=nbytes,
                              TB_per_s=round(rate / 1e12, 3), hbm_peak_share=round(rate / HBM_PEAK, 3))), flush=True)


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else "compare"
    if cmd == "summarise":
        summarise(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else SIZE)
    else:
        {"compare": compare, "profile": profile}[cmd](*(int(a) for a in sys.argv[2:]))
