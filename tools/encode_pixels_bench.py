"""Cost of the input stage of an encode from packed pixels (k_unpixels, gk_unpixels.hip) beside what
a caller does without it, on device-resident 8192 x 8192 RGB images of grok_amd.synth.synth_image.

  python tools/encode_pixels_bench.py compare [SIZE [ROUNDS]]
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/encode_pixels_bench.py profile
  python tools/encode_pixels_bench.py summarise OUT/**/run_kernel_trace.csv [SIZE]

`compare` times two cases, alternating A and B in one process after a warm-up of both, every run
between two host clock reads with a device synchronise inside, and prints one JSON line per case
with every time, the median and the range (max - min) of each side:
  rgb8   (H, W, 3) u8 tensor             A: permute(2, 0, 1).contiguous(), then encode (planar)
  rgb16  (H, W, 3) int16 tensor, prec 12 B: encode_pixels
The codestreams of A and B are compared byte for byte first.  The new path is `within` the old
one's noise when B's median is not above A's median by more than A's own range.
`profile` runs B of both cases a few times for a kernel trace; `summarise` prints k_unpixels's own
time per template instance, its algorithmic bytes (2 * es * C per pixel: every sample read once
and written once) over that time, and the share of the HBM peak (8 TB/s, MI355X)."""
import csv
import json
import os
import re
import statistics
import sys
import time

SIZE = 8192
ROUNDS = 6
HBM_PEAK = 8.0e12
TYPE_BYTES = {"unsigned char": 1, "unsigned short": 2, "unsigned int": 4}


def _setup():
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import grok_amd as G
    from grok_amd.synth import synth_image
    return torch, G, synth_image, G.Engine(0)


def _case(torch, G, synth_image, eng, size, prec):
    """(A, B, out): callables that encode the case's (H, W, 3) device tensor into `out`."""
    import numpy as np
    dt = np.uint8 if prec <= 8 else np.int16
    pix = torch.from_numpy(np.ascontiguousarray(np.moveaxis(synth_image(size, size, 3, prec, 1), 0, 2)).astype(dt)).cuda()
    out = torch.empty(size * size * 3 * 2, dtype=torch.uint8, device="cuda")
    p = G.default_params(numresolution=6)

    def a():
        return eng.encode(pix.permute(2, 0, 1).contiguous(), prec, params=p, out=out)

    def b():
        return eng.encode_pixels(pix, prec, params=p, out=out)
    return a, b, out


def _timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(v):
    return dict(ms=[round(x, 3) for x in v], median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3),
                max_ms=round(max(v), 3), range_ms=round(max(v) - min(v), 3))


def compare(size=SIZE, rounds=ROUNDS):
    torch, G, synth_image, eng = _setup()
    for name, prec in (("rgb8", 8), ("rgb16", 12)):
        a, b, out = _case(torch, G, synth_image, eng, size, prec)
        na = a()
        ref = out[:na].clone()
        nb = b()
        assert na == nb and torch.equal(ref, out[:nb]), "A and B differ"
        for _ in range(2):
            a()
            b()
        ta, tb = [], []
        for _ in range(rounds):
            ta.append(_timed(torch, a))
            tb.append(_timed(torch, b))
        sa, sb = _stats(ta), _stats(tb)
        print(json.dumps(dict(case=name, size=size, prec=prec, stream_bytes=na, A_permute_encode=sa, B_encode_pixels=sb,
                              within=sb["median_ms"] <= sa["median_ms"] + sa["range_ms"])), flush=True)
    eng.close()


def profile(size=SIZE, runs=6):
    torch, G, synth_image, eng = _setup()
    for prec in (8, 12):
        _, b, _ = _case(torch, G, synth_image, eng, size, prec)
        for _ in range(runs):
            b()
        torch.cuda.synchronize()
    eng.close()


def summarise(path, size=SIZE):
    npix = size * size
    groups = {}
    for r in csv.DictReader(open(path)):
        m = re.search(r"k_unpixels<([^<>]*)>", r["Kernel_Name"])
        if not m:
            continue
        args = [a.strip() for a in m.group(1).split(",")]
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        groups.setdefault(tuple(args), []).append(us)
    for args, t in sorted(groups.items()):
        c = int(re.sub(r"\D", "", args[1]))
        nbytes = 2 * TYPE_BYTES[args[0]] * c * npix
        med = statistics.median(t)
        rate = nbytes / (med * 1e-6)
        print(json.dumps(dict(kernel="k_unpixels<%s>" % ", ".join(args), launches=len(t), min_us=round(min(t), 1),
                              median_us=round(med, 1), max_us=round(max(t), 1), bytes=nbytes,
                              TB_per_s=round(rate / 1e12, 3), hbm_peak_share=round(rate / HBM_PEAK, 3))), flush=True)


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else "compare"
    if cmd == "summarise":
        summarise(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else SIZE)
    else:
        {"compare": compare, "profile": profile}[cmd](*(int(a) for a in sys.argv[2:]))
