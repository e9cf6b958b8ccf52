"""Cost of the colour-management stage (GK_DISPLAY_ICC: k_icc_rgb, k_lab_rgb) beside k_ycc_rgb on
same-sized images, on device-resident streams and planes.

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/icc_bench.py run
  python tools/icc_bench.py summarise OUT/**/run_kernel_trace.csv

`run` decodes, REPS times each after one warm-up: an RGB image with a gamma-2.2 matrix profile at 8
bits (u8 planes: the 256-entry tables in LDS, float32) and at 16 bits (u16 planes: pow in double),
the 16-bit one again with 1,024-entry `curv` tables, a CIELab image at 8 bits (u16 planes), and an
sYCC 4:4:4 image at 8 and 16 bits under GK_DISPLAY_RGB.  `summarise` prints min / median / max per
kernel and the median's algorithmic bytes/s (every source sample read once, every output sample
written once)."""
import csv
import json
import os
import re
import statistics
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

SIZE = 8192
REPS = 8


def _box(typ, payload):
    return struct.pack(">I4s", 8 + len(payload), typ) + payload


def _prefix(w, h, prec, colr, cs_len):
    sig = struct.pack(">I4sI", 12, b"jP  ", 0x0d0a870a)
    ftyp = _box(b"ftyp", b"jp2 " + struct.pack(">I", 0) + b"jp2 ")
    ihdr = _box(b"ihdr", struct.pack(">IIHBBBB", h, w, 3, prec - 1, 7, 0, 0))
    return sig + ftyp + _box(b"jp2h", ihdr + colr) + struct.pack(">I4s", 8 + cs_len, b"jp2c")


def run(size=SIZE, reps=REPS):
    import torch
    import grok_amd as G
    import icc_profiles as P
    eng = G.Engine(0)
    buf = torch.empty(size * size * 3, dtype=torch.uint8, device="cuda")
    yy = torch.arange(size, device="cuda", dtype=torch.int32)[:, None]
    xx = torch.arange(size, device="cuda", dtype=torch.int32)[None, :]
    p = G.default_params(numresolution=6, mct=False)
    streams = {}
    for prec in (8, 16):   # smooth planes: small streams, short decodes
        planes = torch.stack([((xx * (3 + k) + yy * (2 + k)) // 8 % (1 << prec)).to(torch.int32) for k in range(3)]).contiguous()
        n = eng.encode(planes, prec, params=p, out=buf)
        streams[prec] = buf[:n].clone()
    sycc = _box(b"colr", struct.pack(">BBBI", 1, 0, 0, 18))
    cases = [("icc_rgb8_gamma", 8, P.colr_profile(P.rgb_profile("adobe", "g22")), dict(icc=True), torch.uint8),
             ("icc_rgb16_gamma", 16, P.colr_profile(P.rgb_profile("adobe", "g22")), dict(icc=True), torch.int16),
             ("icc_rgb16_table", 16, P.colr_profile(P.rgb_profile("adobe", "table1024")), dict(icc=True), torch.int16),
             ("lab8", 8, P.colr_lab(), dict(icc=True), torch.int16),
             ("sycc444_8", 8, sycc, dict(rgb=True), torch.uint8),
             ("sycc444_16", 16, sycc, dict(rgb=True), torch.int16)]
    for name, prec, colr, kw, dt in cases:
        cs = streams[prec]
        pre = torch.frombuffer(bytearray(_prefix(size, size, prec, colr, cs.numel())), dtype=torch.uint8).cuda()
        f = torch.cat([pre, cs]).contiguous()
        y = torch.empty((3, size, size), dtype=dt, device="cuda")
        eng.set_decode_display(**kw)
        for _ in range(reps + 1):
            eng.decode(f, length=f.numel(), out=y)
        print(json.dumps(dict(case=name, flags=kw, reps=reps, size=size)), flush=True)
    eng.set_decode_display()
    eng.close()


TYPE_BYTES = {"unsigned char": 1, "unsigned short": 2, "int": 4}


def summarise(path, size=SIZE):
    npix = size * size
    groups = {}
    for r in csv.DictReader(open(path)):
        m = re.search(r"(k_icc_rgb|k_lab_rgb|k_ycc_rgb)<([^<>]*)>", r["Kernel_Name"])
        if not m:
            continue
        args = [a.strip() for a in m.group(2).split(",")]
        nbytes = 3 * npix * (TYPE_BYTES[args[0]] + TYPE_BYTES[args[1]])
        groups.setdefault(("%s<%s>" % (m.group(1), ", ".join(args)), nbytes), []).append(
            (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print("# %s, image %d x %d x 3; times in us over all launches (warm-up included), TB/s of the median" % (path, size, size))
    print("%-60s %4s %9s %9s %9s %8s %6s" % ("kernel", "n", "min", "median", "max", "MB", "TB/s"))
    for (k, b), t in sorted(groups.items()):
        med = statistics.median(t)
        print("%-60s %4d %9.1f %9.1f %9.1f %8.1f %6.2f" % (k[:60], len(t), min(t), med, max(t), b / 1e6, b / med / 1e6))


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else "run"
    if cmd == "summarise":
        summarise(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else SIZE)
    else:
        run(*(int(a) for a in sys.argv[2:]))
