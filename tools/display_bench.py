"""Cost of the display stage (gk_set_decode_display: k_ycc_rgb, k_upsample) beside its yardsticks
(k_jp2_palette on a 3-channel expansion, k_dwt53_inv_l1), on device-resident streams and planes.

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/display_bench.py run
  python tools/display_bench.py summarise OUT/**/run_kernel_trace.csv     # per kernel: time, bytes/s
  python tools/display_bench.py timings                                   # gk_get_timings, profiler off

`run` decodes, REPS times each after one warm-up: sYCC 4:4:4 / 4:2:2 / 4:2:0 under rgb and 4:2:0
under upsample, 8-bit into u8 planes and 12-bit into u16 planes, then a 256-entry 3-column palette
file into u8 planes.  `summarise` counts the algorithmic bytes of every launch from its kernel's
template arguments and the image size (kept here, with the benchmark) and prints min / median /
max time and the median's bytes/s.  `timings` prints the decoder's stage times for the 8-bit
4:2:0 stream with and without rgb."""
import csv
import json
import re
import statistics
import struct
import sys

SIZE = 8192
REPS = 8
SUBS = {"444": [(1, 1)] * 3, "422": [(1, 1), (2, 1), (2, 1)], "420": [(1, 1), (2, 2), (2, 2)]}


def _box(typ, payload):
    return struct.pack(">I4s", 8 + len(payload), typ) + payload


def _jp2_prefix(w, h, nc, prec, enumcs, cs_len, extra=b""):
    sig = struct.pack(">I4sI", 12, b"jP  ", 0x0d0a870a)
    ftyp = _box(b"ftyp", b"jp2 " + struct.pack(">I", 0) + b"jp2 ")
    ihdr = _box(b"ihdr", struct.pack(">IIHBBBB", h, w, nc, prec - 1, 7, 0, 0))
    colr = _box(b"colr", struct.pack(">BBBI", 1, 0, 0, enumcs))
    return sig + ftyp + _box(b"jp2h", ihdr + colr + extra) + struct.pack(">I4s", 8 + cs_len, b"jp2c")


def _streams(eng, torch, G, size, cases):
    """name -> (device file bytes, length, output dtype)."""
    out = {}
    buf = torch.empty(size * size * 2, dtype=torch.uint8, device="cuda")
    yy = torch.arange(size, device="cuda", dtype=torch.int32)[:, None]
    xx = torch.arange(size, device="cuda", dtype=torch.int32)[None, :]

    def plane(h, w, prec, k):   # smooth, so that the streams stay small and the decodes short
        return ((xx[:, :w] * (3 + k) + yy[:h] * (2 + k)) // 8 % (1 << prec)).to(torch.int32).contiguous()

    def wrap(n, nc, prec, enumcs, extra=b""):
        pre = torch.frombuffer(bytearray(_jp2_prefix(size, size, nc, prec, enumcs, n, extra)), dtype=torch.uint8).cuda()
        return torch.cat([pre, buf[:n]]).contiguous()

    p = G.default_params(numresolution=6, mct=False)
    for name, sub, prec in cases:
        planes = [plane(*G.comp_shape(size, size, dx, dy), prec, k) for k, (dx, dy) in enumerate(sub)]
        if all(d == (1, 1) for d in sub):
            n = eng.encode(torch.stack(planes), prec, params=p, out=buf)
        else:
            n = eng.encode(planes, prec, params=p, out=buf, subsampling=sub, size=(size, size))
        f = wrap(n, 3, prec, 18)
        out[name] = (f, f.numel(), torch.uint8 if prec <= 8 else torch.int16)
    # the palette yardstick: 8-bit indices through a 256 x 3 table of 8-bit columns
    n = eng.encode(plane(size, size, 8, 0)[None], 8, params=p, out=buf)
    lut = bytes((i * 7 + c * 50) & 255 for i in range(256) for c in range(3))
    pclr = _box(b"pclr", struct.pack(">HB", 256, 3) + bytes([7, 7, 7]) + lut)
    cmap = _box(b"cmap", b"".join(struct.pack(">HBB", 0, 1, c) for c in range(3)))
    f = wrap(n, 1, 8, 16, pclr + cmap)
    out["palette"] = (f, f.numel(), torch.uint8)
    return out


def _setup():
    import torch
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import grok_amd as G
    return torch, G, G.Engine(0)


def run(size=SIZE, reps=REPS):
    torch, G, eng = _setup()
    cases = [("%s_%d" % (m, prec), SUBS[m], prec) for prec in (8, 12) for m in ("444", "422", "420")]
    files = _streams(eng, torch, G, size, cases)
    for name, (f, n, dt) in files.items():
        y = torch.empty((3, size, size), dtype=dt, device="cuda")
        modes = [dict()] if name == "palette" else [dict(rgb=True)] + ([dict(upsample=True)] if name.startswith("420") else [])
        for kw in modes:
            eng.set_decode_display(**kw)
            for _ in range(reps + 1):
                eng.decode(f, length=n, out=y)
            print(json.dumps(dict(case=name, flags=kw, reps=reps, size=size)), flush=True)
    eng.set_decode_display()
    eng.close()


def timings(size=SIZE, reps=REPS):
    torch, G, eng = _setup()
    f, n, dt = _streams(eng, torch, G, size, [("420_8", SUBS["420"], 8)])["420_8"]
    fields = ("t2_ms", "t1_ms", "dwt_ms", "mct_ms", "assemble_ms", "total_ms")
    for kw in (dict(), dict(rgb=True), dict(), dict(rgb=True)):   # (alternating: the spread shows)
        eng.set_decode_display(**kw)
        if kw:
            out = torch.empty((3, size, size), dtype=dt, device="cuda")
        else:
            out = [torch.empty(G.comp_shape(size, size, dx, dy), dtype=dt, device="cuda") for dx, dy in SUBS["420"]]
        rows = []
        for _ in range(reps + 1):
            eng.decode(f, length=n, out=out)
            t = eng.timings()
            rows.append([getattr(t, k) for k in fields])
        med = [round(statistics.median(c), 4) for c in zip(*rows[1:])]
        print(json.dumps(dict(case="420_8", flags=kw, size=size, reps=reps, median_ms=dict(zip(fields, med)))), flush=True)
    eng.set_decode_display()
    eng.close()


TYPE_BYTES = {"unsigned char": 1, "unsigned short": 2, "int": 4}


def launch_bytes(name, npix, seq):
    """Algorithmic bytes (read, written) of one launch on an image of npix pixels; seq: position in
    a run of consecutive launches of the same kernel (k_upsample: luma copy, then two chroma planes)."""
    m = re.search(r"(k_\w+)<([^<>]*)>", name)
    if not m:
        return None
    k, args = m.group(1), [a.strip() for a in m.group(2).split(",")]
    if k == "k_ycc_rgb":
        s, d, mode = TYPE_BYTES[args[0]], TYPE_BYTES[args[1]], int(re.sub(r"\D", "", args[2]))
        return ({0: 3.0, 1: 2.0, 2: 1.5, 3: 3.0}[mode] * s * npix, 3 * d * npix)
    if k == "k_upsample":
        s, d = TYPE_BYTES[args[0]], TYPE_BYTES[args[1]]
        return ((1.0 if seq % 3 == 0 else 0.25) * s * npix, d * npix)
    if k == "k_jp2_palette":
        return (TYPE_BYTES[args[0]] * npix, 3 * TYPE_BYTES[args[1]] * npix)
    return None


def summarise(path, size=SIZE):
    npix = size * size
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    groups, prev, seq = {}, None, 0
    for r in rows:
        name = r["Kernel_Name"]
        seq = seq + 1 if name == prev else 0
        prev = name
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        short = re.sub(r"\(anonymous namespace\)::|void |\(Gk\w+\)$", "", name)
        if "k_upsample" in name:
            short += " luma copy" if seq % 3 == 0 else " chroma 2x2"
            key = (short, launch_bytes(name, npix, seq))
        elif "k_ycc_rgb" in name or "k_jp2_palette" in name:
            key = (short, launch_bytes(name, npix, seq))
        elif "k_dwt53_inv_l1" in name:
            key = (short + " grid " + "x".join(r.get(k, "?") for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z")), None)
        else:
            continue
        groups.setdefault(key, []).append(us)
    print("# %s, image %d x %d; times in us over all launches (warm-up included), TB/s of the median" % (path, size, size))
    print("%-78s %5s %9s %9s %9s %8s %7s" % ("kernel", "n", "min", "median", "max", "MB", "TB/s"))
    for (short, b), t in sorted(groups.items()):
        med = statistics.median(t)
        mb = "%8.1f" % (sum(b) / 1e6) if b else "       -"
        rate = "%7.2f" % (sum(b) / med / 1e6) if b else "      -"
        print("%-78s %5d %9.1f %9.1f %9.1f %s %s" % (short[:78], len(t), min(t), med, max(t), mb, rate))


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else "run"
    if cmd == "summarise":
        summarise(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else SIZE)
    else:
        {"run": run, "timings": timings}[cmd](*(int(a) for a in sys.argv[2:]))
