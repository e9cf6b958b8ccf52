"""Cost of the HT 9/7 quantisation control (Engine.set_encode_quant) on device-resident images of
grok_amd.synth.synth_image: a 4096 x 4096 16-bit mono image (one tile) and the 2048 x 2048 crop of
the benchmark's C4 configuration (16-bit mono, 1024 x 1024 tiles, TLM + PLT), both HTJ2K 9/7.

  python tools/htq_bench.py plain [RUNS]    the plain encode alone
  python tools/htq_bench.py quant [RUNS]    plain, STEP at notch 16, BYTES at 1/4 of the notch-0
                                            length, PSNR at 40 dB
  python tools/htq_bench.py psnr [RUNS]     the PSNR case alone (for a kernel trace of k_htq_dist:
                                            rocprofv3 --kernel-trace --stats -- python ... psnr)
  python tools/htq_bench.py ab LIB [ROUNDS [RUNS]]
                                            A / B: `plain` in fresh child processes, alternately with
                                            GROK_AMD_LIB=LIB (A: another build of the library, e.g.
                                            the parent commit's) and without (B: this build), ROUNDS
                                            times; then each side's medians and their spread

One JSON line per image and case after a warm-up call: every run's wall time (a host clock around
the synchronous call, which ends in a stream synchronise) and the engine's own total (HIP events),
their medians, the stream length and, with a setting, what gk_get_encode_quant reports."""
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def main(mode="quant", runs=7):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(HERE, ".."))
    import grok_amd as G
    from grok_amd.synth import synth_image
    images = [("mono16 4096^2", synth_image(4096, 4096, 1, 16, 20), dict()),
              ("C4 crop 2048^2", synth_image(2048, 2048, 1, 16, 20), dict(tiles=(1024, 1024), tlm=True, plt=True))]
    eng = G.Engine(0)
    try:
        for name, a, kw in images:
            img = torch.from_numpy(a.astype(np.int32)).cuda()
            out = torch.empty(a.size * 4, dtype=torch.uint8, device="cuda")
            p = G.default_params(cblk_sty=0x40, irreversible=True, **kw)

            def timed(case):
                wall, tot, n = [], [], 0
                for i in range(runs + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    n = eng.encode(img, 16, params=p, out=out)
                    t1 = time.perf_counter()
                    if i:
                        wall.append((t1 - t0) * 1e3); tot.append(eng.timings().total_ms)
                rec = dict(image=name, case=case, runs_wall_ms=[round(v, 3) for v in wall],
                           wall_ms=round(statistics.median(wall), 3), total_ms=round(statistics.median(tot), 3),
                           t1_ms=round(eng.timings().t1_ms, 3), stream_bytes=n)
                if case != "plain":
                    r = eng.encode_quant()
                    rec.update(notch=r["notch"], t1_passes=r["t1_passes"], stats_passes=r["stats_passes"],
                               est_psnr=round(r["est_psnr"], 3))
                print(json.dumps(rec), flush=True)
                return n
            if mode == "psnr":
                eng.set_encode_quant(psnr=40.0)
                timed("psnr 40 dB")
                eng.set_encode_quant()
                continue
            full = timed("plain")
            if mode != "quant":
                continue
            lo = G.probe_encode_quant(tuple(img.shape), 16, p)[0]
            for case, q in (("step notch 16", dict(step=lo * 4.0)), ("bytes 1/4", dict(max_bytes=full // 4)),
                            ("psnr 40 dB", dict(psnr=40.0))):
                eng.set_encode_quant(**q)
                timed(case)
            eng.set_encode_quant()
    finally:
        eng.close()


def ab(lib, rounds=3, runs=7):
    """`plain` in fresh children, A (GROK_AMD_LIB=lib) and B alternating; medians and spreads."""
    got = {}
    for r in range(rounds):
        for side in ("A", "B"):
            env = dict(os.environ)
            env.pop("GROK_AMD_LIB", None)
            if side == "A":
                env["GROK_AMD_LIB"] = os.path.abspath(lib)
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "plain", str(runs)], env=env, check=True,
                               stdout=subprocess.PIPE, timeout=300).stdout.decode()
            for line in o.splitlines():
                if line.startswith("{"):
                    rec = json.loads(line)
                    print(json.dumps(dict(side=side, round=r + 1, **rec)), flush=True)
                    got.setdefault((rec["image"], side), []).append((rec["wall_ms"], rec["total_ms"]))
    for (image, side), v in sorted(got.items()):
        w, t = [x[0] for x in v], [x[1] for x in v]
        print(json.dumps(dict(image=image, side=side, wall_ms_by_round=w, wall_ms=round(statistics.median(w), 3),
                              wall_spread_ms=round(max(w) - min(w), 3), total_ms_by_round=t,
                              total_ms=round(statistics.median(t), 3), total_spread_ms=round(max(t) - min(t), 3))), flush=True)


if __name__ == "__main__":
    if sys.argv[1:2] == ["ab"]:
        ab(sys.argv[2], *(int(a) for a in sys.argv[3:5]))
    else:
        main(*(sys.argv[1:2] + [int(a) for a in sys.argv[2:3]]))
