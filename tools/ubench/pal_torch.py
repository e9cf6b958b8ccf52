"""The yardstick of tools/ubench/pal_bench.hip: torch's lut[idx.long()] gather of an 8-bit index
plane through a (entries, columns) uint8 table, to the same bytes of output.
  python tools/ubench/pal_torch.py [side = 8192] [entries = 256] [columns = 3] [runs = 5] [reps = 20]
Prints each run's median and their spread (the noise margin of the comparison)."""
import sys

import torch

side, ne, npc, runs, reps = [int(v) for v in sys.argv[1:6]] + [8192, 256, 3, 5, 20][len(sys.argv) - 1:]
g = torch.Generator(device="cuda").manual_seed(1)
idx = torch.randint(0, 256, (side, side), dtype=torch.uint8, device="cuda", generator=g)
lut = torch.randint(0, 256, (ne, npc), dtype=torch.uint8, device="cuda", generator=g)
meds = []
for r in range(runs):
    for _ in range(3):
        out = lut[idx.long().clamp_(max=ne - 1)]
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = lut[idx.long().clamp_(max=ne - 1)]
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    meds.append(ts[len(ts) // 2])
    print("run %d: median %.4f ms (min %.4f, max %.4f)" % (r, meds[-1], ts[0], ts[-1]))
assert tuple(out.shape) == (side, side, npc) and out.dtype == torch.uint8
print("torch lut[idx.long()] %dx%d -> %d x u8: medians %.4f .. %.4f ms, spread %.4f ms" %
      (side, side, npc, min(meds), max(meds), max(meds) - min(meds)))
