"""The corpus of streams written by OpenJPEG's encoder (tests/golden/opj/*.npz, written by
tests/golden/make_opj_fixtures.py): loading only, so that the GPU tests need neither Pillow nor
libopenjp2."""
import glob
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OPJ_DIR = os.path.join(HERE, "golden", "opj")


class OpjFixture:
    def __init__(self, path):
        z = np.load(path)
        self.path = path
        self.name = os.path.basename(path)[:-4]
        self.cs = z["cs"].tobytes()
        self.meta = json.loads(str(z["meta"]))
        self.expect = self.meta["expect"]
        n = self.expect["comps"]
        self.planes = [z["c%d" % k].astype(np.int32) for k in range(n)]
        self.limited = {}   # "r1" / "r2" / "l1" -> planes
        if self.meta["marked"]:
            for tag in ("r1", "r2", "l1"):
                self.limited[tag] = [z["%s_c%d" % (tag, k)].astype(np.int32) for k in range(n)]

    lossless = property(lambda self: not self.expect["irreversible"])
    subsampled = property(lambda self: any(tuple(d) != (1, 1) for d in self.expect["sub"]))
    tiled = property(lambda self: self.expect["tiles"] is not None)
    layered = property(lambda self: self.expect["layers"] > 1)

    def __repr__(self):
        return self.name


def load():
    return [OpjFixture(p) for p in sorted(glob.glob(os.path.join(OPJ_DIR, "*.npz")))]


def planes_of(decoded):
    """Engine / oracle decode result ((C, H, W) array or list of planes) -> list of 2-D planes."""
    return [np.asarray(p) for p in decoded]


def maxabs(got, want):
    """Largest sample difference over the components, None if a shape differs."""
    got, want = planes_of(got), planes_of(want)
    if len(got) != len(want) or any(g.shape != w.shape for g, w in zip(got, want)):
        return None
    return max((int(np.abs(g.astype(np.int64) - w).max()) for g, w in zip(got, want) if g.size), default=0)
