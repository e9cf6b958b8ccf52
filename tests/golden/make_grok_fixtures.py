"""Record Grok 9.2.0's own output under tests/golden/grok/, from the binaries of
`make -C oracle ref GROK_SRC=<source tree>` (tests/grok_ref.py).

One .npz per entry of tests/grok_cases.py::FIXTURES: the image key and its synth_image arguments
(in place of the image), grk_compress's flags and codestream, grk_decompress's flags and decode (or the note that it is the image itself, sample for sample).
Every option family and every decode option (-l, -r, -d, -t) appears at least once.  Each case is
checked against the oracle as it is written (bytes, then decode: equal, 9/7 included), so a
recording that the CPU test would not pass is never made.  Files carry fixed zip timestamps: a
rerun rewrites them byte for byte.

Usage:  python tests/golden/make_grok_fixtures.py
"""
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import grok_cases as C  # noqa: E402
import grok_ref  # noqa: E402

OUT = os.path.join(HERE, "grok")
MAX_FILE = 96 * 1024
MAX_DIR = 1 << 20


def write_npz(path, arrays):
    """An .npz that np.load reads, with fixed timestamps and order (np.savez stamps the clock)."""
    with zipfile.ZipFile(path, "w") as z:
        for k, a in arrays.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(a), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, b.getvalue(), compresslevel=9)


def main():
    assert grok_ref.available(), grok_ref.why_not()
    os.makedirs(OUT, exist_ok=True)
    for f in os.listdir(OUT):
        if f.endswith(".npz"):
            os.remove(os.path.join(OUT, f))
    total = 0
    for i, ((key, flags), dflags) in enumerate(C.FIXTURES):
        cs = C.grok_encode(key, flags)
        assert cs == C.oracle_encode(key, flags), (key, flags)
        dec = grok_ref.decompress(cs, dflags)
        mine = C.oracle_decode(cs, dflags, flags)
        assert dec.shape == mine.shape and (dec == mine).all(), (key, flags, dflags)
        k = key[2:] if key[1:2] == ":" else key
        name = C.fixture_name(i)
        meta = dict(name=name, key=key, flags=flags, dflags=dflags, synth=list(C.IMAGES[k]), grok="9.2.0")
        arrays = dict(cs=np.frombuffer(cs, np.uint8))
        src = C.image(key)[0]
        if dec.shape == src.shape and (dec == src).all():
            meta["decoded"] = "source"   # Grok's decode is the image itself: not stored twice
        else:
            meta["decoded"] = "stored"
            dt = next(t for t in (np.uint8, np.int16, np.uint16) if np.iinfo(t).min <= dec.min() and dec.max() <= np.iinfo(t).max)
            arrays["grok_decoded"] = dec.astype(dt)
        arrays["meta"] = np.array(json.dumps(meta, sort_keys=True))
        path = os.path.join(OUT, name + ".npz")
        write_npz(path, arrays)
        n = os.path.getsize(path)
        assert n < MAX_FILE, (name, n)
        total += n
        print("%-70s %6d B stream %6d B file  decode %s" % (name, len(cs), n, dec.shape))
    assert total < MAX_DIR, total
    print("%d fixtures, %d bytes" % (len(C.FIXTURES), total))


if __name__ == "__main__":
    main()
