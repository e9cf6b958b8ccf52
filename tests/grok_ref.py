"""Grok 9.2.0's own command-line tools as a test reference.

`make -C oracle ref GROK_SRC=<source tree>` builds grk_compress / grk_decompress / grk_dump into
oracle/_ref/bin (not committed).  This module runs them as child processes on temporary PNM / PGX
files; the children never open a GPU.  A test that needs them calls `need()` and skips with the
reason when they are absent or do not start.

    compress(img, bits, flags)      -> codestream bytes       (grk_compress -i .. -o .. <flags>)
    decompress(cs, flags)           -> (C, H, W) int32 array  (grk_decompress -i .. -o x.pgx <flags>)
                                       or a list of planes where the components differ in size

Decoded output goes through PGX, the one format of the CLI that keeps every precision, the sign
and one file per component ("PG ML +|- prec w h", big-endian samples of 1 or 2 bytes).
"""
import os
import shlex
import subprocess
import tempfile

import numpy as np
import pytest

from grok_amd.synth import write_pnm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oracle", "_ref", "bin")
TOOLS = ("grk_compress", "grk_decompress", "grk_dump")

_state = None


def _env():
    # the children are plain CPU programs: the caller's environment, with no device to open
    return dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")


def why_not():
    """'' when the three binaries exist and start, else the reason they cannot be used."""
    global _state
    if _state is None:
        _state = ""
        for t in TOOLS:
            p = os.path.join(BIN, t)
            if not os.access(p, os.X_OK):
                _state = "%s is not built (make -C oracle ref GROK_SRC=<Grok 9.2.0 source>)" % os.path.relpath(p, ROOT)
                break
        if not _state:   # one 8 x 8 round trip: the binaries start and find their library
            try:
                img = (np.arange(64, dtype=np.int32).reshape(1, 8, 8) * 3) % 251
                if not (decompress(compress(img, 8, "-n 2")) == img).all():
                    _state = "oracle/_ref/bin: Grok's 8 x 8 round trip is not lossless"
            except (OSError, subprocess.TimeoutExpired, GrokError) as e:
                _state = "oracle/_ref/bin does not run here: %s" % str(e)[-300:]
    return _state


def available():
    return not why_not()


def need():
    if not available():
        pytest.skip(why_not())


class GrokError(RuntimeError):
    pass


def _run(tool, args):
    cmd = [os.path.join(BIN, tool)] + args
    r = subprocess.run(cmd, env=_env(), capture_output=True, timeout=300, cwd=os.path.dirname(args[1]))
    if r.returncode != 0:
        raise GrokError("%s %s: exit %d\n%s" % (tool, " ".join(args), r.returncode,
                                                (r.stdout + r.stderr)[-800:].decode(errors="replace")))
    return r


def write_pgx(path, plane, bits, signed):
    h, w = plane.shape
    with open(path, "wb") as f:
        f.write(b"PG ML %s %d %d %d\n" % (b"-" if signed else b"+", bits, w, h))
        a = np.asarray(plane).astype(np.int64) & ((1 << (8 if bits <= 8 else 16)) - 1)
        f.write(a.astype(np.uint8).tobytes() if bits <= 8 else a.astype(">u2").tobytes())


def read_pgx(path):
    """-> (H, W) int32 plane, precision, signed."""
    with open(path, "rb") as f:
        d = f.read()
    nl = d.index(b"\n")
    t = d[:nl].split()
    assert t[0] == b"PG" and t[1] in (b"ML", b"LM"), d[:nl]
    if len(t) == 6:
        signed, prec, w, h = t[2] == b"-", int(t[3]), int(t[4]), int(t[5])
    else:   # the sign may be left out, or written against the precision
        signed, prec, w, h = t[2][:1] == b"-", abs(int(t[2])), int(t[3]), int(t[4])
    nb = 1 if prec <= 8 else 2
    dt = np.dtype(np.uint8) if nb == 1 else np.dtype(">u2" if t[1] == b"ML" else "<u2")
    a = np.frombuffer(d[nl + 1:nl + 1 + w * h * nb], dtype=dt).reshape(h, w).astype(np.int32)
    if signed:   # the writer stores the low 8 or 16 bits of the two's complement value
        a = ((a + (1 << (8 * nb - 1))) & ((1 << (8 * nb)) - 1)) - (1 << (8 * nb - 1))
    return a, prec, signed


def compress(img, bits, flags="", signed=False, ext=".j2k", threads=1):
    """Grok's codestream (or .jp2 file with ext=".jp2") of a (C, H, W) image.  signed: one
    component, handed over as PGX (the CLI's PNM reader is unsigned)."""
    img = np.asarray(img)
    with tempfile.TemporaryDirectory() as td:
        if signed:
            assert img.shape[0] == 1, "PGX holds one component"
            src = os.path.join(td, "in.pgx")
            write_pgx(src, img[0], bits, True)
        else:
            src = os.path.join(td, "in.ppm" if img.shape[0] == 3 else "in.pgm")
            write_pnm(src, img, bits)
        out = os.path.join(td, "out" + ext)
        _run("grk_compress", ["-i", src, "-o", out, "-H", str(threads)] + shlex.split(flags))
        with open(out, "rb") as f:
            return f.read()


def decompress(cs, flags="", ext=None, threads=1, info=False):
    """Grok's decode of a codestream or JP2 file, every component through PGX.  flags are
    grk_decompress's (-r, -l, -d x0,y0,x1,y1, -t, -f, -u, -p ...).  Returns a (C, H, W) int32
    array, or a list of planes where the components differ in size; with info=True also
    [(precision, signed)] per component."""
    if ext is None:
        ext = ".jp2" if cs[4:8] == b"jP  " else ".j2k"
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "in" + ext)
        with open(src, "wb") as f:
            f.write(cs)
        _run("grk_decompress", ["-i", src, "-o", os.path.join(td, "out.pgx"), "-H", str(threads)]
             + shlex.split(flags))
        planes, meta, k = [], [], 0
        while os.path.exists(os.path.join(td, "out_%d.pgx" % k)):
            a, prec, sg = read_pgx(os.path.join(td, "out_%d.pgx" % k))
            planes.append(a)
            meta.append((prec, sg))
            k += 1
    if not planes:
        raise GrokError("grk_decompress wrote no component")
    out = np.stack(planes, 0) if all(p.shape == planes[0].shape for p in planes) else planes
    return (out, meta) if info else out
