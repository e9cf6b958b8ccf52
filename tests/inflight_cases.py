"""Engines at work at the same time on one device, one host thread each: the cases and the thread
harness of tests/test_gpu_inflight.py, which runs every scenario below in a child process of its
own (python -c "import inflight_cases; inflight_cases.main(name)"), and the matrix that
tests/test_inflight_cases.py checks on the CPU.

Every scenario computes its oracle answers first, on the main thread (the oracle's decode settings
are process-wide), then starts the threads: one grok_amd.Engine(0) each, a barrier at the start of
every round, failures collected per thread and reported by the main thread, joins with a time limit.
The oracle is the judge everywhere: encoded bytes equal oracle.encode's, decoded samples equal
oracle.decode's, display output equals tests/display_ref.py applied to the oracle's planes.

The shared packing rule (gk_engine.cpp solo_split, `shared`): while another engine of the device is
inside a call, a Part-1 decode gives a block to a solo wave only if it is heavier than 1.3 x the
block at rank min(max(1024, top), nbr - 1), one block per wave, at most min(nbr / 4, waves) of them.
shared_solo() restates it over the oracle's block lengths; shared_matrix() holds one case per edge.
"""
import os
import sys
import threading
import time
import traceback

import numpy as np

import grok_amd as G
import oracle as O

LIMIT = 90.0          # seconds a scenario's threads may take before they count as hung
ROUNDS = 3
# The occupiers of the shared-rule scenario encode 3 x 1024 x 1024 samples, lossless, from host
# memory (a few milliseconds a call, against microseconds between two calls); 2048 x 2048 is the most
# the scenario may use.  The log prints how much of its time each occupier spent inside calls.
OCCUPIER_SHAPE = (3, 1024, 1024)
ATTEMPTS, MAX_ATTEMPTS = 6, 20   # decodes per case; more, up to 20, only while none ran shared
SOLO_WAVES = 512      # solo waves of a decode under 1,100 blocks on an MI355X (gk_t1dec_solo_plan)


# ------------------------------------------------------------------------------------ helpers
def gk_params(kw):
    """oracle.encode keywords -> grok_amd.default_params."""
    k = dict(kw)
    for a, b in (("numres", "numresolution"), ("nlayers", "numlayers")):
        if a in k:
            k[b] = k.pop(a)
    if "layer_rate" in k:
        k["numlayers"] = len(k["layer_rate"])
    return G.default_params(**k)


def smooth(seed, c, h, w, bits=8):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (np.sin(xx / 9.0 + seed) * np.cos(yy / 7.0) + 1) * (1 << (bits - 2))
    return np.clip(base[None].repeat(c, 0) + rng.integers(0, 1 << (bits - 3), size=(c, h, w)), 0,
                   (1 << bits) - 1).astype(np.int32)


def noise(seed, c, h, w, bits=8):
    return np.random.default_rng(seed).integers(0, 1 << bits, size=(c, h, w)).astype(np.int32)


def oracle_decode(cs, partial=False, layers=0, reduce=0):
    O.set_decode_layers(layers)
    O.set_decode_reduce(reduce)
    try:
        return O.decode(cs, partial=partial)[0]
    finally:
        O.set_decode_layers(0)
        O.set_decode_reduce(0)


def same(got, want, what):
    got, want = list(got), list(want)
    assert len(got) == len(want), what
    for c, (g, w) in enumerate(zip(got, want)):
        if not np.array_equal(g, w):
            d = np.abs(np.asarray(g, np.int64) - w) if np.shape(g) == np.shape(w) else None
            raise AssertionError("%s: component %d differs from the oracle (%s)" %
                                 (what, c, "shapes %s / %s" % (np.shape(g), np.shape(w)) if d is None else
                                  "%d samples, largest difference %d" % (int((d != 0).sum()), int(d.max()))))


class Case:
    """One unit of work on an engine; run(e) raises when a result differs from the oracle's."""

    def __init__(self, name, run):
        self.name, self.run = name, run


def enc_dec(name, img, bits, kw):
    """Encode (bytes equal the oracle's), then decode those bytes (samples equal the oracle's)."""
    ref = O.encode(img, bits, **kw)
    want = O.decode(ref)[0]

    def run(e):
        assert e.encode(img, bits, params=gk_params(kw)) == ref, name + ": encoded bytes differ from the oracle's"
        same(e.decode(ref), want, name + " decode")
    return Case(name, run)


# --------------------------------------------------------------------------------- the threads
def run_threads(bodies, limit=LIMIT):
    """bodies[k](k, e, sync): thread k's work on its own engine e; sync() is the barrier that starts
    a round.  Returns after every thread ended; exits the process with a report otherwise."""
    n = len(bodies)
    bar = threading.Barrier(n)
    fails = [[] for _ in range(n)]

    def sync():
        bar.wait(timeout=limit)

    def wrap(k):
        e = None
        try:
            e = G.Engine(0)
            bodies[k](k, e, sync)
        except threading.BrokenBarrierError:
            fails[k].append("stopped at a barrier: another thread failed or did not arrive")
        except BaseException:
            fails[k].append(traceback.format_exc())
            bar.abort()
        finally:
            if e is not None:
                e.close()

    ts = [threading.Thread(target=wrap, args=(k,), daemon=True) for k in range(n)]
    end = time.monotonic() + limit
    for t in ts:
        t.start()
    for t in ts:
        t.join(max(0.0, end - time.monotonic()))
    alive = [k for k, t in enumerate(ts) if t.is_alive()]
    for k in range(n):
        for f in fails[k]:
            print("thread %d: %s" % (k, f))
    for k in alive:
        print("thread %d is still running after %.0f s" % (k, limit))
    sys.stdout.flush()
    if alive:
        os._exit(3)   # (a thread inside a call cannot be stopped)
    if any(fails):
        sys.exit(1)


# ------------------------------------------------------------------------------- a. cold start
def _cold_jobs(pairing):
    """The two first calls of a process, as Cases."""
    from grok_amd.synth import synth_image
    im = [synth_image(256, 264, 3, 8, 3 + k).astype(np.int32) for k in range(2)]

    def dec(name, cs):
        want = O.decode(cs)[0]
        return Case(name, lambda e: same(e.decode(cs), want, name))
    p1 = [dec("Part-1 5/3 decode %d" % k, O.encode(im[k], 8)) for k in range(2)]
    if pairing == "decode_decode":
        return p1
    if pairing == "encode_decode":
        ref = O.encode(im[0], 8)

        def enc(e):
            assert e.encode(im[0], 8, params=gk_params({})) == ref, "first call, an encode: bytes differ from the oracle's"
        return [Case("Part-1 5/3 encode", enc), p1[1]]
    if pairing == "ht_part1":
        return [dec("HT decode", O.encode(im[0], 8, cblk_sty=0x40)), p1[1]]
    if pairing == "97_layers_53":
        img = smooth(5, 3, 200, 136, 12)
        return [dec("9/7 decode, three layers", O.encode(img, 12, irreversible=True, layer_rate=[40, 20, 10])), p1[1]]
    raise KeyError(pairing)


def cold(pairing):
    jobs = _cold_jobs(pairing)

    def body(k, e, sync):
        sync()
        jobs[k].run(e)        # the process's first call, made by both threads together
        sync()
        jobs[1 - k].run(e)    # then each thread the other's
    run_threads([body, body])


# ------------------------------------------------------------------------------- b. mixed work
def mixed_cases(device=True):
    """The case list every thread of the mixed scenarios walks."""
    import display_ref as R
    import jp2_boxes as J
    import subsampling_cases as S
    from grok_amd.synth import synth_image
    out = []
    rgb = smooth(1, 3, 96, 120)
    out.append(enc_dec("5/3 lossless RGB8, stream in host memory", rgb, 8, dict(numres=4, cblk=(32, 32))))
    lay_kw = dict(numres=4, irreversible=True, layer_rate=[40, 20, 10])
    lay = smooth(2, 3, 96, 120, 12)
    out.append(enc_dec("9/7 + ICT 12-bit, three layers", lay, 12, lay_kw))
    out.append(enc_dec("HT 5/3", smooth(3, 3, 80, 96), 8, dict(numres=4, cblk_sty=0x40)))
    out.append(enc_dec("HT 9/7", smooth(4, 3, 80, 96, 12), 12, dict(numres=4, cblk_sty=0x40, irreversible=True)))
    out.append(enc_dec("BYPASS|TERMALL", smooth(5, 3, 64, 80), 8, dict(numres=3, cblk=(32, 32), cblk_sty=0x05)))
    out.append(enc_dec("odd tiles", synth_image(70, 90, 3, 8, 3).astype(np.int32), 8, dict(tiles=(33, 41), numres=3)))

    W, H, sub, prec, _ = S.CASES["420_53"]
    planes = S.planes("420_53")
    ref420 = O.encode(planes, prec, size=(W, H), **S.oracle_kw("420_53"))
    want420 = O.decode(ref420)[0]
    pk, origin = S.engine_params("420_53")

    def run420(e):
        got = e.encode(planes, prec, params=G.default_params(**pk), origin=origin, subsampling=sub, size=(W, H))
        assert got == ref420, "4:2:0: encoded bytes differ from the oracle's"
        same(e.decode(ref420), want420, "4:2:0 decode")
    out.append(Case("4:2:0", run420))

    cs_rgb = O.encode(rgb, 8, numres=4, cblk=(32, 32))
    x0, y0, x1, y1 = win = (7, 5, 78, 63)
    want_win = oracle_decode(cs_rgb, partial=True)[:, y0:y1, x0:x1]
    out.append(Case("odd window", lambda e: same(e.decode_window(cs_rgb, win), want_win, "odd window")))

    want_red = oracle_decode(cs_rgb, reduce=1)

    def run_red(e):
        e.set_decode_reduce(1)
        try:
            same(e.decode(cs_rgb), want_red, "reduced decode")
        finally:
            e.set_decode_reduce(0)
    out.append(Case("reduce 1", run_red))

    cs_lay = O.encode(lay, 12, **lay_kw)
    want_l1 = oracle_decode(cs_lay, layers=1)

    def run_l1(e):
        e.set_decode_layers(1)
        try:
            same(e.decode(cs_lay), want_l1, "one layer of three")
        finally:
            e.set_decode_layers(0)
    out.append(Case("layers 1", run_l1))

    pal = J.cases()["c1_clamp200"]
    assert np.array_equal(O.decode(pal.cs)[0], pal.src)   # (lossless: the palette's input is the oracle's decode)
    h, w = pal.src.shape[1:]
    want_pal = np.stack(R.post_process(list(pal.want), [(1, 1, p, 0) for p in pal.out_prec], R.CS_SRGB, (0, 0, w, h),
                                       True, True)[0])
    ycc = J.cases()["c7_sycc"]
    assert np.array_equal(O.decode(ycc.cs)[0], ycc.src)
    nc, h, w = ycc.src.shape
    want_ycc = R.post_process(list(ycc.src), [(1, 1, 8, 0)] * nc, R.CS_SYCC, (0, 0, w, h), True, False)[0]

    def run_display(e):
        e.set_decode_display(rgb=True, upsample=True)
        try:
            same(e.decode(pal.file), want_pal, "palette file under the display flags")
            same(e.decode(ycc.file), want_ycc, "sYCC file to RGB")
        finally:
            e.set_decode_display()
        same(e.decode(ycc.file), ycc.src, "sYCC file, display off again")
    out.append(Case("jp2 palette + display", run_display))

    if device:
        import torch
        dense = noise(9, 3, 192, 256)
        cs_dev = O.encode(dense, 8)
        assert len(cs_dev) > (64 << 10)   # (several pinned pages)
        d = torch.frombuffer(bytearray(cs_dev), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        out.append(Case("stream on the device", lambda e: same(e.decode(d, len(cs_dev)), dense, "stream on the device")))
    return out


def walk(cases, rounds=ROUNDS, stride=None):
    def body(k, e, sync):
        n = len(cases)
        for r in range(rounds):
            sync()
            for j in range(n):
                cases[(j + k * (stride or 1) + r) % n].run(e)
    return body


def mixed(nthreads):
    nthreads = int(nthreads)
    import torch
    torch.cuda.init()
    cases = mixed_cases()
    run_threads([walk(cases, stride=max(1, len(cases) // nthreads))] * nthreads)


def sticky():
    """Settings held by one engine for the whole run; the others decode the same streams plainly."""
    import display_ref as R
    import jp2_boxes as J
    a = O.encode(smooth(11, 3, 96, 120), 8, numres=4, cblk=(32, 32), layer_rate=[30, 10, 0])
    b = O.encode(smooth(12, 3, 96, 120, 12), 12, numres=4, irreversible=True, layer_rate=[40, 20, 10])
    ycc = J.cases()["c7_sycc"]
    nc, h, w = ycc.src.shape
    rgb = R.post_process(list(ycc.src), [(1, 1, 8, 0)] * nc, R.CS_SYCC, (0, 0, w, h), True, False)[0]
    plain = [oracle_decode(a), oracle_decode(b), list(O.decode(ycc.cs)[0])]
    held = [oracle_decode(a, layers=1, reduce=1), oracle_decode(b, layers=1, reduce=1)]
    streams = [a, b, ycc.file]

    def holder(k, e, sync):
        e.set_decode_reduce(1)
        e.set_decode_layers(1)
        for r in range(ROUNDS):
            sync()
            for q in range(4):
                same(e.decode(streams[q & 1]), held[q & 1], "reduce 1 + one layer, held by this engine")

    def neutral(k, e, sync):
        for r in range(ROUNDS):
            sync()
            for q in range(6):
                same(e.decode(streams[q % 3]), plain[q % 3], "plain decode beside an engine with settings")

    def display(k, e, sync):
        e.set_decode_display(rgb=True)
        for r in range(ROUNDS):
            sync()
            for q in range(4):
                same(e.decode(ycc.file), rgb, "sYCC to RGB, held by this engine")
    run_threads([holder, neutral, display, neutral])


# ---------------------------------------------------------------------------- c. the host pool
def _refusals():
    img = smooth(31, 3, 64, 80)

    def run(e):
        try:
            e.encode_tiles(img, 8, 5, 9, params=gk_params(dict(tiles=(40, 32))))   # (4 tiles)
        except RuntimeError as x:
            assert "bad tile range" in str(x), x
        else:
            raise AssertionError("tiles 5..9 of 4 were encoded")
        try:
            e.encode(img, 8, params=gk_params(dict(cblk_sty=0x41)))   # (HT with a Part-1 mode switch)
        except RuntimeError:
            pass
        else:
            raise AssertionError("HT with a mode switch was encoded")
    return Case("refused encodes", run)


def pool(variant):
    """Rate-controlled encodes at the same time, two threads and then three.  "chunk512": one image
    of 1089 blocks in one band each, more than one chunk of 512; "chunk16": GK_PCRD_CHUNK=16 in the
    environment, small images with tiles, so that the pool gets many short jobs and a thread finds
    it taken for some and free for others."""
    if variant == "chunk512":
        kw = dict(cblk=(16, 16), numres=1, layer_rate=[16, 4])
        cases = [enc_dec("528 x 528, 16 x 16 blocks, two layers (image %d)" % k, smooth(20 + k, 1, 528, 528), 8, kw)
                 for k in range(3)]
        bodies = lambda n: [walk([cases[k]]) for k in range(n)]
    else:
        assert os.environ.get("GK_PCRD_CHUNK") == "16"
        cases = [
            enc_dec("128 x 128 x 3, tiles 64 x 64", smooth(24, 3, 128, 128), 8,
                    dict(numres=3, cblk=(16, 16), tiles=(64, 64), layer_rate=[30, 10])),
            enc_dec("200 x 136 x 3 9/7, tiles 72 x 50", smooth(25, 3, 200, 136, 12), 12,
                    dict(numres=3, cblk=(16, 16), tiles=(50, 72), irreversible=True, layer_rate=[40, 20, 10])),
            enc_dec("128 x 128 x 3 by quality", smooth(26, 3, 128, 128), 8, dict(cblk=(16, 16), quality=[30.0, 38.0])),
            _refusals(),
            enc_dec("200 x 136 x 3 5/3, one tile", smooth(27, 3, 200, 136), 8, dict(cblk=(16, 16), layer_rate=[20, 5])),
        ]
        bodies = lambda n: [walk(cases, stride=2)] * n
    for n in (2, 3):
        run_threads(bodies(n))


# ------------------------------------------------------------------ d. the shared packing rule
def shared_solo(weights, waves=SOLO_WAVES):
    """Blocks the shared rule sends to solo waves, from the block weights in table order."""
    nbr = len(weights)
    if nbr < 8 or not waves:
        return 0
    kmax = min(nbr // 4, 4 * waves)
    top = min(kmax + 1, nbr)
    byl = sorted(weights, reverse=True)
    ref = 1.3 * byl[min(max(1024, top), nbr - 1)]
    k = 0
    while k < min(kmax, waves) and byl[k] > ref:
        k += 1
    return k


def block_weights(img, bits, kw):
    """Weight of every code-block as the decoder sees it: its bytes, 0 without a pass."""
    blocks, _ = O.encode_blocks(img, bits, **kw)
    return [int(b.len) if b.npasses else 0 for b in blocks]


def _textured(h, w, cb, planted, seed):
    """5-bit noise everywhere (blocks of nearly equal weight), 8-bit noise in `planted` blocks spread
    over the grid.  A planted block weighs about 1.6 x a plain one: above the shared rule's 1.3, and
    under the 2.5 at which the default rule would stop giving plain blocks to solo waves, so that the
    two rules split these images differently."""
    rng = np.random.default_rng(seed)
    img = (128 + rng.integers(0, 32, size=(h, w))).astype(np.int32)
    nb = (h // cb) * (w // cb)
    for q in np.linspace(0, nb - 1, planted).astype(int):
        by, bx = divmod(int(q), w // cb)
        img[by * cb:(by + 1) * cb, bx * cb:(bx + 1) * cb] = rng.integers(0, 256, size=(cb, cb))
    return img[None]


class SharedCase:
    """name, stream, the oracle's answer, how to decode it, and what t1_solo_blocks must be when
    the decode ran under the shared rule (a (lo, hi) range, or None: samples only)."""

    def __init__(self, name, cs, want, solo=None, window=None, layers=0, shared=True, weights=None):
        self.name, self.cs, self.want, self.solo, self.window, self.layers = name, cs, want, solo, window, layers
        self.shared, self.weights = shared, weights

    def decode(self, e):
        e.set_decode_layers(self.layers)
        try:
            return e.decode_window(self.cs, self.window) if self.window else e.decode(self.cs)
        finally:
            e.set_decode_layers(0)


def shared_matrix():
    from grok_amd.synth import synth_image
    out = []

    def plain(name, img, bits, kw, solo):
        cs = O.encode(img, bits, **kw)
        w = block_weights(img, bits, kw)
        lo, hi = solo(w) if callable(solo) else solo
        k = shared_solo(w)
        assert lo <= k <= hi, (name, k, lo, hi)   # (the restated rule agrees with what the case is built for)
        want = O.decode(cs)[0]
        assert np.array_equal(want, img), name   # (lossless)
        out.append(SharedCase(name, cs, want, (k, k), weights=w))
        return cs

    # 1: the constant part reaches 8 columns past the middle, so that the 5/3 support of the noise
    # stays out of the left blocks: they are empty and the reference block has weight 0
    img = np.full((1, 128, 128), 128, np.int32)
    img[:, :, 72:] = noise(41, 1, 128, 56)
    plain("1 empty reference block", img, 8, dict(cblk=(32, 32), numres=2),
          lambda w: (min(len(w) // 4, sum(1 for v in w if v)),) * 2)
    # 2: 64 blocks of uniform noise, all within 1.3 x of each other
    plain("2 no solo block", noise(42, 1, 256, 256), 8, dict(cblk=(32, 32), numres=1), (0, 0))
    # 3 / 4: 1089 blocks, rank 1024 is the reference
    kw16 = dict(cblk=(16, 16), numres=1)
    img3 = _textured(528, 528, 16, 5, 43)
    cs3 = plain("3 five outliers of 1089", img3, 8, kw16, (1, 5))
    plain("4 the nbr / 4 cap", _textured(528, 528, 16, 300, 44), 8, kw16, (272, 272))
    # 5: exactly 1024 blocks, the reference is the last one
    plain("5 1024 blocks", _textured(512, 512, 16, 5, 45), 8, kw16, (1, 5))
    # 6: blocks without a pass under the layer limit
    img6 = smooth(46, 3, 200, 136, 12)
    cs6 = O.encode(img6, 12, irreversible=True, layer_rate=[40, 10])
    out.append(SharedCase("6 one layer of two", cs6, oracle_decode(cs6, layers=1), layers=1))
    # 7: several odd tiles, few blocks each
    img7 = synth_image(70, 90, 3, 8, 3).astype(np.int32)
    cs7 = O.encode(img7, 8, tiles=(33, 41), numres=3)
    out.append(SharedCase("7 odd tiles", cs7, O.decode(cs7)[0]))
    # 8: a window of case 3's stream
    x0, y0, x1, y1 = win = (37, 21, 300, 255)
    out.append(SharedCase("8 window", cs3, oracle_decode(cs3, partial=True)[:, y0:y1, x0:x1], window=win))
    # 9: 7 blocks, under the 8 that solo waves need: no rule is taken
    img9 = noise(49, 1, 64, 448)
    cs9 = O.encode(img9, 8, numres=1)
    assert len(block_weights(img9, 8, dict(numres=1))) == 7
    out.append(SharedCase("9 seven blocks", cs9, img9, (0, 0), shared=False))
    return out


def shared():
    """Two occupiers loop an encode each; a third thread decodes the matrix and reads t1_shared."""
    cases = shared_matrix()
    occ = smooth(50, *OCCUPIER_SHAPE)
    occ_ref = O.encode(occ, 8)
    stop = threading.Event()
    duty = [None, None]
    report = []

    def occupier(k, e, sync):
        p = gk_params({})
        sync()
        t0, inside, n = time.monotonic(), 0.0, 0
        try:
            while not stop.is_set():
                a = time.monotonic()
                got = e.encode(occ, 8, params=p)
                inside += time.monotonic() - a
                n += 1
                assert got == occ_ref, "occupier %d: encoded bytes differ from the oracle's" % k
        finally:
            stop.set()
        duty[k] = (inside / max(time.monotonic() - t0, 1e-9), n)

    def decoder(k, e, sync):
        try:
            # on a quiet device: the default rule, which splits cases 2 and 3 differently
            quiet = {}
            for c in cases:
                same(c.decode(e), c.want, c.name + ", quiet device")
                t = e.timings()
                assert t.t1_shared == 0, c.name + ": shared on a quiet device"
                quiet[c.name] = int(t.t1_solo_blocks)
            sync()
            # a sample mismatch ends the run at once; what the rule did is judged for every case
            problems = []
            for c in cases:
                seen, n, solo = 0, 0, set()
                while n < ATTEMPTS or (c.shared and not seen and n < MAX_ATTEMPTS):
                    same(c.decode(e), c.want, c.name + ", busy device")
                    t = e.timings()
                    n += 1
                    if t.t1_shared:
                        seen += 1
                        solo.add(int(t.t1_solo_blocks))
                report.append("shared %-28s %2d of %2d decodes; solo blocks shared %s, quiet %d" %
                              (c.name, seen, n, sorted(solo), quiet[c.name]))
                if c.shared and not seen:
                    problems.append("%s: never observed under the shared rule in %d decodes" % (c.name, n))
                if not c.shared and seen:
                    problems.append(c.name + ": t1_shared set for a decode without solo waves")
                if c.solo and any(not c.solo[0] <= v <= c.solo[1] for v in solo):
                    problems.append("%s: %s solo blocks under the shared rule, built for %d" % (c.name, sorted(solo), c.solo[0]))
            for name in ("2 no solo block", "3 five outliers of 1089"):
                c = [x for x in cases if x.name == name][0]
                if quiet[name] == c.solo[0]:
                    problems.append("%s: the default rule gives the shared rule's split (%d)" % (name, quiet[name]))
            assert not problems, "\n".join(problems)
        finally:
            stop.set()

    try:
        run_threads([occupier, occupier, decoder])
    finally:
        print("occupiers encode %d x %d x %d" % OCCUPIER_SHAPE)
        for k, d in enumerate(duty):
            if d:
                print("occupier %d: %d calls, inside a call %.0f %% of the time" % (k, d[1], 100 * d[0]))
        for line in report:
            print(line)


# ------------------------------------------------- e. engines created and destroyed beside others
def churn():
    import torch
    torch.cuda.init()
    cases = mixed_cases()
    small = smooth(61, 3, 64, 80)
    cs = O.encode(small, 8, numres=3, cblk=(32, 32))
    d = torch.frombuffer(bytearray(cs), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()

    def creator(k, e, sync):
        sync()
        for n in range(20):
            x = G.Engine(0)
            try:
                same(x.decode(d, len(cs)), small, "engine %d of 20, stream on the device" % n)
            finally:
                x.close()
    w = walk(cases, rounds=1, stride=5)
    run_threads([creator, w, w])


SCENARIOS = {"cold": cold, "mixed": mixed, "sticky": sticky, "pool": pool, "shared": shared, "churn": churn}


def main(name, *args):
    t0 = time.monotonic()
    SCENARIOS[name](*args)
    print("ok %s %s %.1f s" % (name, " ".join(args), time.monotonic() - t0))
