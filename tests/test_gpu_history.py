"""A result must not depend on what the engine did before.

One engine (gk_ctx) serves every call and keeps a cached plan, the quantisation last applied to it,
the uploaded block table, its device and pinned buffers, the sticky decode settings and flags set
during a call ("What an engine carries between calls").  Every test here makes a prior
call A on the module's shared engine, then the call B under test: B's result equals the oracle's,
bit for bit, and equals B on an engine created for the test and closed after it.  The oracle is
the judge; the fresh engine only says whether a miss comes from the history or from B itself.
`order` runs each pair as (A, B) and as (B, A, B).

Families: A staged codeword bytes (bytes, hstage2, dout), B coefficient planes (arena) under
calls that leave blocks undecoded, C plan cache and quantisation, D sticky settings, E encode and
decode interleaved, F refused calls.  No call here feeds a kernel corrupt data."""
import ctypes
import functools

import numpy as np
import pytest

import grok_amd as G
import oracle as O
import display_ref as R
import jp2_boxes as J
import test_coc
import tile_coding as TC

pytestmark = pytest.mark.gpu
ORDERS = ["AB", "BAB"]


@pytest.fixture(scope="module")
def eng():
    e = G.Engine(0)
    yield e
    e.close()


# ------------------------------------------------------------------------------------ helpers
def _gk(kw):
    """oracle.encode keywords -> grok_amd.default_params."""
    k = dict(kw)
    for a, b in (("numres", "numresolution"), ("nlayers", "numlayers")):
        if a in k:
            k[b] = k.pop(a)
    if "layer_rate" in k:
        k["numlayers"] = len(k["layer_rate"])
    return G.default_params(**k)


def _noise(c, h, w, bits=8, seed=1):
    return np.random.default_rng(seed).integers(0, 1 << bits, size=(c, h, w)).astype(np.int32)


def _img(seed, c, h, w, bits=8):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (np.sin(xx / 9.0 + seed) * np.cos(yy / 7.0) + 1) * (1 << (bits - 2))
    return np.clip(base[None].repeat(c, 0) + rng.integers(0, 1 << (bits - 3), size=(c, h, w)), 0,
                   (1 << bits) - 1).astype(np.int32)


def _dev(cs):
    import torch
    return torch.frombuffer(bytearray(cs), dtype=torch.uint8).cuda()


def _same(a, b):
    a, b = list(a), list(b)
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _eq(got, want, what):
    got, want = list(got), list(want)
    assert len(got) == len(want), what
    for c, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, err_msg="%s (component %d)" % (what, c))


def _fresh(call):
    e = G.Engine(0)
    try:
        return call(e)
    finally:
        e.close()


def _judge(eng, call, want, what):
    """B on the shared engine equals the oracle (the judge); B on a fresh engine does too."""
    got = call(eng)
    fresh = _fresh(call)
    _eq(got, want, "%s on the used engine; a fresh engine %s the oracle" %
        (what, "equals" if _same(fresh, want) else "also misses"))
    _eq(fresh, want, what + " on a fresh engine")
    return got


def _sequence(eng, order, prior, call, want, what):
    if order == "BAB":
        _judge(eng, call, want, what + ", first")
    prior(eng)
    return _judge(eng, call, want, what + " after the prior call")


def _oracle(cs, partial=False, layers=0, reduce=0):
    O.set_decode_layers(layers)
    O.set_decode_reduce(reduce)
    try:
        return O.decode(cs, partial=partial)[0]
    finally:
        O.set_decode_layers(0)
        O.set_decode_reduce(0)


# ------------------------------------------------------------------------------- prior calls
@functools.lru_cache(maxsize=None)
def poison_streams():
    """name -> (stream, its decode): prior calls that leave hostile bytes behind.  P1: lossless 5/3
    of 3 x 192 x 256 uniform 8-bit noise, whose staged bytes are dense, almost free of 0xFF (the MQ
    coder stuffs a bit after one) and more than any B stages; P2: the same noise coded as HT;
    P3: 12 bits, 9/7, 3 layers."""
    n = _noise(3, 192, 256)
    p1 = O.encode(n, 8)
    p2 = O.encode(n, 8, cblk_sty=0x40)
    p3 = O.encode(_img(3, 3, 192, 256, 12), 12, irreversible=True, layer_rate=[40, 20, 10])
    return {"P1": (p1, n), "P2": (p2, n), "P3": (p3, O.decode(p3)[0])}


def _poison(name):
    cs, want = poison_streams()[name]

    def prior(e):
        _eq(e.decode(cs), want, "prior call " + name)
    return prior


# ------------------------------------------------------------ A: staged codeword bytes
# name -> (stream, whole decode, partial-rule decode, window).  The window selects under half of
# the file's bytes where the stream has tiles or many blocks, which takes the host-gathered staging
# (a pass of one tile of the tile-coded streams is that small even for a whole decode); in
# part1_coc_under_ht it lies in tile 1, whose components are Part-1 under the HT COD.
@functools.lru_cache(maxsize=None)
def _a_case(name):
    win = (0, 0, 16, 16)
    if name in ("part1_under_ht", "ht_and_part1", "mode_switches"):
        cs = test_coc.stream(name)
    elif name in ("part1_coc_under_ht", "part1_tile_under_ht"):
        cs = TC.stream(name)
        np.testing.assert_array_equal(O.decode(cs)[0], TC.expected(name))
        if name == "part1_coc_under_ht":
            win = (80, 0, 96, 16)
    elif name == "plain_4x4":
        cs = O.encode(_img(11, 3, 64, 80), 8, numres=3, cblk=(4, 4))
    elif name == "bypass":
        cs = O.encode(_img(12, 1, 64, 80, 16), 16, numres=3, cblk=(32, 32), cblk_sty=0x01, tiles=(40, 32))
    elif name == "segsym":
        cs = O.encode(_img(13, 3, 64, 80), 8, numres=3, cblk=(32, 32), cblk_sty=0x20, tiles=(40, 32))
    else:
        raise KeyError(name)
    return cs, O.decode(cs)[0], O.decode(cs, partial=True)[0], win


A_CASES = ["part1_under_ht", "part1_coc_under_ht", "part1_tile_under_ht", "ht_and_part1", "mode_switches", "plain_4x4",
           "bypass", "segsym"]
MODES = ["host", "device", "window"]


def _a_call(name, mode):
    cs, whole, part, win = _a_case(name)
    x0, y0, x1, y1 = win
    if mode == "host":
        return (lambda e: e.decode(cs)), whole
    if mode == "device":
        return (lambda e: e.decode(_dev(cs), len(cs))), whole
    return (lambda e: e.decode_window(cs, win)), [p[y0:y1, x0:x1] for p in part]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("prior", ["P1", "P2"])
@pytest.mark.parametrize("name", A_CASES)
def test_staged_bytes(eng, name, prior, mode, order):
    call, want = _a_call(name, mode)
    _sequence(eng, order, _poison(prior), call, want, "%s (%s stream)" % (name, mode))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("prior", ["P1", "P2"])
@pytest.mark.parametrize("name,tile", [("part1_coc_under_ht", 1), ("part1_tile_under_ht", 3)])
def test_staged_bytes_whole_part1_tile_window(eng, name, tile, prior, order):
    # one whole Part-1 tile of four through the window call: a quarter of the file's bytes (the
    # host-gathered staging) and every block of the tile decoded, not the few a 16 x 16 window reaches
    cs, whole, part, win = _a_case(name)
    x0, y0, x1, y1 = TC.tile_rects(name)[tile]
    _sequence(eng, order, _poison(prior), lambda e: e.decode_window(cs, (x0, y0, x1, y1)),
              [p[y0:y1, x0:x1] for p in part], "%s tile %d" % (name, tile))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", A_CASES)
def test_staged_bytes_same_after_either_prior(eng, name, mode):
    call, want = _a_call(name, mode)
    _poison("P1")(eng)
    a = call(eng)
    _poison("P2")(eng)
    b = call(eng)
    _eq(a, b, "%s (%s stream) after P1 and after P2" % (name, mode))
    _eq(a, want, "%s (%s stream) after P1" % (name, mode))


# ------------------------------------------------------------ B: coefficient planes
# The prior call decodes noise coded with B's own parameters, so the plan is reused and the arena
# holds foreign coefficients at the addresses of the blocks that B leaves undecoded.
B_SHAPE = (3, 96, 120)
B_BASE = dict(numres=4, cblk=(32, 32))
B_CODERS = {"53": dict(), "97": dict(irreversible=True), "ht": dict(cblk_sty=0x40)}
B_TILES = (64, 48)
B_WINDOWS = {"window": (7, 5, 45, 39), "window_last": (87, 69, 120, 96), "tile": (64, 48, 120, 96)}
B_CALLS = ["layers1", "patch", "reduce1", "reduce2", "window", "window_last", "tile"]


@functools.lru_cache(maxsize=None)
def _b_case(coder, what):
    """(prior stream, its decode, B stream, B's expected result)."""
    c, h, w = B_SHAPE
    kw = dict(B_BASE, **B_CODERS[coder])
    if what == "layers1":
        # (HT blocks carry one cleanup pass here: the layers beyond the first hold empty packets)
        kw["layer_rate"] = [30, 10, 0]
    if what == "tile":
        kw["tiles"] = B_TILES
    img = _img(21, c, h, w)
    if what == "patch":   # constant outside one 40 x 40 patch: empty code-blocks (numbps 0)
        img = np.full((c, h, w), 100, np.int32)
        img[:, 20:60, 30:70] = _noise(c, 40, 40, seed=5)
    prior = O.encode(_noise(c, h, w, seed=9), 8, **kw)
    cs = O.encode(img, 8, **kw)
    if what == "layers1":
        want = _oracle(cs, layers=1)
    elif what in ("reduce1", "reduce2"):
        want = _oracle(cs, reduce=int(what[-1]))
    elif what in B_WINDOWS:
        x0, y0, x1, y1 = B_WINDOWS[what]
        want = _oracle(cs, partial=True)[:, y0:y1, x0:x1]
    else:
        want = _oracle(cs)
    return prior, O.decode(prior)[0], cs, want


def _b_call(cs, what):
    def call(e):
        if what == "layers1":
            e.set_decode_layers(1)
        elif what in ("reduce1", "reduce2"):
            e.set_decode_reduce(int(what[-1]))
        try:
            return e.decode_window(cs, B_WINDOWS[what]) if what in B_WINDOWS else e.decode(cs)
        finally:
            e.set_decode_layers(0)
            e.set_decode_reduce(0)
    return call


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("what", B_CALLS)
@pytest.mark.parametrize("coder", sorted(B_CODERS))
def test_coefficient_planes(eng, coder, what, order):
    prior, prior_want, cs, want = _b_case(coder, what)
    _sequence(eng, order, lambda e: _eq(e.decode(prior), prior_want, "prior call"), _b_call(cs, what), want,
              "%s %s" % (coder, what))


# ------------------------------------------------------------ C: plan cache and quantisation
# Pairs of one plan_key that differ in what the key leaves out.  name -> (X keywords, Y keywords).
C_SHAPE = (3, 80, 96)
C_BASE = dict(numres=4, cblk=(32, 32))
C_PAIRS = {
    "layers": (dict(), dict(layer_rate=[30, 10, 0])),
    "sop_eph": (dict(), dict(sop=True, eph=True)),
    "order": (dict(), dict(prog_order="RPCL")),
    "plt_tlm": (dict(), dict(plt=True, tlm=True)),
    "qderived": (dict(irreversible=True), dict(irreversible=True, qderived=True)),
    "qcc_qshift": (dict(irreversible=True), dict(irreversible=True, comp_qshift=[0, 1, 2])),
    "qcc_guard_bits": (dict(), dict(comp_guard_bits=[2, 1, 3])),
}
ORACLE_ONLY = ("qderived", "comp_qshift", "comp_guard_bits")   # (the engine's encoder writes one expounded QCD)


@functools.lru_cache(maxsize=None)
def _c_stream(name, which):
    kw = dict(C_BASE, **C_PAIRS[name][which])
    img = _img(31 + which, *C_SHAPE)
    cs = O.encode(img, 8, **kw)
    return kw, img, cs, O.decode(cs)[0]


@pytest.mark.parametrize("swap", [False, True], ids=["XY", "YX"])
@pytest.mark.parametrize("name", sorted(C_PAIRS))
def test_plan_cache_pair(eng, name, swap):
    (kw1, img1, cs1, want1), (kw2, img2, cs2, want2) = _c_stream(name, int(swap)), _c_stream(name, int(not swap))
    _eq(eng.decode(cs1), want1, "first of the pair")
    _judge(eng, lambda e: e.decode(cs2), want2, "%s: second of the pair after the first" % name)
    # the second's parameters encode to the oracle's bytes after a decode of the first (with a
    # foreign QCD or QCC in the first, the plan's own quantisation has to come back)
    if not any(k in kw2 for k in ORACLE_ONLY):
        _eq(eng.decode(cs1), want1, "first of the pair")
        assert eng.encode(img2, 8, params=_gk(kw2)) == cs2, name + ": encode after decoding the other"


def test_encode_97_after_foreign_qcd(eng):
    # a 9/7 stream with derived steps and per-component shifts, then a 9/7 encode of that geometry
    c, h, w = C_SHAPE
    kw = dict(C_BASE, irreversible=True)
    foreign = O.encode(_img(41, c, h, w), 8, qderived=True, comp_qshift=[0, 2, 1], comp_guard_bits=[2, 2, 1], **kw)
    img = _img(42, c, h, w)
    ref = O.encode(img, 8, **kw)
    for _ in range(2):
        _eq(eng.decode(foreign), O.decode(foreign)[0], "foreign QCD")
        assert eng.encode(img, 8, params=_gk(kw)) == ref
        _eq(eng.decode(ref), O.decode(ref)[0], "own QCD after the foreign one")


def test_alternating_plans(eng):
    # two different keys, three times: the plan is rebuilt and the block table uploaded again
    k1, k2 = dict(numres=3, cblk=(32, 32)), dict(numres=5, irreversible=True)
    i1, i2 = _img(51, 3, 64, 80), _img(52, 1, 97, 131, 12)
    c1, c2 = O.encode(i1, 8, **k1), O.encode(i2, 12, **k2)
    w1, w2 = O.decode(c1)[0], O.decode(c2)[0]
    for n in range(3):
        assert eng.encode(i1, 8, params=_gk(k1)) == c1, n
        _eq(eng.decode(c2), w2, "second key, turn %d" % n)
        assert eng.encode(i2, 12, params=_gk(k2)) == c2, n
        _eq(eng.decode(c1), w1, "first key, turn %d" % n)


# ------------------------------------------------------------ D: sticky settings
@functools.lru_cache(maxsize=None)
def _odd_tiles():
    """5/3 with odd-sized tiles: where the whole-tile inverse (H / 2) and the partial one (H >> 1)
    are different code paths."""
    img = _img(61, 3, 45, 50)
    kw = dict(numres=3, tiles=(13, 7))
    cs = O.encode(img, 8, **kw)
    return kw, img, cs


def _use_layers(e):
    cs = O.encode(_img(62, 3, 64, 80), 8, numres=4, layer_rate=[30, 10, 0])
    e.set_decode_layers(1)
    try:
        _eq(e.decode(cs), _oracle(cs, layers=1), "one layer of three")
    finally:
        e.set_decode_layers(0)


def _use_reduce(e):
    cs = O.encode(_img(63, 3, 64, 80), 8, numres=4, irreversible=True)
    e.set_decode_reduce(1)
    try:
        _eq(e.decode(cs), _oracle(cs, reduce=1), "reduced decode")
    finally:
        e.set_decode_reduce(0)


def _use_window_rule(e):
    kw, img, cs = _odd_tiles()
    e.set_window_rule(True)
    try:
        _eq(e.decode_window(cs, (13, 7, 26, 14)), O.decode(cs)[0][:, 7:14, 13:26], "a tile by the whole-tile rule")
    finally:
        e.set_window_rule(False)


def _use_colour(e):
    c = J.cases()["c1_clamp200"]
    e.set_decode_colour(False)
    try:
        _eq(e.decode(c.file), c.src, "components of a palette file")
    finally:
        e.set_decode_colour(True)
    _eq(e.decode(c.file), c.want, "palette applied again")


def _use_display(e):
    c = J.cases()["c7_sycc"]   # 4:4:4 sYCC, lossless: the components are the source planes
    nc, h, w = c.src.shape
    planes = R.post_process(list(c.src), [(1, 1, 8, 0)] * nc, R.CS_SYCC, (0, 0, w, h), True, False)[0]
    e.set_decode_display(rgb=True)
    try:
        _eq(e.decode(c.file), planes, "sYCC to RGB")
    finally:
        e.set_decode_display()
    _eq(e.decode(c.file), c.src, "display off again")


SETTINGS = {"layers": _use_layers, "reduce": _use_reduce, "window_rule": _use_window_rule, "colour": _use_colour,
            "display": _use_display}


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_settings_return_to_neutral(eng, setting, order):
    kw, img, cs = _odd_tiles()
    want = O.decode(cs)[0]
    np.testing.assert_array_equal(want, img)
    _sequence(eng, order, SETTINGS[setting], lambda e: e.decode(cs), want, "odd tiles after " + setting)
    assert eng.encode(img, 8, params=_gk(kw)) == cs


@functools.lru_cache(maxsize=None)
def _single_odd_sample(tw):
    """Tiles `tw` wide and 3 levels leave one-sample-wide resolutions on odd coordinates; a lossy 5/3
    layer of signed noise leaves odd negative high-pass samples there (tests/window_rule_case.py)."""
    h, rate, seed = {1: (128, 0.8, 0), 3: (96, 1.1, 2)}[tw]   # (found by search: the two rules differ)
    img = np.random.default_rng(seed).integers(-128, 128, size=(1, h, 8 * tw)).astype(np.int32)
    cs = O.encode(img, 8, signed=True, numres=4, tiles=(tw, h), layer_rate=[rate])
    return cs, O.decode(cs)[0], O.decode(cs, partial=True)[0]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("tw", [1, 3])
def test_whole_decode_after_a_partial_window(eng, tw, order):
    # (the two rules give different samples on these streams, so a flag left by the window would show)
    cs, whole, part = _single_odd_sample(tw)
    assert not np.array_equal(whole, part)
    h, w = whole.shape[1:]
    win = (tw, 0, w, h // 2)

    def prior(e):
        _eq(e.decode_window(cs, win), part[:, :h // 2, tw:], "window by the partial rule")
    _sequence(eng, order, prior, lambda e: e.decode(cs), whole, "whole decode of %d-wide tiles" % tw)


# ------------------------------------------------------------ E: encode and decode interleaved
E_KW = dict(numres=4, cblk=(32, 32))


def test_encode_decode_encode(eng):
    # (the decode stages more bytes than the encode's slots hold)
    img = _img(71, 3, 64, 80)
    ref = O.encode(img, 8, **E_KW)
    big, noise = poison_streams()["P1"]
    fresh = _fresh(lambda e: e.encode(img, 8, params=_gk(E_KW)))
    for n in range(2):
        assert eng.encode(img, 8, params=_gk(E_KW)) == ref, n
        _eq(eng.decode(big), noise, "decode between the encodes")
    assert eng.encode(img, 8, params=_gk(E_KW)) == ref
    assert fresh == ref


def test_encode_tiles_decode_encode_tiles(eng):
    img = _img(72, 3, 80, 96)
    kw = dict(E_KW, tiles=(48, 40))
    ref, lens = O.encode_tile_parts(img, 0, (80, 96), 8, 0, 4, **kw)
    big, noise = poison_streams()["P2"]
    for n in range(2):
        got, gl = eng.encode_tiles(img, 8, 0, 4, params=_gk(kw))
        assert got == ref and list(gl) == list(lens), n
        _eq(eng.decode(big), noise, "decode between the tile encodes")
    got, gl = eng.encode_tiles(img, 8, 0, 4, params=_gk(kw))
    assert got == ref and list(gl) == list(lens)
    assert _fresh(lambda e: e.encode_tiles(img, 8, 0, 4, params=_gk(kw))[0]) == ref


def test_rate_controlled_encode_between_lossless_ones(eng):
    img = _img(73, 3, 64, 80)
    rc = dict(E_KW, irreversible=True, layer_rate=[40, 20, 10])
    ref, ref_rc = O.encode(img, 8, **E_KW), O.encode(img, 8, **rc)
    big, want = poison_streams()["P3"]
    for n in range(2):
        assert eng.encode(img, 8, params=_gk(E_KW)) == ref, n
        assert eng.encode(img, 8, params=_gk(rc)) == ref_rc, n
        _eq(eng.decode(big), want, "decode between the encodes")
    assert eng.encode(img, 8, params=_gk(E_KW)) == ref
    assert _fresh(lambda e: e.encode(img, 8, params=_gk(rc))) == ref_rc


def _encode_blocks(e, img, prec, params):
    """gk_encode_blocks (the T1 plugin's call): (blocks, bytes) counted."""
    c, h, w = img.shape
    a = np.ascontiguousarray(img, np.int32)
    info = G.ImageInfo(w, h, c, prec, 0, 0)
    ptrs = (ctypes.c_void_p * c)(*[a.ctypes.data + k * h * w * 4 for k in range(c)])
    strides = (ctypes.c_uint32 * c)(*([w] * c))
    nbands, nblocks, npasses, nbytes = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
    rc = e.lib.gk_encode_blocks(ctypes.c_void_p(e.ctx), ctypes.byref(info), ptrs, strides, ctypes.c_int(0),
                                ctypes.byref(params), ctypes.byref(nbands), ctypes.byref(nblocks), ctypes.byref(nbytes),
                                ctypes.byref(npasses))
    assert rc == 0, e.lib.gk_last_error(ctypes.c_void_p(e.ctx))
    return nblocks.value, nbytes.value


def test_plain_encode_after_encode_blocks(eng):
    img, other = _img(74, 3, 64, 80), _noise(3, 64, 80, seed=75)
    ref = O.encode(img, 8, **E_KW)
    blocks, data = O.encode_blocks(other, 8, **E_KW)
    assert eng.encode(img, 8, params=_gk(E_KW)) == ref
    nb, nbytes = _encode_blocks(eng, other, 8, _gk(E_KW))
    assert (nb, nbytes) == (len(blocks), sum(int(b.len) for b in blocks))
    assert eng.encode(img, 8, params=_gk(E_KW)) == ref
    _eq(eng.decode(ref), img, "decode after encode_blocks")


# ------------------------------------------------------------ F: refusals leave no trace
# Every call below is refused on the host, before a kernel is launched.
def _refuse_reduce(e, cs):
    e.set_decode_reduce(4)   # (numres 4)
    try:
        with pytest.raises(RuntimeError, match="reduce must be less"):
            e.decode(cs)
    finally:
        e.set_decode_reduce(0)


def _refuse_reduce_under_the_output_stage(e, cs):
    # refused by the component decode, the innermost level, after the output stage has begun
    e.set_decode_reduce(4)   # (numres 4)
    try:
        with pytest.raises(RuntimeError, match="reduce must be less"):
            e.decode_pixels(cs, sample_bytes=1)
    finally:
        e.set_decode_reduce(0)


def _refuse_window(e, cs):
    with pytest.raises(RuntimeError, match="bad decode window"):
        e.decode_window(cs, (90, 70, 104, 88))   # (past the 96 x 80 image)


def _refuse_truncated_header(e, cs):
    with pytest.raises(RuntimeError):
        e.decode(cs[:60])   # (ends inside the main header: SIZ is 49 bytes, then COD)


def _refuse_jp2h(e, cs):
    for name in ("truncated_pclr", "two_cmap", "cdef_incomplete"):
        data, box = J.malformed()[name]
        with pytest.raises(RuntimeError, match=box):
            e.decode(data)


def _refuse_display(e, cs):
    # upsampling at a reduced resolution is a refused layout (gk_probe_display says the same)
    e.set_decode_display(upsample=True)
    e.set_decode_reduce(1)
    try:
        with pytest.raises(ValueError, match="reduced resolution"):
            G.probe_display(cs, upsample=True, reduce=1)
        with pytest.raises(RuntimeError, match="reduced resolution"):
            e.decode(cs)
    finally:
        e.set_decode_display()
        e.set_decode_reduce(0)


REFUSALS = {"reduce": _refuse_reduce, "window": _refuse_window, "truncated_header": _refuse_truncated_header,
            "jp2h": _refuse_jp2h, "display": _refuse_display, "reduce_in_pixels": _refuse_reduce_under_the_output_stage}


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("refusal", sorted(REFUSALS))
def test_refusal_leaves_no_trace(eng, refusal, order):
    img = _img(81, 3, 80, 96)
    cs = O.encode(img, 8, **E_KW)
    _sequence(eng, order, lambda e: REFUSALS[refusal](e, cs), lambda e: e.decode(cs), img, "decode after a refused " + refusal)
    REFUSALS[refusal](eng, cs)
    assert eng.encode(img, 8, params=_gk(E_KW)) == cs
