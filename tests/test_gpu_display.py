"""Display stage on the GPU (Engine.set_decode_display: k_ycc_rgb, k_cmyk_rgb, k_upsample): every
decode under the flags equals the restatement (tests/display_ref.py) applied to the same engine's
flag-0 decode of the same bytes.  Inputs are lossless 5/3 streams without MCT from eng.encode.

Of the issue's pairing cases none has an empty chroma plane (the smallest, 1 x 1 at (0, 0) and
2 x 2 at (1, 1), keep one chroma sample), so none is dropped."""
import numpy as np
import pytest
import torch

import grok_amd as G
import display_ref as R
import display_cases as C

pytestmark = pytest.mark.gpu
CS_OF = {C.SYCC: R.CS_SYCC, C.EYCC: R.CS_EYCC, C.CMYK: R.CS_CMYK, None: R.CS_UNKNOWN}


@pytest.fixture(scope="module")
def eng():
    e = G.Engine(0)
    yield e
    e.close()


class Img:
    """One encoded image: the file bytes and what is needed to restate its post-processing."""

    def __init__(self, eng, planes, w, h, sub, prec, origin=(0, 0), enumcs=None, signed=False, numres=None):
        self.w, self.h, self.sub, self.prec, self.origin, self.signed = w, h, sub, prec, origin, signed
        self.comps = [(dx, dy, prec, int(signed)) for dx, dy in sub]
        self.space = CS_OF[enumcs]
        p = G.default_params(numresolution=numres or C.numres_for(w, h, sub), mct=False)
        if all(d == (1, 1) for d in sub):
            cs = eng.encode(np.stack(planes).astype(np.int32), prec, signed=signed, params=p, origin=origin)
        else:
            cs = eng.encode([np.ascontiguousarray(x, np.int32) for x in planes], prec, signed=signed, params=p, origin=origin,
                            subsampling=sub, size=(w, h))
        self.file = cs if enumcs is None else C.wrap(cs, w, h, len(sub), prec, enumcs, signed)
        self.bounds = (origin[0], origin[1], origin[0] + w, origin[1] + h)

    def want(self, eng, rgb, upsample):
        """(restated planes stacked, colour space) from the engine's flag-0 decode."""
        eng.set_decode_display()
        got = eng.decode(self.file)
        planes, _, cs, _, _ = R.post_process(list(got), self.comps, self.space, self.bounds, rgb, upsample)
        return np.stack(planes), cs


def _check(eng, im, rgb=True, upsample=False, want_space=R.CS_SRGB):
    want, cs = im.want(eng, rgb, upsample)
    assert cs == want_space
    eng.set_decode_display(rgb=rgb, upsample=upsample)
    try:
        got = eng.decode(im.file)
        assert isinstance(got, np.ndarray) and got.dtype == np.int32
        np.testing.assert_array_equal(got, want)
        assert eng.colour_info().colour_space == want_space
    finally:
        eng.set_decode_display()
    return want


def test_sycc444_every_chroma_pair_8bit(eng):
    yy, xx = np.mgrid[0:256, 0:256]
    y = np.random.RandomState(1).randint(0, 256, (256, 256))
    im = Img(eng, [y, xx, yy], 256, 256, C.S444, 8, enumcs=C.SYCC)
    want = _check(eng, im)
    assert want.min() == 0 and want.max() == 255   # (the clamp works at both ends)


def test_sycc444_16bit_every_term(eng):
    rng = np.random.RandomState(2)
    every = np.arange(65536).reshape(256, 256)
    rnd = lambda: rng.randint(0, 65536, (256, 256))
    # r over every Cr, b over every Cb, g over 2^16 random pairs and the four corners
    _check(eng, Img(eng, [rnd(), rnd(), every], 256, 256, C.S444, 16, enumcs=C.SYCC))
    _check(eng, Img(eng, [rnd(), every, rnd()], 256, 256, C.S444, 16, enumcs=C.SYCC))
    cb, cr = rnd(), rnd()
    cb.flat[:4], cr.flat[:4] = [0, 0, 65535, 65535], [0, 65535, 0, 65535]
    y = rnd()
    y.flat[:4] = 32768
    _check(eng, Img(eng, [y, cb, cr], 256, 256, C.S444, 16, enumcs=C.SYCC))


@pytest.mark.parametrize("signed", [False, True], ids=["unsigned", "signed"])
def test_esycc_every_chroma_pair_8bit(eng, signed):
    yy, xx = np.mgrid[0:256, 0:256]
    off = 128 if signed else 0
    y = np.random.RandomState(3).randint(0, 256, (256, 256)) - off
    _check(eng, Img(eng, [y, xx - off, yy - off], 256, 256, C.S444, 8, enumcs=C.EYCC, signed=signed))


@pytest.mark.parametrize("prec", [8, 12])
@pytest.mark.parametrize("dims", [(33, 17, 0, 0), (34, 18, 1, 1), (33, 18, 1, 0), (2, 2, 1, 1), (1, 1, 0, 0), (2051, 5, 1, 0)],
                         ids=lambda d: "%dx%d@%d,%d" % d)
@pytest.mark.parametrize("sub", [C.S420, C.S422], ids=["420", "422"])
def test_sycc_pairing_and_tails(eng, sub, dims, prec):
    w, h, x0, y0 = dims
    planes = C.random_planes(w, h, sub, prec, (x0, y0), seed=w + h + prec)
    _check(eng, Img(eng, planes, w, h, sub, prec, (x0, y0), enumcs=C.SYCC))


@pytest.mark.parametrize("prec", [8, 16])
def test_cmyk(eng, prec):
    sub = [(1, 1)] * 4
    planes = C.random_planes(37, 19, sub, prec, seed=prec)
    for k in range(4):   # the ends of the range, where the float quotient meets 1
        planes[k].flat[:2] = [0, (1 << prec) - 1]
    im = Img(eng, planes, 37, 19, sub, prec, enumcs=C.CMYK)
    want = _check(eng, im)
    assert want.shape == (3, 19, 37)
    eng.set_decode_display(rgb=True)
    try:
        assert eng.read_header(im.file).prec == 8
        np.testing.assert_array_equal(eng.decode(im.file, sample_bytes=1), want.astype(np.uint8))
        if prec == 16:   # planes sized for the components, not for the 8-bit output
            with pytest.raises(RuntimeError, match="output planes"):
                eng.decode(im.file, sample_bytes=2)
    finally:
        eng.set_decode_display()


@pytest.mark.parametrize("origin", [(0, 0), (1, 1)])
@pytest.mark.parametrize("d", [(2, 2), (3, 2), (1, 4)])
def test_upsample(eng, d, origin):
    sub = [(1, 1), d, d]
    planes = C.random_planes(37, 19, sub, 8, origin, seed=sum(d))
    im = Img(eng, planes, 37, 19, sub, 8, origin)
    want = _check(eng, im, rgb=False, upsample=True, want_space=R.CS_UNKNOWN)
    assert want.shape == (3, 19, 37)


def test_both_flags(eng):
    # 4:2:0: converted, nothing left to upsample; dx = 4 sYCC: no conversion, upsampled YCC
    planes = C.random_planes(37, 19, C.S420, 8, (1, 1), seed=5)
    _check(eng, Img(eng, planes, 37, 19, C.S420, 8, (1, 1), enumcs=C.SYCC), rgb=True, upsample=True)
    sub = [(1, 1), (4, 1), (4, 1)]
    planes = C.random_planes(37, 19, sub, 8, seed=6)
    im = Img(eng, planes, 37, 19, sub, 8, enumcs=C.SYCC)
    _check(eng, im, rgb=True, upsample=True, want_space=R.CS_SYCC)
    # rgb alone leaves that file as it is: the subsampled planes
    eng.set_decode_display(rgb=True)
    try:
        got = eng.decode(im.file)
        assert isinstance(got, list) and [g.shape for g in got] == [(19, 37), (19, 10), (19, 10)]
        for g, p in zip(got, planes):
            np.testing.assert_array_equal(g, p)
        ci = eng.colour_info()
        assert (ci.colour_space, ci.display_applied) == (R.CS_SYCC, 0)
    finally:
        eng.set_decode_display()


@pytest.fixture(scope="module")
def im420(eng):
    planes = C.random_planes(34, 18, C.S420, 8, (1, 1), seed=8)
    im = Img(eng, planes, 34, 18, C.S420, 8, (1, 1), enumcs=C.SYCC)
    return im, im.want(eng, True, False)[0]


def test_sample_types_and_placement(eng, im420):
    im, want = im420
    w, h = im.w, im.h
    d = torch.from_numpy(np.frombuffer(im.file, np.uint8).copy()).cuda()
    eng.set_decode_display(rgb=True)
    try:
        assert eng.decode(im.file).dtype == np.int32
        got = eng.decode(im.file, sample_bytes=1)
        assert got.dtype == np.uint8
        np.testing.assert_array_equal(got, want)
        with pytest.raises(RuntimeError, match="output planes"):
            eng.decode(im.file, sample_bytes=2)
        for dt in (torch.uint8, torch.int32):
            y = torch.zeros((3, h, w), dtype=dt, device="cuda")
            eng.decode(d, length=len(im.file), out=y)
            np.testing.assert_array_equal(y.cpu().numpy(), want.astype(y.cpu().numpy().dtype))
        # a view whose base offset (3 samples) and row stride (w + 5 = 39) are no multiples of the
        # kernel's vector: the scalar-store path; what surrounds the view stays untouched
        for dt, fill in ((torch.uint8, 77), (torch.int32, -5)):
            buf = torch.full((3, h, w + 5), fill, dtype=dt, device="cuda")
            eng.decode_window(d, (0, 0, w, h), length=len(im.file), out=buf[:, :, 3:3 + w])
            got = buf.cpu().numpy()
            np.testing.assert_array_equal(got[:, :, 3:3 + w], want.astype(got.dtype))
            assert (got[:, :, :3] == fill).all() and (got[:, :, 3 + w:] == fill).all()
    finally:
        eng.set_decode_display()


def test_sixteen_bit_planes(eng):
    planes = C.random_planes(34, 18, C.S422, 12, seed=9)
    im = Img(eng, planes, 34, 18, C.S422, 12, enumcs=C.SYCC)
    want = im.want(eng, True, False)[0]
    eng.set_decode_display(rgb=True)
    try:
        got = eng.decode(im.file, sample_bytes=2)
        assert got.dtype == np.uint16
        np.testing.assert_array_equal(got, want)
        y = torch.zeros((3, 18, 34), dtype=torch.int16, device="cuda")
        eng.decode(im.file, out=y)
        np.testing.assert_array_equal(y.cpu().numpy().view(np.uint16), want.astype(np.uint16))
    finally:
        eng.set_decode_display()


def test_reduce_window_and_flags_off_again(eng):
    planes = C.random_planes(64, 48, C.S420, 8, seed=10)
    im = Img(eng, planes, 64, 48, C.S420, 8, enumcs=C.SYCC, numres=3)
    post = lambda comps: np.stack(R.post_process(list(comps), im.comps, im.space, (0, 0, 0, 0), True, False, odd_first=(0, 0))[0])
    win = (16, 8, 48, 40)
    eng.set_decode_reduce(1)
    try:
        want_red = post(eng.decode(im.file))
        eng.set_decode_display(rgb=True)
        got = eng.decode(im.file)
        assert got.shape == (3, 24, 32)
        np.testing.assert_array_equal(got, want_red)
        eng.set_decode_display(rgb=True, upsample=True)
        with pytest.raises(RuntimeError, match="reduced resolution"):
            eng.decode(im.file)
    finally:
        eng.set_decode_display()
        eng.set_decode_reduce(0)
    want_win = post(eng.decode_window(im.file, win))
    eng.set_decode_display(rgb=True)
    try:
        got = eng.decode_window(im.file, win)
        assert got.shape == (3, 32, 32)
        np.testing.assert_array_equal(got, want_win)
        np.testing.assert_array_equal(got, eng.decode(im.file)[:, 8:40, 16:48])
        with pytest.raises(RuntimeError, match="do not pair"):   # an odd left edge
            eng.decode_window(im.file, (17, 8, 48, 40))
    finally:
        eng.set_decode_display()
    # flags 0 after flags set: the three component planes again
    got = eng.decode(im.file)
    assert isinstance(got, list) and [g.shape for g in got] == [(48, 64), (24, 32), (24, 32)]
    for g, p in zip(got, planes):
        np.testing.assert_array_equal(g, p)
    assert eng.colour_info().colour_space == R.CS_SYCC


def test_some_tiles_only_is_refused(eng):
    planes = C.random_planes(64, 48, C.S420, 8, seed=11)
    p = G.default_params(numresolution=3, mct=False, tiles=(32, 32))
    hdr, body, _ = eng.encode_tiles_subsampled(planes, 8, 0, 2, C.S420, (64, 48), params=p)
    part = hdr + body + b"\xff\xd9"
    eng.set_decode_display(rgb=True)
    try:
        with pytest.raises(RuntimeError, match="only some of its tiles"):
            eng.decode(part)
    finally:
        eng.set_decode_display()
