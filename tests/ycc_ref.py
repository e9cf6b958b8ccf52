"""NumPy restatement of the engine's forward colour conversion (k_rgb_ycc, gk_rgbycc.hip; the
arithmetic of include/grok_amd.h's gk_encode_convert and DESIGN.md §3): R, G, B to sYCC with the
chroma planes on the 4:4:4, 4:2:2 or 4:2:0 grid.  Grok has no forward conversion to restate (its
CLI takes subsampled raw YUV), so this file IS the definition, in integers:

  Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
  Cb = floor((-11059 SR - 21709 SG + 32768 SB + 2^(s-1)) / 2^s) + offset, clamped to [0, upb]
  Cr = floor(( 32768 SR - 27439 SG -  5329 SB + 2^(s-1)) / 2^s) + offset, clamped to [0, upb]

SR, SG, SB the sums over the chroma sample's box of n = 1, 2 or 4 pixels, s = 16 + log2(n).  Python
integers / int64 throughout: `>>` and `//` floor."""
import numpy as np

KY = (19595, 38470, 7471)
KB = (-11059, -21709, 32768)
KR = (32768, -27439, -5329)
assert sum(KY) == 65536 and sum(KB) == 0 and sum(KR) == 0

S444, S422, S420 = (1, 1), (2, 1), (2, 2)


def luma(r, g, b):
    r, g, b = (np.asarray(v, np.int64) for v in (r, g, b))
    return (KY[0] * r + KY[1] * g + KY[2] * b + 32768) >> 16


def chroma(sr, sg, sb, n, prec, clamp=True):
    """(Cb, Cr) of boxes of n pixels (an array or a scalar: 1, 2 or 4) whose sums are sr, sg, sb."""
    sr, sg, sb, n = (np.asarray(v, np.int64) for v in (sr, sg, sb, n))
    assert np.isin(n, (1, 2, 4)).all()
    s = 16 + (n >> 1)                       # 16 + log2(n)
    half = np.int64(1) << (s - 1)
    offset, upb = 1 << (prec - 1), (1 << prec) - 1
    cb = ((KB[0] * sr + KB[1] * sg + KB[2] * sb + half) >> s) + offset
    cr = ((KR[0] * sr + KR[1] * sg + KR[2] * sb + half) >> s) + offset
    if clamp:
        cb, cr = np.clip(cb, 0, upb), np.clip(cr, 0, upb)
    return cb, cr


def chroma_shape(w, h, chroma_sub, origin=(0, 0)):
    dx, dy = chroma_sub
    ofx = origin[0] & 1 if dx == 2 else 0
    ofy = origin[1] & 1 if dy == 2 else 0
    return -(-(h - ofy) // dy), -(-(w - ofx) // dx)


def rgb_to_ycc(rgb, prec, chroma_sub=S444, origin=(0, 0)):
    """rgb: (H, W, 3) unsigned samples of `prec` bits -> [Y (H, W), Cb, Cr (chroma_shape)] int32.
    Column 0 under an odd x0 and row 0 under an odd y0 (on a subsampled axis) belong to no box."""
    rgb = np.asarray(rgb).astype(np.int64)
    assert rgb.ndim == 3 and rgb.shape[2] == 3 and 1 <= prec <= 16
    assert rgb.min() >= 0 and rgb.max() < (1 << prec)
    assert tuple(chroma_sub) in (S444, S422, S420)
    h, w, _ = rgb.shape
    dx, dy = chroma_sub
    ofx = origin[0] & 1 if dx == 2 else 0
    ofy = origin[1] & 1 if dy == 2 else 0
    y = luma(rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2])
    ch, cw = chroma_shape(w, h, chroma_sub, origin)
    if (dx, dy) == S444:
        cb, cr = chroma(rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2], 1, prec)
        return [y.astype(np.int32), cb.astype(np.int32), cr.astype(np.int32)]
    # the box sums: the image from (ofx, ofy) on, padded with zeros to whole boxes
    body = rgb[ofy:, ofx:, :]
    pad = np.zeros((ch * dy, cw * dx, 3), np.int64)
    pad[:body.shape[0], :body.shape[1], :] = body
    cnt = np.zeros((ch * dy, cw * dx), np.int64)
    cnt[:body.shape[0], :body.shape[1]] = 1
    sums = pad.reshape(ch, dy, cw, dx, 3).sum(axis=(1, 3))
    n = cnt.reshape(ch, dy, cw, dx).sum(axis=(1, 3))
    if n.size:
        cb, cr = chroma(sums[:, :, 0], sums[:, :, 1], sums[:, :, 2], n, prec)
    else:
        cb = cr = np.zeros((ch, cw), np.int64)
    return [y.astype(np.int32), cb.astype(np.int32), cr.astype(np.int32)]


def subsampling(chroma_sub):
    """The [(dx, dy)] list of the planar encode of rgb_to_ycc's planes."""
    return [(1, 1), tuple(chroma_sub), tuple(chroma_sub)]


def box_constant(rng, w, h, prec, chroma_sub=S420, origin=(0, 0)):
    """(H, W, 3) random pixels that are constant on each chroma box (and grey in front of the first
    box: those pixels are converted back without a chroma sample)."""
    dx, dy = chroma_sub
    ofx = origin[0] & 1 if dx == 2 else 0
    ofy = origin[1] & 1 if dy == 2 else 0
    ch, cw = chroma_shape(w, h, chroma_sub, origin)
    cells = rng.randint(0, 1 << prec, (max(ch, 1), max(cw, 1), 3))
    img = np.repeat(np.repeat(cells, dy, axis=0), dx, axis=1)
    out = np.empty((h, w, 3), np.int64)
    grey = rng.randint(0, 1 << prec, (h, w))
    out[:, :, :] = grey[:, :, None]
    out[ofy:, ofx:, :] = img[:h - ofy, :w - ofx, :]
    return out
