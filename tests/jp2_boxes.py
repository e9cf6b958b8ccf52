"""JP2 files with colour boxes (jp2h: colr, pclr, cmap, cdef) built by hand around oracle-encoded
codestreams, a numpy restatement of what Grok's library makes of them on decode
(FileFormatDecompress::apply_palette_clr :1299-1436, apply_channel_definition :876-930), and a
JP2 decode through OpenJPEG (Pillow's libopenjp2, codec 2) that pins the restatement.

The case list is shared by the CPU tests (restatement against OpenJPEG, header probes) and the
GPU tests (engine against the restatement).  Sources are coded losslessly, so every expectation
is built from the source samples alone.  Test infrastructure only."""
import ctypes
import functools
import glob
import os
import struct
import tempfile

import numpy as np

import oracle as O

# GRK_COLOR_SPACE (grk_abi.h) / OPJ_COLOR_SPACE (openjpeg.h) by colr EnumCS
GRK_CLRSPC = {None: 0, 0: 0, 16: 2, 17: 3, 18: 4, 24: 5, 12: 6, "icc": 9}
OPJ_CLRSPC = {16: 1, 17: 2, 18: 3, 24: 4, 12: 5}


# ------------------------------------------------------------------------------ boxes
def box(typ, payload):
    return struct.pack(">I4s", 8 + len(payload), typ.encode()) + payload


def ihdr(h, w, nc, prec, signed=False):
    return box("ihdr", struct.pack(">IIHBBBB", h, w, nc, (prec - 1) | (0x80 if signed else 0), 7, 0, 0))


def colr_enum(cs):
    return box("colr", struct.pack(">BBBI", 1, 0, 0, cs))


def colr_icc(profile):
    return box("colr", struct.pack(">BBB", 2, 0, 0) + bytes(profile))


def pclr(lut, precs, signed=None, ne=None, truncate=0):
    """lut: (NE, NPC) array; precs: column precisions.  ne overrides the NE field; truncate drops
    that many bytes from the end of the entries."""
    lut = np.asarray(lut)
    n, npc = lut.shape
    signed = signed or [False] * npc
    b = struct.pack(">HB", n if ne is None else ne, npc)
    b += bytes(((p - 1) | (0x80 if s else 0)) for p, s in zip(precs, signed))
    ent = bytearray()
    for j in range(n):
        for i in range(npc):
            ent += int(lut[j, i]).to_bytes((precs[i] + 7) // 8, "big")
    if truncate:
        ent = ent[:-truncate]
    return box("pclr", b + bytes(ent))


def cmap(entries):
    """entries: [(CMP, MTYP, PCOL)]"""
    return box("cmap", b"".join(struct.pack(">HBB", c, m, p) for c, m, p in entries))


def cdef(entries):
    """entries: [(Cn, Typ, Asoc)]"""
    return box("cdef", struct.pack(">H", len(entries)) + b"".join(struct.pack(">HHH", *e) for e in entries))


def jp2_file(cs, subboxes):
    """A JP2 file: signature, ftyp, a jp2h holding `subboxes` (bytes, in that order), jp2c."""
    sig = struct.pack(">I4sI", 12, b"jP  ", 0x0d0a870a)
    ftyp = box("ftyp", b"jp2 " + struct.pack(">I", 0) + b"jp2 ")
    return sig + ftyp + box("jp2h", b"".join(subboxes)) + box("jp2c", cs)


# ------------------------------------------------------------------------------ restatement
def _default_typ(c):
    """GrkImage::create's component type: colour for the first three, then unspecified."""
    return 0 if c < 3 else 65535


def apply_palette(planes, lut, cmap_entries):
    """apply_palette_clr: planes (list of 2-D int arrays, the codestream's components) -> the NPC
    channels and the component each was made from (the new component is a copy of it, type
    included).  Indices are clamped to [0, NE - 1] (:1417-1421); channel i of a direct mapping
    lands in slot i, a palette mapping in slot PCOL (:1359-1375)."""
    lut = np.asarray(lut, dtype=np.int64)
    out, src = [None] * lut.shape[1], [None] * lut.shape[1]
    for i, (c, mtyp, pcol) in enumerate(cmap_entries):
        if mtyp == 0:
            out[i], src[i] = np.array(planes[c], dtype=np.int32), c
        else:
            k = np.clip(np.asarray(planes[c], dtype=np.int64), 0, lut.shape[0] - 1)
            out[pcol], src[pcol] = lut[k, pcol].astype(np.int32), c
    return out, src


def apply_cdef(planes, entries, typ=None):
    """apply_channel_definition: Grok's swap sequence, later entries rewritten after each swap
    (:909-927).  Returns (planes, [typ per position])."""
    planes = list(planes)
    n = len(planes)
    typ = list(typ) if typ is not None else [_default_typ(k) for k in range(n)]
    info = [list(e) for e in entries]
    for i in range(len(info)):
        cn, t, asoc = info[i]
        if cn >= n:
            continue
        typ[cn] = t
        if t != 0 or asoc == 0:
            continue
        if asoc > n:
            continue
        a = asoc - 1
        if cn != a:
            planes[cn], planes[a] = planes[a], planes[cn]
            typ[cn], typ[a] = typ[a], typ[cn]
            for j in range(i + 1, len(info)):
                if info[j][0] == cn:
                    info[j][0] = a
                elif info[j][0] == a:
                    info[j][0] = cn
    return planes, typ


def expected(planes, lut=None, cmap_entries=None, cdef_entries=None):
    """What a decode returns for the codestream components `planes`: (C, H, W) int32, channel types."""
    out = list(planes)
    typ = [_default_typ(k) for k in range(len(out))]
    if lut is not None and cmap_entries is not None:
        out, src = apply_palette(out, lut, cmap_entries)
        typ = [_default_typ(c) for c in src]
    if cdef_entries is not None:
        out, typ = apply_cdef(out, cdef_entries, typ)
    return np.stack([np.asarray(p, dtype=np.int32) for p in out]), typ


# ------------------------------------------------------------------------------ cases
class Case:
    def __init__(self, name, src, prec, enc, lut=None, precs=None, cmap_entries=None, cdef_entries=None, enumcs=None,
                 icc=None):
        self.name, self.src, self.prec = name, src, prec
        self.lut, self.precs, self.cmap, self.cdef = lut, precs, cmap_entries, cdef_entries
        self.enumcs, self.icc = enumcs, icc
        c, h, w = src.shape
        self.cs = O.encode(src, prec, **enc)   # lossless: a decode of it is `src`
        sub = [ihdr(h, w, c, prec)]
        sub.append(colr_icc(icc) if icc is not None else colr_enum(enumcs))
        if lut is not None:
            sub.append(pclr(lut, precs))
            sub.append(cmap(cmap_entries))
        if cdef_entries is not None:
            sub.append(cdef(cdef_entries))
        self.file = jp2_file(self.cs, sub)
        self.want, self.typ = expected(list(src), lut, cmap_entries, cdef_entries)
        # per output channel precision: the palette's column precisions (apply_palette_clr sets
        # every channel's, :1387), else the components'; cdef moves them with the channels
        pr = list(precs) if lut is not None else [prec] * c
        if cdef_entries is not None:
            pr = [int(p[0, 0]) for p in apply_cdef([np.full((1, 1), v) for v in pr], cdef_entries)[0]]
        self.out_prec = pr
        self.colour_space = GRK_CLRSPC["icc" if icc is not None else enumcs]

    def expected_of(self, planes):
        """The restatement applied to other component planes (a reduced decode)."""
        return expected(list(planes), self.lut, self.cmap, self.cdef)[0]

    def __repr__(self):
        return self.name


def _indices(h, w, n, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, n, (h, w)).astype(np.int32)
    a.flat[:n] = np.arange(n)   # every value occurs
    return a


def _lut(ne, precs, seed):
    rng = np.random.RandomState(seed)
    return np.stack([rng.randint(0, 1 << p, ne) for p in precs], axis=1).astype(np.int64)


# NPC of case 4: gk_colour.hip stages tables of up to 64 KiB in LDS, an entry being the columns
# padded to an odd number of dwords.  1024 entries of 30 16-bit columns are 15 dwords each
# (60 KiB, staged); 31 columns are 16 -> 17 dwords (68 KiB): the first table gathered from
# global memory.
CASE4_NPC = 31


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case; the seven file cases of the JP2 colour feature (case 7 is two files)."""
    one = dict(mct=False, numres=3)
    out = []
    # 1: one tile, 8-bit indices over all 256 values, 200 entries: indices 200..255 are clamped
    out.append(Case("c1_clamp200", _indices(48, 64, 256, 1)[None], 8, one, _lut(200, [8, 8, 8], 11), [8, 8, 8],
                    [(0, 1, 0), (0, 1, 1), (0, 1, 2)], enumcs=16))
    # 2: odd width, 12-bit columns: two-byte entries, 16-bit output
    out.append(Case("c2_odd_12bit", _indices(33, 47, 256, 2)[None], 8, one, _lut(256, [12, 12, 12], 12), [12, 12, 12],
                    [(0, 1, 0), (0, 1, 1), (0, 1, 2)], enumcs=16))
    # 3: tiled, 10-bit indices, 1024 x 3 16-bit columns: 1024 entries of 3 dwords = 12 KiB, the
    # largest three-column table, staged in LDS
    out.append(Case("c3_tiles_1024", _indices(150, 230, 1024, 3)[None], 10, dict(mct=False, tiles=(64, 64), numres=3),
                    _lut(1024, [16, 16, 16], 13), [16, 16, 16], [(0, 1, 0), (0, 1, 1), (0, 1, 2)], enumcs=16))
    # 4: a table past the LDS limit (global gather)
    out.append(Case("c4_global", _indices(33, 47, 256, 4)[None], 8, one, _lut(1024, [16] * CASE4_NPC, 14), [16] * CASE4_NPC,
                    [(0, 1, k) for k in range(CASE4_NPC)], enumcs=0))
    # 5: component 0 through the palette into three channels, component 1 direct as the fourth;
    # the cdef reverses the colours and marks the fourth channel as opacity
    src5 = np.stack([_indices(33, 47, 256, 5), _indices(33, 47, 256, 6)])
    out.append(Case("c5_direct_cdef", src5, 8, one, _lut(256, [8, 8, 8, 8], 15), [8, 8, 8, 8],
                    [(0, 1, 0), (0, 1, 1), (0, 1, 2), (1, 0, 0)], [(0, 0, 3), (1, 0, 2), (2, 0, 1), (3, 1, 0)], enumcs=16))
    # 6: no palette: four components, colours 3, 2, 1 and a whole-image opacity
    src6 = np.stack([_indices(40, 52, 256, 20 + k) for k in range(4)])
    out.append(Case("c6_cdef_only", src6, 8, dict(mct=False, numres=3), cdef_entries=[(0, 0, 3), (1, 0, 2), (2, 0, 1), (3, 1, 0)],
                    enumcs=16))
    # 7: colour description only: sYCC, and a 200-byte ICC profile; samples unchanged
    src7 = np.stack([_indices(40, 52, 256, 30 + k) for k in range(3)])
    out.append(Case("c7_sycc", src7, 8, dict(mct=False, numres=3), enumcs=18))
    out.append(Case("c7_icc", src7, 8, dict(mct=False, numres=3), icc=bytes(np.random.RandomState(7).randint(0, 256, 200).astype(np.uint8))))
    return {c.name: c for c in out}


def malformed():
    """name -> (file bytes, box the message must name); every file is refused by the header probes."""
    h, w = 16, 16
    src = _indices(h, w, 256, 40)[None]
    cs = O.encode(src, 8, mct=False, numres=2)
    src3 = np.stack([_indices(h, w, 256, 41 + k) for k in range(3)])
    cs3 = O.encode(src3, 8, mct=False, numres=2)
    head, head3 = [ihdr(h, w, 1, 8), colr_enum(16)], [ihdr(h, w, 3, 8), colr_enum(16)]
    lut = _lut(256, [8, 8, 8], 42)
    p3 = pclr(lut, [8, 8, 8])
    m3 = [(0, 1, 0), (0, 1, 1), (0, 1, 2)]
    big = _lut(1025, [8, 8, 8], 43)
    f = {}
    f["ne_0"] = (jp2_file(cs, head + [pclr(lut, [8, 8, 8], ne=0), cmap(m3)]), "pclr")
    f["ne_1025"] = (jp2_file(cs, head + [pclr(big, [8, 8, 8]), cmap(m3)]), "pclr")
    f["signed_column"] = (jp2_file(cs, head + [pclr(lut, [8, 8, 8], signed=[False, True, False]), cmap(m3)]), "pclr")
    f["truncated_pclr"] = (jp2_file(cs, head + [pclr(lut, [8, 8, 8], truncate=5), cmap(m3)]), "pclr")
    f["cmap_before_pclr"] = (jp2_file(cs, head + [cmap(m3), p3]), "cmap")
    f["two_cmap"] = (jp2_file(cs, head + [p3, cmap(m3), cmap(m3)]), "cmap")
    f["mtyp_2"] = (jp2_file(cs, head + [p3, cmap([(0, 1, 0), (0, 2, 1), (0, 1, 2)])]), "cmap")
    f["column_twice"] = (jp2_file(cs, head + [p3, cmap([(0, 1, 0), (0, 1, 1), (0, 1, 1)])]), "cmap")
    f["cdef_cn_range"] = (jp2_file(cs3, head3 + [cdef([(0, 0, 1), (1, 0, 2), (3, 0, 3)])]), "cdef")
    f["cdef_incomplete"] = (jp2_file(cs3, head3 + [cdef([(0, 0, 1), (1, 0, 2)])]), "cdef")
    f["icc_len_0"] = (jp2_file(cs3, [ihdr(h, w, 3, 8), colr_icc(b"")]), "colr")
    f["prec_above_ne"] = (jp2_file(cs, head + [pclr(lut[:4], [8, 8, 8]), cmap(m3)]), "pclr")
    return f


def pclr_without_cmap():
    """(file, source): a palette with no component mapping is dropped (applyColour :383-388)."""
    src = _indices(16, 16, 256, 50)[None]
    cs = O.encode(src, 8, mct=False, numres=2)
    return jp2_file(cs, [ihdr(16, 16, 1, 8), colr_enum(17), pclr(_lut(256, [8, 8, 8], 51), [8, 8, 8])]), src


# ------------------------------------------------------------------------------ OpenJPEG (JP2)
class _Comp(ctypes.Structure):   # opj_image_comp_t (openjpeg.h, 2.5)
    _fields_ = [("dx", ctypes.c_uint32), ("dy", ctypes.c_uint32), ("w", ctypes.c_uint32), ("h", ctypes.c_uint32),
                ("x0", ctypes.c_uint32), ("y0", ctypes.c_uint32), ("prec", ctypes.c_uint32), ("bpp", ctypes.c_uint32),
                ("sgnd", ctypes.c_uint32), ("resno_decoded", ctypes.c_uint32), ("factor", ctypes.c_uint32),
                ("data", ctypes.POINTER(ctypes.c_int32)), ("alpha", ctypes.c_uint16)]


class _Image(ctypes.Structure):  # opj_image_t
    _fields_ = [("x0", ctypes.c_uint32), ("y0", ctypes.c_uint32), ("x1", ctypes.c_uint32), ("y1", ctypes.c_uint32),
                ("numcomps", ctypes.c_uint32), ("color_space", ctypes.c_int), ("comps", ctypes.POINTER(_Comp)),
                ("icc_profile_buf", ctypes.POINTER(ctypes.c_uint8)), ("icc_profile_len", ctypes.c_uint32)]


_opj = None


def _find():
    try:
        import PIL
    except ImportError:
        return None
    d = os.path.join(os.path.dirname(os.path.dirname(PIL.__file__)), "pillow.libs")
    hits = sorted(glob.glob(os.path.join(d, "libopenjp2*.so*")))
    return hits[0] if hits else None


def opj_available():
    return _find() is not None


def _lib():
    global _opj
    if _opj is None:
        L = ctypes.CDLL(_find())
        L.opj_create_decompress.restype = ctypes.c_void_p
        L.opj_create_decompress.argtypes = [ctypes.c_int]
        L.opj_set_default_decoder_parameters.argtypes = [ctypes.c_void_p]
        L.opj_setup_decoder.restype = ctypes.c_int
        L.opj_setup_decoder.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.opj_stream_create_default_file_stream.restype = ctypes.c_void_p
        L.opj_stream_create_default_file_stream.argtypes = [ctypes.c_char_p, ctypes.c_int]
        L.opj_read_header.restype = ctypes.c_int
        L.opj_read_header.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.POINTER(_Image))]
        L.opj_decode.restype = ctypes.c_int
        L.opj_decode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(_Image)]
        L.opj_end_decompress.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.opj_stream_destroy.argtypes = [ctypes.c_void_p]
        L.opj_destroy_codec.argtypes = [ctypes.c_void_p]
        L.opj_image_destroy.argtypes = [ctypes.POINTER(_Image)]
        _opj = L
    return _opj


def opj_decode_jp2(data):
    """Decode JP2 file bytes with OpenJPEG (OPJ_CODEC_JP2): dict(planes (C, H, W) int32, prec, alpha
    (per channel: the cdef Typ OpenJPEG records), color_space (OPJ_COLOR_SPACE), icc bytes)."""
    L = _lib()
    with tempfile.NamedTemporaryFile(suffix=".jp2", delete=False) as f:
        f.write(data)
        path = f.name
    codec = stream = None
    img = ctypes.POINTER(_Image)()
    try:
        codec = L.opj_create_decompress(2)   # OPJ_CODEC_JP2
        params = ctypes.create_string_buffer(1 << 16)   # opj_dparameters_t (a few KB)
        L.opj_set_default_decoder_parameters(params)
        if not L.opj_setup_decoder(codec, params):
            raise RuntimeError("opj_setup_decoder failed")
        stream = L.opj_stream_create_default_file_stream(path.encode(), 1)
        if not stream or not L.opj_read_header(stream, codec, ctypes.byref(img)):
            raise RuntimeError("opj_read_header failed")
        if not L.opj_decode(codec, stream, img):
            raise RuntimeError("opj_decode failed")
        L.opj_end_decompress(codec, stream)
        I = img.contents
        planes, prec, alpha = [], [], []
        for c in range(I.numcomps):
            cp = I.comps[c]
            planes.append(np.ctypeslib.as_array(cp.data, shape=(cp.h, cp.w)).copy())
            prec.append(cp.prec)
            alpha.append(cp.alpha)
        icc = bytes(I.icc_profile_buf[:I.icc_profile_len]) if I.icc_profile_len else b""
        return dict(planes=np.stack(planes), prec=prec, alpha=alpha, color_space=I.color_space, icc=icc)
    finally:
        if img:
            L.opj_image_destroy(img)
        if stream:
            L.opj_stream_destroy(stream)
        if codec:
            L.opj_destroy_codec(codec)
        os.unlink(path)
