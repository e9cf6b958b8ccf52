"""OpenJPEG 2.5.4 (the libopenjp2 Pillow ships) driven through its C API with ctypes: an
independent decoder that returns every component at its own size, and an independent encoder
(encode(), which tests/golden/make_opj_fixtures.py records streams from).

Pillow's own JPEG 2000 plugin refuses subsampled components except as sYCC, which it converts to
RGB; the library itself decodes them plane by plane (opj_image_comp_t w / h / dx / dy), which is
what the subsampling tests compare against.  Test infrastructure only."""
import ctypes
import glob
import os
import tempfile

import numpy as np

_lib = None


def _find():
    try:
        import PIL
    except ImportError:
        return None
    d = os.path.join(os.path.dirname(os.path.dirname(PIL.__file__)), "pillow.libs")
    hits = sorted(glob.glob(os.path.join(d, "libopenjp2*.so*")))
    return hits[0] if hits else None


class _Comp(ctypes.Structure):   # opj_image_comp_t (openjpeg.h, 2.5)
    _fields_ = [("dx", ctypes.c_uint32), ("dy", ctypes.c_uint32), ("w", ctypes.c_uint32), ("h", ctypes.c_uint32),
                ("x0", ctypes.c_uint32), ("y0", ctypes.c_uint32), ("prec", ctypes.c_uint32), ("bpp", ctypes.c_uint32),
                ("sgnd", ctypes.c_uint32), ("resno_decoded", ctypes.c_uint32), ("factor", ctypes.c_uint32),
                ("data", ctypes.POINTER(ctypes.c_int32)), ("alpha", ctypes.c_uint16)]


class _Image(ctypes.Structure):  # opj_image_t
    _fields_ = [("x0", ctypes.c_uint32), ("y0", ctypes.c_uint32), ("x1", ctypes.c_uint32), ("y1", ctypes.c_uint32),
                ("numcomps", ctypes.c_uint32), ("color_space", ctypes.c_int), ("comps", ctypes.POINTER(_Comp)),
                ("icc_profile_buf", ctypes.c_void_p), ("icc_profile_len", ctypes.c_uint32)]


def available():
    return _find() is not None


def lib():
    global _lib
    if _lib is None:
        path = _find()
        if path is None:
            raise RuntimeError("libopenjp2 not found")
        L = ctypes.CDLL(path)
        L.opj_version.restype = ctypes.c_char_p
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
        _lib = L
    return _lib


def version():
    return lib().opj_version().decode()


def decode(cs, reduce=0, layers=0):
    """Decode a raw codestream (J2K) -> [(dx, dy, plane int32 (h, w))] per component.  reduce
    discards that many resolutions, layers > 0 keeps only the first layers (opj_decompress -r / -l:
    cp_reduce and cp_layer, the first two uint32 of opj_dparameters_t; the reduced planes'
    ceil(x / 2^reduce) sizes show the layout holds, tests/test_opj_streams.py)."""
    L = lib()
    with tempfile.NamedTemporaryFile(suffix=".j2k", delete=False) as f:
        f.write(cs)
        path = f.name
    codec = stream = None
    img = ctypes.POINTER(_Image)()
    try:
        codec = L.opj_create_decompress(0)   # OPJ_CODEC_J2K
        params = ctypes.create_string_buffer(1 << 16)   # opj_dparameters_t (a few KB)
        L.opj_set_default_decoder_parameters(params)
        head = ctypes.cast(params, ctypes.POINTER(ctypes.c_uint32))
        head[0], head[1] = int(reduce), int(layers)
        if not L.opj_setup_decoder(codec, params):
            raise RuntimeError("opj_setup_decoder failed")
        stream = L.opj_stream_create_default_file_stream(path.encode(), 1)
        if not stream or not L.opj_read_header(stream, codec, ctypes.byref(img)):
            raise RuntimeError("opj_read_header failed")
        if not L.opj_decode(codec, stream, img):
            raise RuntimeError("opj_decode failed")
        L.opj_end_decompress(codec, stream)
        out = []
        for c in range(img.contents.numcomps):
            cp = img.contents.comps[c]
            a = np.ctypeslib.as_array(cp.data, shape=(cp.h, cp.w)).copy()
            out.append((cp.dx, cp.dy, a))
        return out
    finally:
        if img:
            L.opj_image_destroy(img)
        if stream:
            L.opj_stream_destroy(stream)
        if codec:
            L.opj_destroy_codec(codec)
        os.unlink(path)


# ------------------------------------------------------------------------------------ encoder
# No OpenJPEG header is installed; opj_cparameters_t (openjpeg.h, 2.5) is addressed as an array of
# int32 around one anchor: the defaults numresolution, cblockw_init, cblockh_init, mode,
# irreversible, roi_compno, roi_shift, res_spec = 6, 64, 64, 0, 0, -1, 0, 0, a run that occurs once
# in what opj_set_default_encoder_parameters fills.  Every field set here is read back from the
# written stream's markers by tests/test_opj_streams.py (the header probes), which is what pins
# the offsets.
_ANCHOR = [6, 64, 64, 0, 0, -1, 0, 0]
_PARAM_BYTES = 1 << 16
# ints from the front (LP64): tile_size_on, cp_tx0, cp_ty0, cp_tdx, cp_tdy, cp_disto_alloc,
# cp_fixed_alloc, cp_fixed_quality, cp_matrice (pointer), cp_comment (pointer), csty, prog_order
_TILE_ON, _TX0, _TY0, _TDX, _TDY, _DISTO, _QUALITY, _COMMENT, _CSTY, _PROG = 0, 1, 2, 3, 4, 5, 7, 10, 12, 13
# ints from the anchor: tcp_numlayers, tcp_rates[100], tcp_distoratio[100] in front of it; behind
# it prcw_init[33], prch_init[33], infile / outfile / index (char[4096] each, index_on between),
# image_offset_x0 / y0, subsampling_dx / dy, decod_format, cod_format, the JPWL block (118 ints),
# cp_cinema, max_comp_size, cp_rsiz, the chars tp_on / tp_flag / tcp_mct, jpip_on, mct_data
# (pointer), max_cs_size, rsiz (uint16)
_NLAYERS, _RATES, _DISTO_RATIO = -201, -200, -100
_PRCW, _PRCH = 8, 41
_OFFX, _OFFY, _SUBDX = 3147, 3148, 3149
_MAX_COMP, _TP_CHARS, _JPIP = 3272, 3274, 3275
CSTY_PRT, CSTY_SOP, CSTY_EPH = 1, 2, 4
MODE_BYPASS, MODE_RESET, MODE_TERMALL, MODE_VSC, MODE_PTERM, MODE_SEGSYM = 1, 2, 4, 8, 16, 32
PROGS = ["LRCP", "RLCP", "RPCL", "PCRL", "CPRL"]
CINEMA = {"cinema2k": 3, "cinema4k": 4}   # OPJ_PROFILE_CINEMA_2K / 4K (rsiz)
_CINEMA_24_CS, _CINEMA_24_COMP = 1302083, 1041666   # OPJ_CINEMA_24_CS / _COMP


_MSG_CB = ctypes.CFUNCTYPE(None, ctypes.c_char_p, ctypes.c_void_p)   # opj_msg_callback


class _CmptParm(ctypes.Structure):   # opj_image_cmptparm_t
    _fields_ = [(n, ctypes.c_uint32) for n in ("dx", "dy", "w", "h", "x0", "y0", "prec", "bpp", "sgnd")]


def _enc_lib():
    L = lib()
    if not getattr(L, "_enc_ready", False):
        L.opj_set_default_encoder_parameters.argtypes = [ctypes.c_void_p]
        L.opj_create_compress.restype = ctypes.c_void_p
        L.opj_create_compress.argtypes = [ctypes.c_int]
        L.opj_image_create.restype = ctypes.POINTER(_Image)
        L.opj_image_create.argtypes = [ctypes.c_uint32, ctypes.POINTER(_CmptParm), ctypes.c_int]
        L.opj_setup_encoder.restype = ctypes.c_int
        L.opj_setup_encoder.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(_Image)]
        L.opj_encoder_set_extra_options.restype = ctypes.c_int
        L.opj_encoder_set_extra_options.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p)]
        for f in ("opj_start_compress", "opj_encode", "opj_end_compress"):
            getattr(L, f).restype = ctypes.c_int
        L.opj_start_compress.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Image), ctypes.c_void_p]
        L.opj_encode.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.opj_end_compress.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.opj_set_error_handler.argtypes = [ctypes.c_void_p, _MSG_CB, ctypes.c_void_p]
        L._enc_ready = True
    return L


def encoder_params():
    """(buffer, int32 view, anchor index) of default opj_cparameters_t, or None when the anchor run
    is not found exactly once (another OpenJPEG layout: callers skip)."""
    L = _enc_lib()
    buf = ctypes.create_string_buffer(_PARAM_BYTES)
    L.opj_set_default_encoder_parameters(buf)
    a = np.frombuffer(buf, np.int32)
    hits = [i for i in range(len(a) - len(_ANCHOR)) if a[i:i + len(_ANCHOR)].tolist() == _ANCHOR]
    if len(hits) != 1 or a[hits[0] + _SUBDX:hits[0] + _SUBDX + 4].tolist() != [1, 1, -1, -1]:
        return None
    return buf, a, hits[0]


def encode(planes, prec, signed=False, subsampling=None, size=None, origin=(0, 0), numres=6, cblk=(64, 64), mode=0,
           irreversible=False, roi=None, sop=False, eph=False, prog="LRCP", rates=None, dB=None, tiles=None,
           tile_origin=(0, 0), precincts=None, mct=False, plt=False, tlm=False, comment=None, cinema=None):
    """OpenJPEG's encoder (opj_compress's call sequence) -> raw codestream bytes.

    planes: (C, H, W) array, or with subsampling=[(dx, dy), ...] one 2-D plane per component on its
    own grid and size=(W, H).  rates: compression ratios per layer (cp_disto_alloc, 0 or 1 =
    lossless); dB: PSNR per layer (cp_fixed_quality, 0 = lossless); neither: one lossless layer.
    roi=(component, shift); tiles=(w, h); precincts=[(w, h), ...] from the highest resolution down;
    cinema="cinema2k" / "cinema4k" (the 24 fps budgets; the library then forces the profile's
    coding itself)."""
    L = _enc_lib()
    got = encoder_params()
    if got is None:
        raise RuntimeError("opj_cparameters_t layout not recognised")
    buf, a, R = got
    f32 = np.frombuffer(buf, np.float32)
    u8 = np.frombuffer(buf, np.uint8)
    comps = [np.ascontiguousarray(p, np.int32) for p in planes]
    if subsampling:
        W, H = size
    else:
        H, W = comps[0].shape
        subsampling = [(1, 1)] * len(comps)
    x0, y0 = origin
    a[R], a[R + 1], a[R + 2], a[R + 3], a[R + 4] = numres, cblk[0], cblk[1], mode, int(irreversible)
    if roi:
        a[R + 5], a[R + 6] = roi
    a[_CSTY] = (CSTY_SOP if sop else 0) | (CSTY_EPH if eph else 0)
    a[_PROG] = PROGS.index(prog)
    layers = rates or dB or [0]
    a[R + _NLAYERS] = len(layers)
    a[_QUALITY if dB else _DISTO] = 1
    f32[R + (_DISTO_RATIO if dB else _RATES):][:len(layers)] = layers
    if tiles:
        a[_TILE_ON], a[_TDX], a[_TDY] = 1, tiles[0], tiles[1]
        a[_TX0], a[_TY0] = tile_origin
    if precincts:
        a[_CSTY] |= CSTY_PRT
        a[R + 7] = len(precincts)
        for i, (pw, ph) in enumerate(precincts):
            a[R + _PRCW + i], a[R + _PRCH + i] = pw, ph
    a[R + _OFFX], a[R + _OFFY] = x0, y0
    u8[(R + _TP_CHARS) * 4 + 2] = int(mct)
    keep = None
    if comment is not None:
        keep = ctypes.create_string_buffer(comment.encode())
        ctypes.cast(ctypes.byref(buf, _COMMENT * 4), ctypes.POINTER(ctypes.c_void_p))[0] = ctypes.addressof(keep)
    if cinema:
        a[R + _MAX_COMP] = _CINEMA_24_COMP
        o = -(-(R + _JPIP + 1) * 4 // 8) * 8 + 8   # past mct_data (pointer-aligned)
        a[o // 4] = _CINEMA_24_CS
        np.frombuffer(buf, np.uint16)[o // 2 + 2] = CINEMA[cinema]
    cd = lambda v, d: -(-v // d)
    parms = (_CmptParm * len(comps))()
    for c, (p, (dx, dy)) in enumerate(zip(comps, subsampling)):
        assert p.shape == (cd(y0 + H, dy) - cd(y0, dy), cd(x0 + W, dx) - cd(x0, dx)), (c, p.shape)
        parms[c].dx, parms[c].dy, parms[c].w, parms[c].h = dx, dy, p.shape[1], p.shape[0]
        parms[c].x0, parms[c].y0, parms[c].prec, parms[c].bpp, parms[c].sgnd = x0, y0, prec, prec, int(signed)
    img = L.opj_image_create(len(comps), parms, 1 if len(comps) >= 3 else 2)   # OPJ_CLRSPC_SRGB / GRAY
    if not img:
        raise RuntimeError("opj_image_create failed")
    codec = stream = None
    fd, path = tempfile.mkstemp(suffix=".j2k")
    os.close(fd)
    try:
        img.contents.x0, img.contents.y0, img.contents.x1, img.contents.y1 = x0, y0, x0 + W, y0 + H
        for c, p in enumerate(comps):
            ctypes.memmove(img.contents.comps[c].data, p.ctypes.data, p.nbytes)
        codec = L.opj_create_compress(0)   # OPJ_CODEC_J2K
        errors = []
        on_error = _MSG_CB(lambda msg, _: errors.append(msg.decode(errors="replace").strip()))
        L.opj_set_error_handler(codec, on_error, None)
        if not L.opj_setup_encoder(codec, buf, img):
            raise RuntimeError("opj_setup_encoder failed: " + "; ".join(errors))
        opts = [o for o, on in ((b"PLT=YES", plt), (b"TLM=YES", tlm)) if on]
        if opts and not L.opj_encoder_set_extra_options(codec, (ctypes.c_char_p * (len(opts) + 1))(*opts, None)):
            raise RuntimeError("opj_encoder_set_extra_options failed")
        stream = L.opj_stream_create_default_file_stream(path.encode(), 0)
        if not stream:
            raise RuntimeError("opj_stream_create_default_file_stream failed")
        if not (L.opj_start_compress(codec, img, stream) and L.opj_encode(codec, stream)
                and L.opj_end_compress(codec, stream)):
            raise RuntimeError("OpenJPEG encode failed: " + "; ".join(errors))
        L.opj_stream_destroy(stream)   # (flushes the file)
        stream = None
        with open(path, "rb") as f:
            return f.read()
    finally:
        if stream:
            L.opj_stream_destroy(stream)
        if codec:
            L.opj_destroy_codec(codec)
        L.opj_image_destroy(img)
        os.unlink(path)
