"""lcms2 (the colour-management library Grok links) through ctypes: Pillow's wheel carries it in
pillow.libs, as it carries libopenjp2 (tests/openjpeg.py).  Only the calls Grok's CLI makes
(bin/common/color.cpp: color_apply_icc_profile, color_cielab_to_rgb).  Test infrastructure only."""
import ctypes
import glob
import os

import numpy as np

# pixel formats (lcms2.h: COLORSPACE_SH(pt) << 16 | CHANNELS_SH(n) << 3 | BYTES_SH(b); FLOAT_SH 1 << 22)
TYPE_GRAY_8 = (3 << 16) | (1 << 3) | 1
TYPE_RGB_8 = (4 << 16) | (3 << 3) | 1
TYPE_RGB_16 = (4 << 16) | (3 << 3) | 2
TYPE_Lab_DBL = (1 << 22) | (10 << 16) | (3 << 3) | 0
INTENT_PERCEPTUAL = 0
FLAGS_NOOPTIMIZE = 0x0100

_lib = None


def _find():
    try:
        import PIL
    except ImportError:
        return None
    d = os.path.join(os.path.dirname(os.path.dirname(PIL.__file__)), "pillow.libs")
    hits = sorted(glob.glob(os.path.join(d, "liblcms2*.so*")))
    return hits[0] if hits else None


def available():
    return _find() is not None


class _xyY(ctypes.Structure):
    _fields_ = [("x", ctypes.c_double), ("y", ctypes.c_double), ("Y", ctypes.c_double)]


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(_find())
        L.cmsOpenProfileFromMem.restype = ctypes.c_void_p
        L.cmsOpenProfileFromMem.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
        L.cmsCreate_sRGBProfile.restype = ctypes.c_void_p
        L.cmsCreateLab4Profile.restype = ctypes.c_void_p
        L.cmsCreateLab4Profile.argtypes = [ctypes.c_void_p]
        L.cmsWhitePointFromTemp.restype = ctypes.c_int
        L.cmsWhitePointFromTemp.argtypes = [ctypes.POINTER(_xyY), ctypes.c_double]
        L.cmsGetHeaderRenderingIntent.restype = ctypes.c_uint32
        L.cmsGetHeaderRenderingIntent.argtypes = [ctypes.c_void_p]
        L.cmsCreateTransform.restype = ctypes.c_void_p
        L.cmsCreateTransform.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                         ctypes.c_uint32]
        L.cmsDoTransform.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
        L.cmsCloseProfile.argtypes = [ctypes.c_void_p]
        L.cmsDeleteTransform.argtypes = [ctypes.c_void_p]
        _lib = L
    return _lib


def _run(in_prof, in_type, out_type, intent, flags, src, out):
    L = lib()
    out_prof = L.cmsCreate_sRGBProfile()
    t = L.cmsCreateTransform(in_prof, in_type, out_prof, out_type, intent, flags)
    L.cmsCloseProfile(in_prof)
    L.cmsCloseProfile(out_prof)
    if not t:
        raise RuntimeError("cmsCreateTransform failed")
    src = np.ascontiguousarray(src)
    L.cmsDoTransform(t, src.ctypes.data, out.ctypes.data, src.shape[0])
    L.cmsDeleteTransform(t)
    return out


def apply_profile(profile, samples, bits=8, flags=0):
    """color_apply_icc_profile's transform: samples (N, 3) for an RGB profile, (N,) for a grey one
    (8-bit only, TYPE_GRAY_8 -> TYPE_RGB_8 as Grok calls it) -> (N, 3) sRGB at `bits` (8 or 16)."""
    L = lib()
    prof = L.cmsOpenProfileFromMem(bytes(profile), len(profile))
    if not prof:
        raise RuntimeError("cmsOpenProfileFromMem failed")
    intent = L.cmsGetHeaderRenderingIntent(prof)
    samples = np.asarray(samples)
    if samples.ndim == 1:
        assert bits == 8
        return _run(prof, TYPE_GRAY_8, TYPE_RGB_8, intent, flags, samples.astype(np.uint8),
                    np.empty((samples.shape[0], 3), np.uint8))
    dt, ty = (np.uint8, TYPE_RGB_8) if bits == 8 else (np.uint16, TYPE_RGB_16)
    return _run(prof, ty, ty, intent, flags, samples.astype(dt), np.empty(samples.shape, dt))


def lab_to_rgb16(lab, temp=None):
    """color_cielab_to_rgb's transform: (N, 3) float64 L*a*b* -> (N, 3) uint16 sRGB (TYPE_Lab_DBL ->
    TYPE_RGB_16, perceptual, flags 0).  temp: the white point cmsWhitePointFromTemp gives for that
    temperature (None: D50, a null white point)."""
    L = lib()
    if temp is None:
        prof = L.cmsCreateLab4Profile(None)
    else:
        wp = _xyY()
        L.cmsWhitePointFromTemp(ctypes.byref(wp), float(temp))
        prof = L.cmsCreateLab4Profile(ctypes.byref(wp))
    lab = np.ascontiguousarray(lab, np.float64)
    return _run(prof, TYPE_Lab_DBL, TYPE_RGB_16, INTENT_PERCEPTUAL, 0, lab, np.empty(lab.shape, np.uint16))
