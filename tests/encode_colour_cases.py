"""Colour descriptions on encode: the case list shared by the CPU tests (gk_jp2_boxes against the
hand-built boxes of tests/jp2_boxes.py, the header probes and OpenJPEG) and the GPU tests (the
engine's JP2 encodes).  Each case holds the codestream components, the arguments of
Engine.set_encode_colour / grok_amd.jp2_boxes, and the jp2h sub-boxes Grok's write_jp2h would
write for them, in its order: ihdr, colr, [cdef], [pclr, cmap].  Test infrastructure only."""
import functools
import struct

import numpy as np

import jp2_boxes as J

RGBA = [(0, 1), (0, 2), (0, 3), (1, 0)]            # (typ, asoc) per component: opacity on channel 3
SPACE = {"srgb": (2, 16), "grey": (3, 17), "sycc": (4, 18), "esycc": (5, 24), "cmyk": (6, 12), "icc": (9, 0)}   # GRK_COLOR_SPACE, EnumCS
COLOUR_CHANNELS = {"srgb": 3, "grey": 1, "sycc": 3, "esycc": 3, "cmyk": 4, "icc": 0}


class Case:
    def __init__(self, name, src, prec, space, icc=None, channels=None, palette=None):
        self.name, self.src, self.prec, self.space = name, src, prec, space
        self.icc, self.channels, self.palette = icc, channels, palette
        self.kw = dict(space=space)
        if icc is not None:
            self.kw["icc"] = icc
        if channels is not None:
            self.kw["channels"] = channels
        if palette is not None:
            self.kw["palette"] = palette
        nc = src.shape[0]
        # initCompress :840-865: the first color_channels entries forced, the rest from the image
        self.cdef = None
        if channels is not None and any(t != 0 for t, _ in channels):
            k = COLOUR_CHANNELS[space]
            self.cdef = [(i, 0, i + 1) if i < k else (i, channels[i][0], channels[i][1]) for i in range(nc)]
        self.lut, self.precs, self.cmap = palette if palette is not None else (None, None, None)

    def subboxes(self, shape=None):
        c, h, w = shape or self.src.shape
        sub = [J.ihdr(h, w, c, self.prec), J.colr_icc(self.icc) if self.space == "icc" else J.colr_enum(SPACE[self.space][1])]
        if self.cdef is not None:
            sub.append(J.cdef(self.cdef))
        if self.palette is not None:
            sub += [J.pclr(self.lut, self.precs), J.cmap(self.cmap)]
        return sub

    def file(self, cs):
        return J.jp2_file(cs, self.subboxes())

    def prefix(self):
        """The bytes in front of the codestream (any length below 4 GiB - 8: the jp2c LBox aside)."""
        return J.jp2_file(b"", self.subboxes())[:-8]

    def expected(self):
        """(planes, typ) a decode of the file returns (the restatement of tests/jp2_boxes.py)."""
        return J.expected(list(self.src), self.lut, self.cmap, self.cdef)

    def __repr__(self):
        return self.name


def _planes(n, h, w, prec, seed):
    return np.stack([J._indices(h, w, 1 << prec, seed + k) for k in range(n)])


ICC = bytes(np.random.RandomState(9).randint(0, 256, 200).astype(np.uint8))
H, W = 40, 52


@functools.lru_cache(maxsize=None)
def cases():
    out = [
        Case("grey_opacity", _planes(2, H, W, 8, 100), 8, "grey", channels=[(0, 1), (1, 0)]),
        Case("rgba", _planes(4, H, W, 8, 110), 8, "srgb", channels=RGBA),
        Case("rgb_premultiplied", _planes(4, H, W, 8, 120), 8, "srgb", channels=[(0, 1), (0, 2), (0, 3), (2, 0)]),
        Case("sycc", _planes(3, H, W, 8, 130), 8, "sycc"),
        Case("esycc", _planes(3, H, W, 8, 140), 8, "esycc"),
        Case("cmyk", _planes(4, H, W, 8, 150), 8, "cmyk"),
        Case("icc", _planes(3, H, W, 8, 160), 8, "icc", icc=ICC),
        Case("icc_opacity", _planes(4, H, W, 8, 170), 8, "icc", icc=ICC, channels=RGBA),
        Case("palette8_200", _planes(1, H, W, 8, 180), 8, "srgb",
             palette=(J._lut(200, [8, 8, 8], 21), [8, 8, 8], [(0, 1, 0), (0, 1, 1), (0, 1, 2)])),
        Case("palette10_1024", _planes(1, H, W, 10, 190), 10, "srgb",
             palette=(J._lut(1024, [16, 16, 16], 22), [16, 16, 16], [(0, 1, 0), (0, 1, 1), (0, 1, 2)])),
        Case("palette_and_direct", _planes(2, H, W, 8, 200), 8, "srgb",
             palette=(J._lut(256, [8, 8, 8, 8], 23), [8, 8, 8, 8], [(0, 1, 0), (0, 1, 1), (0, 1, 2), (1, 0, 0)])),
    ]
    return {c.name: c for c in out}


# the > 2^30-byte geometry: the jp2c box takes an 8-byte XLBox (boxes only; no such image is coded)
XL_SHAPE, XL_CS_LEN = (4, 20000, 20000), (5 << 30) + 12345


def xl_prefix():
    c = Case("xl", np.zeros((4, 1, 1), np.int32), 8, "srgb", channels=RGBA)
    head = J.jp2_file(b"", c.subboxes(XL_SHAPE))[:-8]
    return c, head + struct.pack(">I4sQ", 1, b"jp2c", XL_CS_LEN + 16)


def refusals():
    """name -> (shape, prec, signed, colour arguments, the box or field the message must name)."""
    pal3 = [(0, 1, 0), (0, 1, 1), (0, 1, 2)]
    lut = J._lut(256, [8, 8, 8], 31)
    one, three = (1, 16, 16), (3, 16, 16)
    bad = lut.copy()
    bad[7, 1] = 256

    def pal(lut=lut, precs=(8, 8, 8), cm=pal3):
        return dict(space="srgb", palette=(lut, list(precs), list(cm)))

    r = {
        "space_unknown": (three, 8, False, dict(space=0), "colour_space"),
        "space_custom_cie": (three, 8, False, dict(space=8), "colour_space"),
        "space_out_of_enum": (three, 8, False, dict(space=77), "colour_space"),
        "space_default_cie": (three, 8, False, dict(space="cie"), "CIE"),
        "icc_without_profile": (three, 8, False, dict(space="icc"), "icc"),
        "icc_empty_profile": (three, 8, False, dict(space="icc", icc=b""), "icc"),
        "profile_with_srgb": (three, 8, False, dict(space="srgb", icc=ICC), "icc"),
        "colour_channels_above_comps": (three, 8, False, dict(space="cmyk", channels=[(0, 1), (0, 2), (1, 0)]), "cdef"),
        "typ_count": (three, 8, False, dict(space="srgb", channels=RGBA), "typ"),
        "ne_0": (one, 8, False, pal(lut=lut[:0]), "pclr"),
        "ne_1025": (one, 8, False, pal(lut=J._lut(1025, [8, 8, 8], 32)), "pclr"),
        "npc_0": (one, 8, False, pal(lut=np.zeros((4, 0), np.int64), precs=(), cm=()), "pclr"),
        "column_17_bits": (one, 8, False, pal(lut=J._lut(256, [8, 17, 8], 33), precs=(8, 17, 8)), "pclr"),
        "lut_value_out_of_range": (one, 8, False, pal(lut=bad), "pclr"),
        "lut_value_negative": (one, 8, False, pal(lut=-bad), "pclr"),
        "mtyp_2": (one, 8, False, pal(cm=[(0, 1, 0), (0, 2, 1), (0, 1, 2)]), "cmap"),
        "column_twice": (one, 8, False, pal(cm=[(0, 1, 0), (0, 1, 1), (0, 1, 1)]), "cmap"),
        "column_out_of_range": (one, 8, False, pal(cm=[(0, 1, 0), (0, 1, 1), (0, 1, 5)]), "cmap"),
        "direct_with_column": (one, 8, False, pal(cm=[(0, 1, 0), (0, 1, 1), (0, 0, 2)]), "cmap"),
        "component_out_of_range": (one, 8, False, pal(cm=[(0, 1, 0), (0, 1, 1), (1, 1, 2)]), "cmap"),
        "signed_mapped_component": (one, 8, True, pal(), "cmap"),
        "component_bits_above_entries": (one, 8, False, pal(lut=lut[:4]), "pclr"),
        "cdef_incomplete": (one, 8, False, dict(space="grey", channels=[(1, 0)], palette=(lut, [8, 8, 8], pal3)), "cdef"),
        "cdef_contradictory": ((5, 16, 16), 8, False, dict(space="srgb", channels=RGBA + [(1, 0)]), "cdef"),
        "cdef_illegal_type": ((4, 16, 16), 8, False, dict(space="srgb", channels=[(0, 1), (0, 2), (0, 3), (7, 0)]), "cdef"),
    }
    return r
