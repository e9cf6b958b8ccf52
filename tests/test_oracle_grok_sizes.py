"""Known answers from Grok 9.2.0 itself for rate control on tiles, progression order changes
and odd-parity tiles.

The round-3 and round-4 reviews ran Grok's own grk_compress on
grok_amd.synth.synth_image(384, 520, 3, 8, 7) ("A") and synth_image(300, 260, 1, 16, 21)
("B") with the CLI flags below and recorded the codestream size and SHA-256 (first 16 hex
digits); these tests hold the oracle to them byte for byte.  They pin:

  * CodeStreamCompress::updateRates (:951-1027): per-tile budgets from the tile's pixel count,
    the header bytes (TLM and POC markers included) shared by area, the (parts - 1) x 14 bytes
    of tile-part generation;
  * T2Compress::compressPacketsSimulate (:59-112, :347-434) in Grok's own arithmetic: a packet
    met with no byte left passes and the uint32 budget wraps; a budget reached inside a
    number-of-passes or comma code is not seen (BitIO::putnumpasses / putcommacode return
    nothing, BitIO.cpp:144-178), so that header's count runs past the budget, the subtraction
    wraps and the rest of the layer "fits" (oracle GrkSimBitIO);
  * the final simulation's packet lengths as the PLT marker and, for a tile in one part with
    one progression, the precalculated tile-part length in SOT / TLM (TileProcessor.cpp:243-259):
    after such a swallowed failure they are not the bytes written;
  * progression order changes (-P): POC in the main header and in each tile's first part, one
    tile part per entry, the rate-control simulation in the tile's own progression.

These numbers were typed in from the reviews' own Grok builds, on full-size images.  Grok can be
rebuilt beside this repository (`make -C oracle ref`): tests/test_grok_live.py
and tests/test_grok_fixtures.py hold the same option families to its binaries and to recordings
of their output on small images; the numbers here stay as the full-size pin.
"""
import hashlib

import numpy as np
import pytest

import oracle as O
from conftest import parse_flags
from grok_amd.synth import synth_image

# (input, Grok CLI flags, Grok bytes, Grok SHA-256 prefix or None where only the size was recorded)
KNOWN = [
    ("A", "-t 256,256 -r 20,5 -X", 118560, None),
    ("A", "-t 128,128 -r 30", 22142, None),
    ("A", "-r 20,10 -P T0=0,0,2,3,3,RLCP/T0=3,0,2,6,3,LRCP", 59621, "0be62df5a6eaa292"),
    ("A", "-P T0=0,0,2,3,3,RLCP/T0=3,0,2,6,3,LRCP", 410830, None),
    ("A", "-t 64,64 -r 40,10", 58693, "74e205793d99ec86"),
    ("A", "-t 64,64 -r 40,10 -X", 59057, "3aed03d6d38355b3"),
    ("A", "-t 64,64 -r 40,10 -X -L", 61386, "e0f30b121f864170"),
    ("A", "-t 128,128 -r 20,5 -M 1", 116460, "5e610ced8e4b3ec4"),
    ("A", "-M 3 -t 128,128 -r 20,5", 116863, "761c07175aa1d9ef"),
    ("A", "-p PCRL -c [128,128] -r 30,10 -t 256,256", 59432, "9ea438908929a4fe"),
    ("A", "-S -E -p RPCL -c [64,64],[32,32] -r 20,5 -t 256,256 -X -L", 126044, "cf3dffa94f7c4d5d"),
    ("A", "-t 256,256 -r 20,5 -u L", 118792, "8eb104ee7af67c2f"),
    ("A", "-t 200,160 -r 30,10", 59002, "233358c512356ea7"),
    ("A", "-p CPRL -c [64,64],[32,32] -r 20,5,1", 430903, "4b2a4e73b5768a8a"),
    ("B", "-t 96,96 -r 30,5", 31004, "a484a6cb530b7307"),
    # precinct sizes halved down to 1 at resolution 0: Grok writes exponent 0 there (1 x 1
    # code-blocks; CodeStreamCompress.cpp:573-590 clamps only a size below 1 to exponent 1)
    ("A", "-c [32,32]", 460644, "1a20eebb14e5bdae"),
    ("A", "-c [128,128] -n 8", 414895, "a579b4e7db961bcc"),
    ("A", "-c [32,32] -t 128,128 -r 25,8", 81116, "d1d86b10027d07d8"),
]
# code-blocks with a side above 64 (grk_compress.cpp:981-988 accepts 4 <= w, h <= 1024 with
# w * h <= 4096; T1.cpp:337-398 sizes the flags from the block)
KNOWN_WIDE = [
    ("A", "-b 128,32", 410963, "69f2f8af6486a243"),
    ("A", "-b 1024,4 -r 20,5", 119723, "e7f7599fcd9dc5ef"),
    ("A", "-b 256,16 -t 256,256 -r 30,10 -X -L", 60250, "3181016eaffb0732"),
    ("B", "-b 512,8", 134945, "f208992db5ed0200"),
]
# Grok 9.2.0's grk_decompress on Grok's own streams (round-5 review): (input, encode flags,
# reduce -r, window -d at full resolution or None, output shape, SHA-256 prefix of the decoded
# C x H x W array as little-endian uint16).  A window is returned on the reduced canvas with every
# edge ceil(x / 2^r) (CodeStreamDecompress.cpp:390, 471-481) and decoded under the partial-tile
# rule a window selects (WaveletReverse.cpp:1551-1554).
DECODES = [
    ("A", "-t 128,128", 2, (37, 51, 300, 333), (3, 71, 65), "8e8e070182473ca1"),
    ("A", "", 1, (10, 20, 200, 170), (3, 75, 95), "2116a8a1fc0a78b3"),
    ("A", "-I -t 128,128", 2, (37, 51, 300, 333), (3, 71, 65), "d14027a6df793e4f"),
    ("D", "-p RPCL -c [128,128],[64,64] -t 256,256", 1, (100, 200, 650, 611), (3, 206, 275), "292c11071aec9bbf"),
    ("A", "-I -t 128,128 -r 40,20,10", 0, (37, 51, 300, 333), (3, 282, 263), "867ec517e1d2a93d"),
    ("B", "-M 64", 2, None, (1, 75, 65), "6351293e6e33fed7"),
]
IMAGES = {"A": ((384, 520, 3, 8, 7), 8), "B": ((300, 260, 1, 16, 21), 16), "D": ((700, 900, 3, 8, 55), 8)}


def u16_sha(a):
    return hashlib.sha256(np.ascontiguousarray(a.astype("<u2")).tobytes()).hexdigest()[:16]


def oracle_reduced(cs, red, win):
    """The oracle's decode of cs at reduction red, cropped to the full-resolution window win."""
    O.set_decode_reduce(red)
    try:
        dec, _ = O.decode(cs, partial=win is not None)
    finally:
        O.set_decode_reduce(0)
    if win is None:
        return dec
    cd = lambda v: -(-v >> red)
    return dec[:, cd(win[1]):cd(win[3]), cd(win[0]):cd(win[2])]


@pytest.fixture(scope="module")
def images():
    return {k: (synth_image(*a).astype(np.int32), bits) for k, (a, bits) in IMAGES.items()}


@pytest.mark.parametrize("which,flags,grok_bytes,grok_sha", KNOWN + KNOWN_WIDE, ids=[k[1] for k in KNOWN + KNOWN_WIDE])
def test_oracle_equals_grok(images, which, flags, grok_bytes, grok_sha):
    img, bits = images[which]
    cs = O.encode(img, bits, **parse_flags(flags))
    assert len(cs) == grok_bytes, flags
    if grok_sha:
        assert hashlib.sha256(cs).hexdigest()[:16] == grok_sha, flags


@pytest.mark.parametrize("which,flags,red,win,shape,grok_sha", DECODES, ids=["%s %s -r %d" % (d[0], d[1], d[2]) for d in DECODES])
def test_oracle_decode_equals_grok(images, which, flags, red, win, shape, grok_sha):
    img, bits = images[which]
    dec = oracle_reduced(O.encode(img, bits, **parse_flags(flags)), red, win)
    assert dec.shape == shape
    assert u16_sha(dec) == grok_sha


def test_oracle_precinct_exponent_zero(images):
    # -c [32,32] with 6 resolutions: 32, 16, 8, 4, 2, 1 -> exponents 5 .. 0; the COD's last
    # precinct byte (resolution 0) is 0x00 and the stream decodes losslessly
    img, bits = images["A"]
    p = O.params(precincts=[(32, 32)])
    assert [p.prcw_exp[r] for r in range(6)] == [0, 1, 2, 3, 4, 5]
    p = O.params(precincts=[(2, 2)], numres=4)   # 2, 1, 0 -> exponents 1, 0, then clamped 1
    assert [p.prcw_exp[r] for r in range(4)] == [1, 1, 0, 1]
    cs = O.encode(img, bits, precincts=[(32, 32)])
    i = cs.index(b"\xff\x52")
    assert cs[i + 2 + 2 + 10:i + 2 + 2 + 16] == bytes([0x00, 0x11, 0x22, 0x33, 0x44, 0x55])
    np.testing.assert_array_equal(O.decode(cs)[0], img)
    # exponent 0 above resolution 0 has no band partition (B.6): refused, as the engine does
    with pytest.raises(RuntimeError):
        O.encode(img, bits, precincts=[(2, 2)], numres=4)


def test_grok_poc_stream_decodes(images):
    # Grok's -P stream (main-header POC RLCP/LRCP; its tile-part POC lists both entries as the
    # tile's own progression, LRCP): the tile-part list is appended to the main header's
    # (CodeStreamDecompress::read_poc, :1171-1172), so the main header's order rules and the
    # stream decodes at Grok's and OpenJPEG 2.5.4's 31.33 dB
    img, bits = images["A"]
    cs = O.encode(img, bits, **parse_flags("-r 20,10 -P T0=0,0,2,3,3,RLCP/T0=3,0,2,6,3,LRCP"))
    assert hashlib.sha256(cs).hexdigest()[:16] == "0be62df5a6eaa292"
    dec, _ = O.decode(cs)
    mse = ((dec.astype(np.float64) - img) ** 2).mean()
    assert abs(10 * np.log10(255.0 ** 2 / mse) - 31.33) < 0.01


@pytest.mark.parametrize("tiles,numres", [((200, 160), 6), ((24, 40), 6), ((13, 7), 3), ((100, 70), 4)])
def test_odd_parity_tiles_lossless_round_trip(images, tiles, numres):
    # resolutions starting on odd coordinates take the odd ("cas1") lifting (WaveletFwd.cpp:486-489,
    # WaveletReverse.cpp:559-663): the 5/3 path stays lossless
    img, _ = images["A"]
    cs = O.encode(img, 8, tiles=tiles, numres=numres)
    dec, _ = O.decode(cs)
    np.testing.assert_array_equal(dec, img)
