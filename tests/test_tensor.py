"""Float tensors without a GPU: gk_probe_tensor (the layout rule and every refusal of a
description, from a resolved view alone), grok_amd._tensor_affine, the C layout of gk_tensor, and
the numpy restatement of the rule (tests/tensor_ref.py) against torch on the CPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
import grok_amd as G
import oracle as O
import display_cases as C
import tensor_ref as T


@pytest.fixture(scope="module")
def views():
    rgb = O.encode(np.stack(C.random_planes(53, 37, [(1, 1)] * 3, 8, seed=5)), 8, mct=False, numres=3)
    one = O.encode(np.stack(C.random_planes(64, 48, [(1, 1)], 8, seed=6)), 8, mct=False, numres=1)
    return {"rgb": G.probe_view(rgb, size=(20, 13)), "turned": G.probe_view(rgb, size=(20, 13), rotate=90),
            "grey": G.probe_view(one, size=(8, 6)), "row": G.probe_view(rgb, size=(20, 1))}


# ---------------------------------------------------------------- 1. gk_probe_tensor
def test_probe_extents(views):
    v = views["rgb"]                                              # 3 channels, 20 wide, 13 high
    assert (v.channels, v.pix_w, v.pix_h) == (3, 20, 13)
    assert G.probe_tensor(v, "float32", (260, 20, 1)) == 780     # CHW
    assert G.probe_tensor(v, "float16", (1, 60, 3)) == 780       # HWC
    assert G.probe_tensor(v, "bfloat16", (1, 60, 3), on_device=False) == 780
    assert G.probe_tensor(v, np.float32, (260, 20, 1), on_device=False) == 780
    # one image of a (N, 3, 15, 23) batch: 1 + 2 * 345 + 12 * 23 + 19
    assert G.probe_tensor(v, torch.bfloat16, (345, 23, 1)) == 986
    assert G.probe_tensor(v, "float16", (1, 64, 3)) == 1 + 2 + 12 * 64 + 19 * 3   # HWC with padded rows
    assert G.probe_tensor(v, "float32", (13, 1, 39)) == 1 + 2 * 13 + 12 + 19 * 39   # columns outermost: no alias either
    t = views["turned"]                                           # 90 degrees: the written image is 13 wide, 20 high
    assert (t.pix_w, t.pix_h) == (13, 20) and G.probe_tensor(t, "float32", (260, 13, 1)) == 780
    g = views["grey"]                                             # one channel: its stride is ignored, whatever it holds
    for junk in (0, -7, 1, 2 ** 62):
        assert G.probe_tensor(g, "float32", (junk, 8, 1), on_device=False) == 48
    assert G.probe_tensor(views["row"], "float16", (20, -1, 1), on_device=False) == 60   # one row: stride_y ignored
    assert G.probe_tensor(v, "float32", (260, 20, 1), scale=[1, 2, 3], bias=0.5) == 780
    assert G.probe_tensor(v, "float32", (260, 20, 1), scale=list(range(1, 17))) == 780


@pytest.mark.parametrize("needle,kw", [
    ("dtype 0", dict(dtype=0)), ("dtype 4", dict(dtype=4)),
    ("stride_x is 0", dict(strides=(260, 20, 0))), ("stride_c is -260", dict(strides=(-260, 20, 1))),
    ("stride_y is 0", dict(strides=(260, 0, 1))),
    ("overlapping strides: stride_y 19", dict(strides=(260, 19, 1))),      # rows shorter than the image
    ("overlapping strides: stride_c 259", dict(strides=(259, 20, 1))),     # planes one element short
    ("overlapping strides: stride_x 2", dict(strides=(1, 60, 2))),         # HWC with two of three channels' room
    ("overlapping strides", dict(strides=(1, 1, 1))),
    ("must be dense", dict(strides=(345, 23, 1), on_device=False)),
    ("17 scale / bias entries", dict(scale=[1.0] * 17)),
    ("scale entry 1 is not finite", dict(scale=[1.0, float("nan"), 1.0])),
    ("scale entry 0 is not finite", dict(scale=float("inf"))),
    ("bias entry 2 is not finite", dict(bias=[0.0, 0.0, float("-inf")])),
    ("bias entry 0 is not finite", dict(scale=2.0, bias=float("nan"))),
])
def test_probe_refusals(views, needle, kw):
    args = dict(dtype="float32", strides=(260, 20, 1))
    args.update(kw)
    dtype = args.pop("dtype")
    if isinstance(dtype, int):      # (the binding refuses an unknown name itself: the engine is asked directly)
        t = G.Tensor(None, 1, dtype, *args["strides"], 0, None, None)
        msg, ext = ctypes.create_string_buffer(512), ctypes.c_uint64(77)
        assert G.load_library().gk_probe_tensor(ctypes.byref(views["rgb"]), ctypes.byref(t), ctypes.byref(ext), msg, 512) == -1
        assert needle in msg.value.decode() and ext.value == 77
        return
    with pytest.raises(ValueError, match=needle):
        G.probe_tensor(views["rgb"], dtype, **args)


def test_probe_raw_refusals(views):
    lib = G.load_library()
    msg, ext = ctypes.create_string_buffer(512), ctypes.c_uint64(0)
    one = (ctypes.c_float * 1)(1.0)
    fp = ctypes.cast(one, ctypes.POINTER(ctypes.c_float))

    def ask(t, view=views["rgb"]):
        rc = lib.gk_probe_tensor(ctypes.byref(view) if view is not None else None, ctypes.byref(t) if t is not None else None,
                                 ctypes.byref(ext), msg, 512)
        return rc, msg.value.decode()

    assert ask(None) == (-1, "tensor: no description")
    assert ask(G.Tensor(None, 1, 1, 260, 20, 1, 0, None, None), view=None) == (-1, "tensor: no view")
    assert ask(G.Tensor(None, 1, 1, 260, 20, 1, 1, None, fp)) == (-1, "tensor: n = 1 without scale")
    assert ask(G.Tensor(None, 1, 1, 260, 20, 1, 1, fp, None)) == (-1, "tensor: n = 1 without bias")
    assert ask(G.Tensor(None, 1, 1, 260, 20, 1, 1, fp, fp))[0] == 0 and ext.value == 780
    # a device pointer is judged by its value alone: never read
    assert ask(G.Tensor(0x1002, 1, 2, 260, 20, 1, 0, None, None))[0] == 0
    rc, why = ask(G.Tensor(0x1002, 1, 1, 260, 20, 1, 0, None, None))
    assert rc == -1 and "not aligned" in why
    rc, why = ask(G.Tensor(0x1001, 1, 3, 260, 20, 1, 0, None, None))
    assert rc == -1 and "not aligned" in why
    with pytest.raises(ValueError, match="dtype"):
        G.probe_tensor(views["rgb"], "int8", (260, 20, 1))


# ---------------------------------------------------------------- 2. _tensor_affine
def test_affine_is_float64_rounded_once():
    s, b = G._tensor_affine(0.485, 0.229, prec=16)
    assert s.dtype == b.dtype == np.float32 and s.shape == b.shape == (1,)
    assert s[0] == np.float32(1.0 / (65535.0 * 0.229)) and b[0] == np.float32(-0.485 / 0.229)
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    s, b = G._tensor_affine(mean, std, prec=8)
    assert s.tolist() == [np.float32(1.0 / (255.0 * d)) for d in std]
    assert b.tolist() == [np.float32(-m / d) for m, d in zip(mean, std)]
    s, b = G._tensor_affine(mean, 0.5, unit=2047, sgnd=True)      # a number repeats; a unit serves a signed view
    assert s.tolist() == [np.float32(1.0 / (2047.0 * 0.5))] * 3 and b.tolist() == [np.float32(-m / 0.5) for m in mean]
    s, b = G._tensor_affine(None, None, prec=10)
    assert s.tolist() == [np.float32(1.0 / 1023.0)] and b.tolist() == [0.0]
    with pytest.raises(ValueError, match="signed"):
        G._tensor_affine(0.5, 0.5, prec=12, sgnd=True)


# ---------------------------------------------------------------- 3. the C layout
def test_tensor_struct_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include "grok_amd.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void){printf("%zu %zu %zu %zu %u %u %u\\n", sizeof(gk_tensor), offsetof(gk_tensor, stride_c),'
                   ' offsetof(gk_tensor, n), offsetof(gk_tensor, bias), GK_TENSOR_F32, GK_TENSOR_F16, GK_TENSOR_BF16);'
                   'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(G.Tensor), G.Tensor.stride_c.offset, G.Tensor.n.offset, G.Tensor.bias.offset,
                   G.GK_TENSOR_F32, G.GK_TENSOR_F16, G.GK_TENSOR_BF16]
    assert {"gk_probe_tensor", "gk_decode_view_tensor"} <= set(G.EXPORTS)


# ---------------------------------------------------------------- 4. the restatement against torch on the CPU
def _torch_rule(v, scale, bias, dtype):
    z = torch.from_numpy(v).to(torch.float32) * torch.tensor(scale, dtype=torch.float32) + torch.tensor(bias, dtype=torch.float32)
    if dtype == "float32":
        return z.numpy().view(np.uint32)
    return z.to(torch.float16 if dtype == "float16" else torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_reference_equals_torch_cpu(dtype):
    rng = np.random.default_rng(11)
    scale, bias = G._tensor_affine(0.485, 0.1 if dtype == "float16" else 0.229, prec=16)
    v = np.concatenate([np.arange(0, 65536, 13), rng.integers(0, 65536, 3000)]).astype(np.int32).reshape(-1, 1, 1)
    want = _torch_rule(v, float(scale[0]), float(bias[0]), dtype)
    np.testing.assert_array_equal(T.bits(T.apply(v, scale, bias, dtype, "hwc")), want)
    # signed values past 2^24, where int32 -> float32 rounds, and per-channel constants
    w = rng.integers(-2 ** 31, 2 ** 31, (40, 25, 3)).astype(np.int32)
    w[0, :6, 0] = [2 ** 24 + 1, 2 ** 24 + 3, 2 ** 25 - 1, -2 ** 24 - 1, 2 ** 31 - 1, -2 ** 31]
    sc, bi = [1.0 / 3, 1e-3, 7.0], [0.25, -1.5, 1e5]
    for k in range(3):
        want = _torch_rule(w[:, :, k], sc[k], bi[k], dtype)
        got = T.bits(T.apply(w, sc, bi, dtype, "chw"))[k]
        np.testing.assert_array_equal(got, want)


def test_a_fused_multiply_add_is_caught():
    """The reason the comparisons can be exact: one rounding where the rule has two differs often."""
    scale, bias = G._tensor_affine(0.485, 0.229, prec=16)
    v = np.arange(65536, dtype=np.int32).reshape(-1, 1, 1)
    two = T.apply(v, scale, bias, "float32", "hwc").reshape(-1)
    fused = (v.reshape(-1).astype(np.float64) * np.float64(scale[0]) + np.float64(bias[0])).astype(np.float32)   # exact product and sum, one rounding
    assert (two != fused).mean() > 0.2                            # (about half of them, here)


def test_reference_rounds_to_even_and_refuses_subnormals():
    v = np.array([[[2 ** 24 + 1], [2 ** 24 + 3], [2 ** 25 - 1]]], np.int32)
    assert T.apply(v, dtype="float32", layout="hwc").reshape(-1).tolist() == [2.0 ** 24, 2.0 ** 24 + 4, 2.0 ** 25]
    assert T.bfloat16_bits(np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, np.inf, -np.inf], np.float32)).tolist() == \
        [0x3F80, 0x3F82, 0x7F80, 0xFF80]                          # halves go to the even neighbour; infinities pass
    one = np.ones((1, 1, 1), np.int32)
    with pytest.raises(AssertionError, match="subnormal"):
        T.apply(one, 1e-5, 0.0, "float16")
    with pytest.raises(AssertionError, match="subnormal"):
        T.apply(one, 1e-39, 0.0, "float32")
    assert T.apply(one, 1e-5, 0.0, "bfloat16").shape == (1, 1, 1)
