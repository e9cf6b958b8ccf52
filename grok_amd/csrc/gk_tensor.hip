// gk_tensor.hip — the last stage of gk_decode_view_tensor: the decoded region, rw x rh packed int32
// pixels on the reduced canvas, resampled to exactly ow x oh pixels, mirrored and rotated as k_view
// does (gk_view.hip), and written as a normalised float tensor in the caller's strides.
//
// The rule (include/grok_amd.h; tests/tensor_ref.py is the same arithmetic in numpy).
// v is the int32 the view returns for channel k of written pixel (x, y): gk_area_pixel, the one
// definition k_view, k_render and k_levels share.  Then three IEEE operations in a fixed order,
//     f = float32(v)     g = f * scale_k     z = g + bias_k        each rounded to nearest even
// and z is stored as float32, or rounded to nearest even once more to float16 or bfloat16.  The
// multiplication and the addition are never fused: an FMA rounds once where the rule rounds twice,
// and the results differ in a third of all 16-bit inputs.  So the file and the function that holds
// the two operations compile under fp contract(off), and the operations are the plain operators:
// written as __fmul_rn / __fadd_rn, which HIP's headers define outside the pragma, they came out
// as one v_fmac_f32 in the float32 and bfloat16 kernels even under the file's pragma (read in the
// ISA; DESIGN.md §3 and §8 record the same of the 9/7 and colour kernels).  As it stands the code
// object's only v_fma / v_fmac are those of the integer divisions.  bfloat16 is rounded on the
// float32's bits in integers; z is never a NaN (v, scale and bias are finite), and an infinity
// passes through unchanged.
//
// Shape.  The geometry of k_view: a 256-thread block owns a 16 x 16 tile of the output in
// pre-rotation coordinates, and the lanes of a 16-lane group run along the axis that becomes the
// written image's x, the tile's columns for rotate 0 / 180 and its rows for 90 / 270.  A lane
// computes four channels at a time and stores each at k stride_c + y stride_y + x stride_x.  With
// the lanes along x a planar (CHW) store is one run of 16 elements per group and channel, 64 bytes
// of float32 or 32 bytes of float16 / bfloat16, and a packed (HWC) store is one contiguous run of
// 16 C elements per group, written a channel at a time as k_view writes its pixels.  This was
// decided from the code, not measured; a tile wider than 16 along x for planar 16-bit output (full
// 64-byte runs) is a later, measured question.
// Every source index is checked against rw / rh and every written position against pix_w / pix_h.
// No atomics, no LDS, no inline assembly.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gk_common.h"
#include "gk_launch.h"
#include "gk_area.h"

#pragma clang fp contract(off)

namespace {
constexpr int TILE = GK_AREA_TILE;
constexpr int CG = GK_AREA_CG;

struct Bf16 { uint16_t bits; };   // (the element type of a bfloat16 tensor: its bits)

// g = f * scale, z = g + bias: two roundings
__device__ __forceinline__ float tensor_affine(float f, float scale, float bias) {
#pragma clang fp contract(off)
    const float g = f * scale;
    return g + bias;
}

template <typename DST> __device__ __forceinline__ DST tensor_element(float z);
template <> __device__ __forceinline__ float tensor_element<float>(float z) { return z; }
template <> __device__ __forceinline__ _Float16 tensor_element<_Float16>(float z) { return (_Float16)z; }   // round to nearest even
template <> __device__ __forceinline__ Bf16 tensor_element<Bf16>(float z) {
    const uint32_t u = __float_as_uint(z);
    return Bf16{(uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16)};   // round to nearest even on the bits
}

template <typename DST>
__global__ __launch_bounds__(256) void k_tensor(GkTensorArgs t) {
    const GkViewArgs& a = t.v;
    const uint32_t lo = threadIdx.x & (TILE - 1), hi = threadIdx.x >> 4;
    // the fast lane index along the written image's x
    const uint32_t bx = blockIdx.x % a.tiles_x, by = blockIdx.x / a.tiles_x;
    const uint32_t i = bx * TILE + (a.swap ? hi : lo);   // output column before orientation
    const uint32_t j = by * TILE + (a.swap ? lo : hi);   // output row before orientation
    if (i >= a.ow || j >= a.oh) return;
    // orientation: mirror left-right, then rotate clockwise
    const uint32_t im = a.mirror ? a.ow - 1 - i : i;
    uint32_t px, py;
    switch (a.rot) {
        case 1: px = a.oh - 1 - j; py = im; break;              // 90
        case 2: px = a.ow - 1 - im; py = a.oh - 1 - j; break;   // 180
        case 3: px = j; py = a.ow - 1 - im; break;              // 270
        default: px = im; py = j; break;
    }
    if (px >= a.pix_w || py >= a.pix_h) return;
    DST* d = (DST*)a.dst + ((int64_t)py * t.stride_y + (int64_t)px * t.stride_x);
    const int32_t* src = (const int32_t*)a.src;
    const uint32_t C = a.nch;
    for (uint32_t c0 = 0; c0 < C; c0 += CG) {
        int32_t v[CG];
        gk_area_pixel(src, a.rw, a.rh, a.ow, a.oh, C, i, j, c0, v);
#pragma unroll
        for (int k = 0; k < CG; ++k) {
            if (c0 + k >= C) continue;
            const float z = tensor_affine((float)v[k], t.scale[c0 + k], t.bias[c0 + k]);
            d[(int64_t)(c0 + k) * t.stride_c] = tensor_element<DST>(z);
        }
    }
}
}  // namespace

int gk_launch_tensor(hipStream_t st, uint32_t dtype, const GkTensorArgs& args) {
    GkTensorArgs t = args;
    GkViewArgs& a = t.v;
    if (!a.src || !a.dst || dtype < GK_TT_F32 || dtype > GK_TT_BF16) return -1;
    if (!a.ow || !a.oh || !a.rw || !a.rh || !a.nch || a.nch > GK_PIX_MAX_CH || a.ow > a.rw || a.oh > a.rh || a.rot > 3) return -1;
    a.swap = a.rot & 1;
    a.pix_w = a.swap ? a.oh : a.ow;
    a.pix_h = a.swap ? a.ow : a.oh;
    a.tiles_x = (a.ow + TILE - 1) / TILE;
    const uint64_t tiles = (uint64_t)a.tiles_x * ((a.oh + TILE - 1) / TILE);   // (one grid axis: no 65535-row limit)
    if (tiles > GK_VIEW_MAX_TILES) return -1;
    const dim3 grid((uint32_t)tiles);
    if (dtype == GK_TT_F32) hipLaunchKernelGGL((k_tensor<float>), grid, dim3(256), 0, st, t);
    else if (dtype == GK_TT_F16) hipLaunchKernelGGL((k_tensor<_Float16>), grid, dim3(256), 0, st, t);
    else hipLaunchKernelGGL((k_tensor<Bf16>), grid, dim3(256), 0, st, t);
    return 0;
}
