// HT 9/7 quantisation control (gk_set_encode_quant): the distortion statistics of the float
// coefficients and the length sum of a coded pass.  Both are two-stage reductions with a fixed
// order: per-lane accumulation, a wave tree, the workgroup's waves in order, one partial per
// workgroup, and a second kernel that adds the partials in index order.  No atomics: the results
// are the same bits on every run.
#include "gk_launch.h"

#define HTQ_WG 256

// Sum of a wave's 64 values, the same tree in every wave (xor butterflies: every lane ends with it).
__device__ __forceinline__ float htq_wave_sum(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ uint64_t htq_wave_sum(uint64_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor((unsigned long long)v, d, 64);
    return v;
}

// ---- k_htq_dist: D[n] = sum (|x| - trunc(|x| * (1 / step_n)) * step_n)^2 over the coefficients
// of one work item (blocks of one band class: component, resolution, orientation), for the
// GK_HTQ_RUNGS steps [n0, n0 + GK_HTQ_RUNGS) of the class's step list.  The index is the
// encoder's (k_ht_enc: the float coefficient times the reciprocal step, truncated), the
// reconstruction point the lower edge of the bin: the estimate's, and a cautious one, since
// k_ht_dec rebuilds a non-zero index at the centre of its bin, as Grok's decoder does.
//
// Registers: GK_HTQ_RUNGS float accumulators per lane, and the compiler keeps the rungs' steps and
// reciprocals (read once from LDS) in registers too: its resource report gives 138 VGPRs at 32
// rungs, 3 waves per SIMD; the whole ladder of a 16-bit image (121 notches) would not fit at all,
// so the ladder takes one launch per 32 notches.  A coefficient costs one 4-byte load against 4
// operations per rung.  Measured on a 4096 x 4096 image (514 workgroups, 67 MB of coefficients):
// 93 us per launch, i.e. 0.72 TB/s read (11 % of the 6.29 TB/s copy rate) and 23 T lane-operations
// per second (about 30 % of the FP32 vector rate): the launch is held by neither, it is short
// and two waves per SIMD wide.  Work items of 2 blocks instead of 8 quadruple the workgroups:
// over the same twelve calls k_htq_dist then took 2.76 ms instead of 3.74, but k_htq_dist_sum's
// serial walk over four times the partials 1.00 ms instead of 0.27: 8 stays
// (profiles/htq_bench.txt).
__global__ __launch_bounds__(HTQ_WG) void k_htq_dist(const float* __restrict__ coef, const GkBlock* __restrict__ blocks,
                                                     const uint32_t* __restrict__ order,
                                                     const GkHtqItem* __restrict__ items, const float* __restrict__ steps,
                                                     uint32_t nsteps, uint32_t n0, float* __restrict__ partial) {
    __shared__ float s_step[GK_HTQ_RUNGS], s_inv[GK_HTQ_RUNGS];
    __shared__ float s_red[HTQ_WG / 64][GK_HTQ_RUNGS];
    const uint32_t tid = threadIdx.x;
    const GkHtqItem it = items[blockIdx.x];
    const uint32_t nn = min((uint32_t)GK_HTQ_RUNGS, nsteps - n0);
    if (tid < GK_HTQ_RUNGS) {
        const float s = tid < nn ? steps[(size_t)it.cls * nsteps + n0 + tid] : 1.0f;
        s_step[tid] = s;
        s_inv[tid] = 1.0f / s;
    }
    __syncthreads();
    float acc[GK_HTQ_RUNGS];
#pragma unroll
    for (int j = 0; j < GK_HTQ_RUNGS; ++j) acc[j] = 0.0f;
    for (uint32_t k = 0; k < it.count; ++k) {
        const GkBlock G = blocks[order[it.first + k]];
        const float* src = coef + G.band_off;
        const uint32_t w = G.w, n = (uint32_t)G.w * G.h, stride = G.stride;
        for (uint32_t i = tid; i < n; i += HTQ_WG) {
            const uint32_t y = i / w, x = i - y * w;
            const float a = fabsf(src[(size_t)y * stride + x]);
#pragma unroll
            for (int j = 0; j < GK_HTQ_RUNGS; ++j) {
                const float q = truncf(a * s_inv[j]);
                const float e = fmaf(-q, s_step[j], a);
                acc[j] = fmaf(e, e, acc[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < GK_HTQ_RUNGS; ++j) {
        const float v = htq_wave_sum(acc[j]);
        if ((tid & 63) == 0) s_red[tid >> 6][j] = v;
    }
    __syncthreads();
    if (tid < nn) {
        float v = s_red[0][tid];
#pragma unroll
        for (int wv = 1; wv < HTQ_WG / 64; ++wv) v += s_red[wv][tid];
        partial[(size_t)blockIdx.x * nsteps + n0 + tid] = v;
    }
}

// Second stage: out[cls][n] = the partials of the class's items, added in item order, in double.
__global__ __launch_bounds__(HTQ_WG) void k_htq_dist_sum(const float* __restrict__ partial,
                                                         const uint32_t* __restrict__ cls_first, uint32_t ncls,
                                                         uint32_t nsteps, double* __restrict__ out) {
    const uint32_t i = blockIdx.x * HTQ_WG + threadIdx.x;
    if (i >= ncls * nsteps) return;
    const uint32_t cls = i / nsteps, n = i - cls * nsteps;
    double s = 0.0;
    for (uint32_t q = cls_first[cls]; q < cls_first[cls + 1]; ++q) s += (double)partial[(size_t)q * nsteps + n];
    out[i] = s;
}

void gk_launch_htq_dist(hipStream_t st, const float* coef, const GkBlock* blocks, const uint32_t* order,
                        const GkHtqItem* items, uint32_t nitems, const float* steps, uint32_t nsteps,
                        const uint32_t* cls_first, uint32_t ncls, float* partial, double* out) {
    if (!nitems || !nsteps || !ncls) return;
    for (uint32_t n0 = 0; n0 < nsteps; n0 += GK_HTQ_RUNGS)
        hipLaunchKernelGGL(k_htq_dist, dim3(nitems), dim3(HTQ_WG), 0, st, coef, blocks, order, items, steps, nsteps, n0,
                           partial);
    hipLaunchKernelGGL(k_htq_dist_sum, dim3((ncls * nsteps + HTQ_WG - 1) / HTQ_WG), dim3(HTQ_WG), 0, st, partial, cls_first,
                       ncls, nsteps, out);
}

// ---- k_htq_len: the bytes of a coded HT pass and a lower bound of its packet-header bits, from
// the encoder's per-block results (info: 4 words per block, [1] passes, [2] bytes).  A block's
// first (and only) packet header holds at least its inclusion bit, one zero-bit-plane tag-tree
// bit, the one-pass code, the Lblock increments (a comma code of k + 1 bits) and the length in
// 3 + k bits, k = max(0, bits(len) - 3); a block that was not coded its inclusion bit.
__device__ __forceinline__ uint32_t htq_header_bits(uint32_t passes, uint32_t len) {
    if (!passes) return 1;
    const uint32_t nb = 32 - __clz(len | 1u);
    const uint32_t k = nb > 3 ? nb - 3 : 0;
    return 7 + 2 * k;
}
__device__ __forceinline__ void htq_wg_sum(uint64_t a, uint64_t b, uint64_t* dst) {
    __shared__ uint64_t s_a[HTQ_WG / 64], s_b[HTQ_WG / 64];
    a = htq_wave_sum(a); b = htq_wave_sum(b);
    if ((threadIdx.x & 63) == 0) { s_a[threadIdx.x >> 6] = a; s_b[threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t x = 0, y = 0;
        for (int wv = 0; wv < HTQ_WG / 64; ++wv) { x += s_a[wv]; y += s_b[wv]; }
        dst[0] = x; dst[1] = y;
    }
}
__global__ __launch_bounds__(HTQ_WG) void k_htq_len(const uint32_t* __restrict__ info, uint32_t nblocks,
                                                    uint64_t* __restrict__ partial) {
    uint64_t bytes = 0, bits = 0;
    const uint32_t i0 = blockIdx.x * (HTQ_WG * GK_HTQ_LEN_PER);
    for (uint32_t k = 0; k < GK_HTQ_LEN_PER; ++k) {
        const uint32_t i = i0 + k * HTQ_WG + threadIdx.x;
        if (i < nblocks) {
            const uint4 v = reinterpret_cast<const uint4*>(info)[i];
            bytes += v.z;
            bits += htq_header_bits(v.y, v.z);
        }
    }
    htq_wg_sum(bytes, bits, partial + 2 * (size_t)blockIdx.x);
}
__global__ __launch_bounds__(HTQ_WG) void k_htq_len_sum(const uint64_t* __restrict__ partial, uint32_t n,
                                                        uint64_t* __restrict__ out) {
    uint64_t bytes = 0, bits = 0;
    for (uint32_t i = threadIdx.x; i < n; i += HTQ_WG) { bytes += partial[2 * (size_t)i]; bits += partial[2 * (size_t)i + 1]; }
    htq_wg_sum(bytes, bits, out);
}

uint32_t gk_htq_len_partials(uint32_t nblocks) { return (nblocks + HTQ_WG * GK_HTQ_LEN_PER - 1) / (HTQ_WG * GK_HTQ_LEN_PER); }

void gk_launch_htq_len(hipStream_t st, const uint32_t* info, uint32_t nblocks, uint64_t* partial, uint64_t* out) {
    const uint32_t np = gk_htq_len_partials(nblocks);
    if (!np) return;
    hipLaunchKernelGGL(k_htq_len, dim3(np), dim3(HTQ_WG), 0, st, info, nblocks, partial);
    hipLaunchKernelGGL(k_htq_len_sum, dim3(1), dim3(HTQ_WG), 0, st, partial, np, out);
}
