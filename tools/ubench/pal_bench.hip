// pal_bench.hip — times k_jp2_palette (grok_amd/csrc/gk_colour.hip) on one index plane.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I grok_amd/csrc tools/ubench/pal_bench.hip \
//         grok_amd/csrc/gk_colour.hip -o tools/ubench/pal_bench
//   tools/ubench/pal_bench [side = 8192] [entries = 256] [columns = 3] [reps = 20]
// 8-bit indices -> `columns` 8-bit planes; prints every launch time, the median, the bytes
// moved (1 B in + columns B out per sample) and the bandwidth they imply.  tools/ubench/
// pal_torch.py times torch's lut[idx.long()] gather to the same output as the yardstick.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gk_launch.h"

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char** argv) {
    const uint32_t side = argc > 1 ? (uint32_t)atoi(argv[1]) : 8192, ne = argc > 2 ? (uint32_t)atoi(argv[2]) : 256;
    const uint32_t npc = argc > 3 ? (uint32_t)atoi(argv[3]) : 3;
    const int reps = argc > 4 ? atoi(argv[4]) : 20;
    if (!side || side % 16 || !ne || ne > 1024 || !npc || npc > 255 || reps < 1) { fprintf(stderr, "bad arguments\n"); return 2; }
    const size_t n = (size_t)side * side;
    std::vector<uint8_t> idx(n);
    uint32_t s = 12345;
    for (size_t i = 0; i < n; ++i) { s = s * 1664525u + 1013904223u; idx[i] = (uint8_t)(s >> 24); }
    const uint32_t ew = gk_pal_entry_words(npc, 1);
    std::vector<uint8_t> tab((size_t)ne * ew * 4, 0);
    for (uint32_t j = 0; j < ne; ++j)
        for (uint32_t c = 0; c < npc; ++c) tab[(size_t)j * ew * 4 + c] = (uint8_t)(j * 7 + c * 31 + 5);
    uint8_t *didx, *dout, *dtab;
    GkPalChan* dch;
    CHK(hipMalloc(&didx, n));
    CHK(hipMalloc(&dout, n * npc));
    CHK(hipMalloc(&dtab, tab.size()));
    CHK(hipMalloc(&dch, npc * sizeof(GkPalChan)));
    std::vector<GkPalChan> ch(npc);
    for (uint32_t c = 0; c < npc; ++c) {
        ch[c] = GkPalChan{};
        ch[c].dst = dout + n * c; ch[c].dst_stride = side; ch[c].col = c;
    }
    CHK(hipMemcpy(didx, idx.data(), n, hipMemcpyHostToDevice));
    CHK(hipMemcpy(dtab, tab.data(), tab.size(), hipMemcpyHostToDevice));
    CHK(hipMemcpy(dch, ch.data(), npc * sizeof(GkPalChan), hipMemcpyHostToDevice));
    GkPalArgs a{};
    a.idx = didx; a.idx_stride = side; a.w = side; a.h = side;
    a.chans = dch; a.nchan = npc; a.npal = npc;
    a.table = (const uint32_t*)dtab; a.ne = ne; a.entry_words = ew; a.elem_bytes = 1; a.vec_store = 1;
    hipEvent_t e0, e1;
    CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
    int mode = 0;
    for (int i = 0; i < 3; ++i) mode = gk_launch_jp2_palette(nullptr, GK_U8, GK_U8, a);
    CHK(hipDeviceSynchronize());
    std::vector<float> ms(reps);
    for (int i = 0; i < reps; ++i) {
        CHK(hipEventRecord(e0, nullptr));
        gk_launch_jp2_palette(nullptr, GK_U8, GK_U8, a);
        CHK(hipEventRecord(e1, nullptr));
        CHK(hipEventSynchronize(e1));
        CHK(hipEventElapsedTime(&ms[i], e0, e1));
    }
    CHK(hipGetLastError());
    std::vector<uint8_t> out(n * npc);
    CHK(hipMemcpy(out.data(), dout, out.size(), hipMemcpyDeviceToHost));
    size_t bad = 0;
    for (uint32_t c = 0; c < npc; ++c)
        for (size_t i = 0; i < n; i += 4093) {
            const uint32_t k = std::min<uint32_t>(idx[i], ne - 1);
            bad += out[n * c + i] != tab[(size_t)k * ew * 4 + c];
        }
    for (int i = 0; i < reps; ++i) printf("launch %d: %.4f ms\n", i, ms[i]);
    std::sort(ms.begin(), ms.end());
    const double med = ms[reps / 2], bytes = (double)n * (1 + npc);
    printf("k_jp2_palette %ux%u u8 -> %u x u8, %u entries, table path %d: median %.4f ms (min %.4f, max %.4f), %.0f bytes, %.1f GB/s, mismatches %zu\n",
           side, side, npc, ne, mode, med, ms[0], ms[reps - 1], bytes, bytes / med / 1e6, bad);
    return bad ? 3 : 0;
}
