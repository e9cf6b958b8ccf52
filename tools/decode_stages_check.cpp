// Host-only check of the decode core's stages (gk_engine.cpp: tile_rect, blocks_needed,
// fill_table, solo_split, lane_layout, output_rects) on small plans with generated packet state.
// No GPU call is made.  Build: as tools/pool_stress.cpp (tests/test_decode_stages.py); run with
// no arguments.  Exits non-zero with a message on the first failure.
#ifndef ENGINE_SRC
#define ENGINE_SRC "../grok_amd/csrc/gk_engine.cpp"
#endif
#include ENGINE_SRC
#include <random>

#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("FAILED %s:%d (%s): ", __FILE__, __LINE__, #cond);        \
            printf(__VA_ARGS__);                                             \
            printf("\n");                                                    \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

// 200 x 150 at canvas origin (3, 5), 3 components (1 and 2 subsampled sdx x sdy), 3 resolutions,
// 16 x 16 code-blocks (cb = 4; cb = 2: 4 x 4, enough blocks for fill_table to take the pool);
// tiled: 64 x 48 tiles (16, partial at two edges), else one tile
static Plan make_plan(bool irrev, uint32_t sdx, uint32_t sdy, bool tiled, uint32_t sty, uint32_t cb = 4) {
    Plan P;
    P.w = 200; P.h = 150; P.x0 = 3; P.y0 = 5; P.nc = 3; P.prec = 8; P.sgnd = 0;
    P.cdx = {1, (uint8_t)sdx, (uint8_t)sdx}; P.cdy = {1, (uint8_t)sdy, (uint8_t)sdy};
    P.p.numres = 3; P.p.cbw = cb; P.p.cbh = cb; P.p.irrev = irrev; P.p.mct = 0; P.p.cblk_sty = sty;
    if (tiled) { P.p.tw = 64; P.p.th = 48; }
    for (int i = 0; i < GK_MAXRLVLS; ++i) { P.p.prcw[i] = 15; P.p.prch[i] = 15; }
    build_plan(P);
    CHECK(P.tiles.size() == (tiled ? 16u : 1u), "%zu tiles", P.tiles.size());
    return P;
}
static std::vector<TilePart> parts_of(const Plan& P, const uint32_t* win, int drop) {
    std::vector<TilePart> parts;
    for (uint32_t t = 0; t < P.tiles.size(); ++t) {
        const TileG& T = P.tiles[t];
        if ((int)t == drop) continue;
        if (win && !(T.x0 - P.x0 < win[2] && win[0] < T.x1 - P.x0 && T.y0 - P.y0 < win[3] && win[1] < T.y1 - P.y0)) continue;
        TilePart tp{};
        tp.tile = t;
        parts.push_back(tp);
    }
    return parts;
}
// packet state as a parse might leave it: lengths, numbps, pass counts (0 included), segment lists
static std::vector<PartState> gen_states(const Plan& P, const std::vector<TilePart>& parts, bool multiseg, std::mt19937& rng) {
    std::vector<PartState> ps(parts.size());
    for (size_t q = 0; q < parts.size(); ++q) {
        const TileG& T = P.tiles[parts[q].tile];
        const uint32_t n = T.b1 - T.b0;
        PartState& s = ps[q];
        s.included.assign(n, 1); s.numbps.resize(n); s.npasses.resize(n); s.numlenbits.assign(n, 3); s.len.resize(n);
        if (multiseg) { s.seglens.assign(n, {}); s.segp.assign(n, 0); }
        for (uint32_t b = 0; b < n; ++b) {
            s.numbps[b] = (uint8_t)(rng() % 13);
            s.npasses[b] = (uint16_t)(rng() % 5 == 0 ? 0 : rng() % 34);
            s.len[b] = rng() % 4 == 0 ? 0 : 1 + rng() % 300;
            if (multiseg)
                for (uint32_t k = rng() % 5; k; --k) s.seglens[b].push_back(rng() % 97);
        }
    }
    return ps;
}
static std::vector<std::vector<uint8_t>> needs(const Plan& P, const std::vector<TilePart>& parts, const TileRect& TR, const uint32_t* win) {
    const uint32_t cw[4] = {TR.rx0 + P.x0, TR.ry0 + P.y0, TR.rx1 + P.x0, TR.ry1 + P.y0};
    std::vector<std::vector<uint8_t>> need(parts.size());
    for (size_t q = 0; q < parts.size(); ++q) blocks_needed(P, P.tiles[parts[q].tile], win ? cw : nullptr, need[q]);
    return need;
}

// ---- 1. fill_table against a plain serial fill in table order
static void check_fill(const char* name, const Plan& P, const uint32_t* win, int drop, std::mt19937& rng, bool pool = false) {
    bool multiseg = false;
    for (uint32_t c = 0; c < P.nc; ++c) multiseg = multiseg || (P.p.c_sty(c) & (GK_STY_LAZY | GK_STY_TERMALL));
    const std::vector<TilePart> parts = parts_of(P, win, drop);
    const TileRect TR = tile_rect(P, parts, win, false);
    const std::vector<std::vector<uint8_t>> need = needs(P, parts, TR, win);
    const std::vector<PartState> ps = gen_states(P, parts, multiseg, rng);
    size_t nmax = 0, nall = 0;
    for (const auto& nd : need) { nmax += (size_t)std::count(nd.begin(), nd.end(), (uint8_t)1); nall += nd.size(); }
    if (win) CHECK(nmax < nall, "%s: the window drops no block", name);
    CHECK(pool == (nall >= 1024), "%s: %zu blocks, fill_table takes the pool from 1,024", name, nall);
    std::vector<GkBlock> got(nmax + 1), ref(nmax + 1);
    memset(got.data(), 0, got.size() * sizeof(GkBlock)); memset(ref.data(), 0, ref.size() * sizeof(GkBlock));
    const BlockTable BT = fill_table(P, TR, need, ps, got.data());
    // the restatement
    uint32_t n = 0;
    uint64_t oo = 0, t1 = 0;
    std::vector<uint32_t> seglen;
    std::vector<std::vector<int32_t>> idx(parts.size());
    for (uint32_t t = 0; t < P.tiles.size(); ++t) {
        const uint32_t i = t % P.ntx, j = t / P.ntx;
        if (i < TR.ib || i >= TR.ie || j < TR.jb || j >= TR.je || TR.part_of[t] < 0) continue;
        const int32_t q = TR.part_of[t];
        const TileG& T = P.tiles[t];
        idx[q].assign(T.b1 - T.b0, -1);
        for (uint32_t b = T.b0; b < T.b1; ++b) {   // Plan::blocks is in table order within a tile
            const uint32_t lb = b - T.b0;
            if (!need[q][lb]) continue;
            GkBlock G = P.blocks[b];
            const BandG* B = nullptr;
            for (const ResG& R : T.comps[G.comp].res)
                for (uint32_t bi = 0; bi < R.bands.size(); ++bi)
                    for (const PrecG& PG : R.prc[bi])
                        if (b >= PG.first_block && b < PG.first_block + PG.cw * PG.ch) B = &R.bands[bi];
            CHECK(B, "%s: block %u in no precinct", name, b);
            G.band_off = relocate(P, TR.RGg[P.group_of[G.comp]], G.band_off);
            G.stride = TR.RG.stride; G.band_numbps = (uint8_t)B->numbps; G.step = B->step_dec / 2.0f;
            G.numbps = ps[q].numbps[lb]; G.len = ps[q].len[lb]; G.npasses = G.len ? ps[q].npasses[lb] : 0;
            if (multiseg) { G.data_cap = (uint32_t)seglen.size(); seglen.insert(seglen.end(), ps[q].seglens[lb].begin(), ps[q].seglens[lb].end()); }
            G.data_off = oo;
            idx[q][lb] = (int32_t)n;
            ref[n++] = G;
            t1 += G.len; oo += (((uint64_t)G.len + 15) & ~15ull) + 32;
        }
    }
    CHECK(BT.nblk == n && n == nmax, "%s: %u blocks, %u expected (%zu needed)", name, BT.nblk, n, nmax);
    CHECK(BT.staged == oo && BT.t1_bytes == t1, "%s: staged %llu / %llu, T1 bytes %llu / %llu", name, (unsigned long long)BT.staged,
          (unsigned long long)oo, (unsigned long long)BT.t1_bytes, (unsigned long long)t1);
    for (uint32_t k = 0; k < n; ++k)
        CHECK(!memcmp(&got[k], &ref[k], sizeof(GkBlock)), "%s: table entry %u differs (comp %u / %u, data_off %llu / %llu)", name, k,
              got[k].comp, ref[k].comp, (unsigned long long)got[k].data_off, (unsigned long long)ref[k].data_off);
    CHECK(BT.seglen == seglen, "%s: segment lengths differ (%zu / %zu)", name, BT.seglen.size(), seglen.size());
    CHECK(BT.part_idx == idx, "%s: part_idx differs", name);
}

// ---- 2. blocks_needed
static void check_needed(const Plan& P, std::mt19937& rng) {
    for (const TileG& T : P.tiles) {
        std::vector<uint8_t> all, a, b;
        const uint32_t cover[4] = {T.x0 > 2 ? T.x0 - 2 : 0, T.y0, T.x1, T.y1 + 7};
        blocks_needed(P, T, cover, all);
        CHECK(std::count(all.begin(), all.end(), (uint8_t)1) == (long)all.size(), "a covering window drops blocks");
        for (int it = 0; it < 20; ++it) {   // nested windows inside the tile
            const uint32_t w = T.x1 - T.x0, h = T.y1 - T.y0;
            auto rnd = [&](uint32_t m) { return (uint32_t)(rng() % m); };
            uint32_t B[4] = {T.x0 + rnd(w), T.y0 + rnd(h), 0, 0};
            B[2] = B[0] + 1 + rng() % (T.x1 - B[0]); B[3] = B[1] + 1 + rng() % (T.y1 - B[1]);
            uint32_t A[4] = {B[0] + rnd(B[2] - B[0]), B[1] + rnd(B[3] - B[1]), 0, 0};
            A[2] = A[0] + 1 + rng() % (B[2] - A[0]); A[3] = A[1] + 1 + rng() % (B[3] - A[1]);
            blocks_needed(P, T, A, a);
            blocks_needed(P, T, B, b);
            for (size_t k = 0; k < a.size(); ++k) CHECK(!a[k] || b[k], "need(A) is not within need(B) at block %zu", k);
            // one sample: a block of every band that has blocks, of every component with a sample there
            const uint32_t one[4] = {A[0], A[1], A[0] + 1, A[1] + 1};
            blocks_needed(P, T, one, a);
            for (uint32_t c = 0; c < P.nc; ++c) {
                if (ceildiv(one[0], P.sx(c)) == ceildiv(one[2], P.sx(c)) || ceildiv(one[1], P.sy(c)) == ceildiv(one[3], P.sy(c))) continue;
                for (uint32_t r = 0; r < T.comps[c].res.size(); ++r) {
                    const ResG& R = T.comps[c].res[r];
                    for (uint32_t bi = 0; bi < R.bands.size(); ++bi) {
                        uint32_t have = 0, needed = 0;
                        for (const PrecG& PG : R.prc[bi])
                            for (uint32_t k = 0; k < PG.cw * PG.ch; ++k) { ++have; needed += a[PG.first_block + k - T.b0]; }
                        CHECK(!have || needed, "sample (%u, %u): no block of component %u resolution %u band %u", one[0], one[1], c, r, bi);
                    }
                }
            }
        }
    }
}

// ---- 3. solo_split
static std::vector<GkBlock> weights(int kind, uint32_t n, std::mt19937& rng) {
    std::vector<GkBlock> blk(n);
    memset(blk.data(), 0, n * sizeof(GkBlock));
    for (uint32_t q = 0; q < n; ++q) {
        blk[q].npasses = 1 + rng() % 30; blk[q].numbps = 1 + rng() % 12;
        blk[q].len = kind == 0 ? 500 : 400 + rng() % 40;
        if (kind == 1 && (q == n / 5 || q == n / 2 || q == n - 1)) blk[q].len = 900 + q % 7;   // a plateau with three outliers
        if (kind == 2 && q % 3 == 0) { if (q % 2) blk[q].npasses = 0; else blk[q].len = 0; }   // weight-0 blocks
    }
    return blk;
}
static uint64_t wgt(const GkBlock& G) { return G.npasses ? G.len : 0; }
static void check_solo(std::mt19937& rng) {
    const int forced[] = {-1, 0, 5, 13};
    const uint32_t packed[] = {0, 12, 24};
    for (int kind = 0; kind < 3; ++kind)
        for (uint32_t n : {7u, 1000u})
            for (int variant = 0; variant < 6; ++variant)
                for (int shared = 0; shared < (variant < 3 ? 2 : 1); ++shared) {   // (the shared rule needs forced < 0)
                    const std::vector<GkBlock> blk = weights(kind, n, rng);
                    GkSoloPlan sp{0, -1, 2.5f};
                    if (variant < 3) sp.waves = packed[variant];
                    else { sp.forced = (int)std::min<uint32_t>((uint32_t)forced[variant - 2], n); sp.waves = ((uint32_t)sp.forced + 11) / 12 * 12; }
                    std::vector<std::vector<uint32_t>> bins;
                    const uint32_t nsb = solo_split(blk.data(), n, sp, shared != 0, bins);
                    std::vector<uint32_t> order(n);   // heaviest first, ties by lower index
                    for (uint32_t q = 0; q < n; ++q) order[q] = q;
                    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return wgt(blk[x]) > wgt(blk[y]); });
                    std::vector<uint32_t> seen(n, 0);
                    uint32_t tot = 0;
                    CHECK(bins.size() <= sp.waves, "%zu bins for %u waves", bins.size(), sp.waves);
                    for (const auto& b : bins) {
                        CHECK(b.size() <= 64, "a bin of %zu blocks", b.size());
                        for (uint32_t q : b) { CHECK(q < n && !seen[q]++, "block %u in two bins", q); ++tot; }
                    }
                    CHECK(tot == nsb, "%u blocks in bins, %u solo", tot, nsb);
                    if (!sp.waves) { CHECK(nsb == 0, "solo blocks without solo waves"); continue; }
                    const uint32_t kmax = sp.forced >= 0 ? (uint32_t)sp.forced : std::min<uint32_t>(n / 4, 4u * sp.waves);
                    if (sp.forced >= 0) {
                        CHECK(nsb == (uint32_t)sp.forced, "forced %d: %u solo", sp.forced, nsb);
                        for (uint32_t j = 0; j < nsb; ++j)
                            CHECK(bins[j].size() == 1 && bins[j][0] == order[j], "forced: wave %u does not hold rank %u", j, j);
                    } else if (shared) {
                        const uint32_t top = std::min<uint32_t>(kmax + 1, n), r = std::min<uint32_t>(std::max<uint32_t>(1024u, top), n - 1);
                        const double ref = 1.3 * (double)wgt(blk[order[r]]);
                        for (uint32_t j = 0; j < bins.size(); ++j) {
                            CHECK(bins[j].size() <= 1, "shared: %zu blocks in a wave", bins[j].size());
                            if (!bins[j].empty()) CHECK(bins[j][0] == order[j] && (double)wgt(blk[order[j]]) > ref, "shared: wave %u holds a block that is no outlier", j);
                        }
                        if (nsb < std::min(kmax, sp.waves)) CHECK(!((double)wgt(blk[order[nsb]]) > ref), "shared: an outlier was left to the lanes");
                    } else {
                        // max(solo side, lane side) of k solo blocks, packed longest-first into the least loaded wave
                        auto cost = [&](uint32_t k) {
                            std::vector<uint64_t> load(sp.waves, 0);
                            std::vector<uint32_t> cnt(sp.waves, 0);
                            for (uint32_t j = 0; j < k; ++j) {
                                int best = -1;
                                for (uint32_t b = 0; b < sp.waves; ++b)
                                    if (cnt[b] < 64 && (best < 0 || load[b] < load[best])) best = (int)b;
                                if (best < 0) break;
                                load[best] += wgt(blk[order[j]]); ++cnt[best];
                            }
                            const double solo = (double)*std::max_element(load.begin(), load.end()) / sp.ratio;
                            return std::max(solo, k < n ? (double)wgt(blk[order[k]]) : 0.0);
                        };
                        CHECK(nsb <= kmax, "%u solo blocks above the limit %u", nsb, kmax);
                        if (nsb > 0) CHECK(cost(nsb - 1) >= cost(nsb), "packed: k - 1 = %u is better (%g < %g)", nsb - 1, cost(nsb - 1), cost(nsb));
                        if (nsb < kmax) CHECK(cost(nsb + 1) >= cost(nsb), "packed: k + 1 = %u is better (%g < %g)", nsb + 1, cost(nsb + 1), cost(nsb));
                    }
                }
}

// ---- 4. lane_layout
static void check_lanes(std::mt19937& rng) {
    for (uint32_t L : {64u, 16u, 1u})
        for (uint32_t n : {1u, 7u, 8u, 63u, 64u, 65u, 1000u})
            for (int variant = 0; variant < 3; ++variant) {
                const std::vector<GkBlock> blk = weights(variant, n, rng);
                GkSoloPlan sp{0, -1, 2.5f};
                if (variant == 1) { sp.forced = (int)std::min(5u, n); sp.waves = 12; }
                if (variant == 2) sp.waves = 24;
                std::vector<std::vector<uint32_t>> bins;
                const uint32_t nsb = solo_split(blk.data(), n, sp, false, bins);
                LaneTables T(bins, n, nsb, L);
                std::vector<uint64_t> buf(T.bytes() / 8 + 2, 0x5555555555555555ull);
                T.bind(buf.data());
                lane_layout(blk.data(), bins, L, T);
                CHECK(T.nsw % 12 == 0 && T.nslots == T.nw * 64 && T.nw >= T.nsw, "wave counts %u / %u / %u", T.nsw, T.nw, T.nslots);
                CHECK((nsb == 0) == (T.nsw == 0), "%u solo blocks in %u solo waves", nsb, T.nsw);
                uint32_t used = 0, last_np = 0xffffffffu, solo_seen = 0;
                for (uint32_t s = 0; s < T.nslots; ++s) {
                    const uint32_t q = T.ord[s], wv = s / 64, lane = s % 64;
                    if (q == 0xffffffffu) continue;
                    CHECK(q < n && T.pos[q] == s, "slot %u holds block %u whose slot is %u", s, q, q < n ? T.pos[q] : 0);
                    ++used;
                    if (wv < T.nsw) { ++solo_seen; continue; }
                    CHECK(lane < L, "a lane wave uses slot %u of %u lanes", lane, L);
                    CHECK(blk[q].npasses <= last_np, "lane blocks not in non-increasing pass order at slot %u", s);
                    last_np = blk[q].npasses;
                }
                CHECK(used == n && solo_seen == nsb, "%u of %u blocks placed, %u of %u solo", used, n, solo_seen, nsb);
                for (uint32_t q = 0; q < n; ++q) CHECK(T.ids[q] == q && T.ord[T.pos[q]] == q, "block %u not at its slot", q);
                uint64_t sum = 0;
                for (uint32_t wv = 0; wv < T.nw; ++wv) {
                    CHECK(T.wo[wv] == sum && T.wo[wv + 1] >= T.wo[wv], "wave %u scratch offset", wv);
                    uint32_t mp = 0, cnt = 0;
                    for (uint32_t i = wv * 64; i < wv * 64 + 64; ++i)
                        if (T.ord[i] != 0xffffffffu) { mp = std::max<uint32_t>(mp, blk[T.ord[i]].numbps); ++cnt; }
                    CHECK(wv < T.nsw || cnt, "an empty lane wave");
                    sum += cnt ? gk_t1dec_lane_words(mp) * 64 : 0;
                }
                CHECK(T.wo[T.nw] == sum, "scratch total %llu, slabs sum to %llu", (unsigned long long)T.wo[T.nw], (unsigned long long)sum);
            }
}

// ---- 5. output_rects against comp_dims
static void check_rects(const Plan& P) {
    const std::vector<TilePart> parts = parts_of(P, nullptr, -1);
    const uint32_t wins[][4] = {{0, 0, P.w, P.h}, {0, 0, 1, 1}, {P.w - 1, 0, P.w, 1}, {0, P.h - 1, 1, P.h}, {P.w - 1, P.h - 1, P.w, P.h},
                                {50, 35, 75, 50}};
    for (uint32_t red = 0; red < 3; ++red)
        for (int wi = -1; wi < (int)(sizeof wins / sizeof wins[0]); ++wi) {
            const uint32_t* win = wi < 0 ? nullptr : wins[wi];
            const TileRect TR = tile_rect(P, parts, win, false);
            const OutRects O = output_rects(P, TR.RG, win, red, win ? win[0] : 0, win ? win[1] : 0);
            bool empty = false;
            std::vector<uint32_t> w(P.nc), h(P.nc);
            for (uint32_t c = 0; c < P.nc; ++c) {
                comp_dims(P, P.sx(c), P.sy(c), red, win, w[c], h[c]);
                empty = empty || !w[c] || !h[c];
            }
            CHECK(O.win_empty == (win && empty), "reduce %u window %d: empty %d, comp_dims says %d", red, wi, O.win_empty, empty);
            if (empty) continue;
            for (uint32_t c = 0; c < P.nc; ++c) {
                const CompRect& r = O.c[c];
                const SGroup& G = P.groups[P.group_of[c]];
                CHECK(r.x1 - r.x0 == w[c] && r.y1 - r.y0 == h[c], "reduce %u window %d component %u: %u x %u, comp_dims %u x %u", red, wi, c,
                      r.x1 - r.x0, r.y1 - r.y0, w[c], h[c]);
                // inside the region's plane on the component's reduced grid, at or after the caller plane's origin
                const Region& Rg = TR.RGg[P.group_of[c]];
                const uint32_t px0 = ceildivpow2(Rg.x0 + G.ox, red) - r.rox, px1 = ceildivpow2(Rg.x0 + G.ox + Rg.w, red) - r.rox;
                const uint32_t py0 = ceildivpow2(Rg.y0 + G.oy, red) - r.roy, py1 = ceildivpow2(Rg.y0 + G.oy + Rg.h, red) - r.roy;
                CHECK(px0 <= r.x0 && r.x1 <= px1 && py0 <= r.y0 && r.y1 <= py1, "reduce %u window %d component %u outside the plane", red, wi, c);
                CHECK(r.wx0 <= r.x0 && r.wy0 <= r.y0, "reduce %u window %d component %u before the caller plane's origin", red, wi, c);
                if (win) CHECK(r.wx0 == r.x0 && r.wy0 == r.y0, "reduce %u window %d component %u: the window's origin is not the rectangle's", red, wi, c);
            }
        }
}

int main() {
    std::mt19937 rng(20);
    const uint32_t win[4] = {70, 60, 75, 66};   // inside tile (1, 1): most blocks of the tile are not needed
    const uint32_t win4[4] = {50, 35, 75, 50};  // straddles four tiles
    for (int irrev = 0; irrev < 2; ++irrev)
        for (int s = 0; s < 2; ++s) {
            const uint32_t sdx = 2, sdy = s ? 2 : 1;
            const Plan P16 = make_plan(irrev, sdx, sdy, true, 0), P1 = make_plan(irrev, sdx, sdy, false, 0);
            const Plan Pms = make_plan(irrev, sdx, sdy, true, GK_STY_LAZY | GK_STY_TERMALL);
            check_fill("16 tiles", P16, nullptr, -1, rng);
            check_fill("one tile", P1, nullptr, -1, rng);
            check_fill("BYPASS | TERMALL", Pms, nullptr, -1, rng);
            check_fill("BYPASS | TERMALL, window", Pms, win4, -1, rng);
            check_fill("window", P16, win, -1, rng);
            check_fill("window over four tiles", P16, win4, -1, rng);
            check_fill("window, one tile", P1, win, -1, rng);
            check_fill("a tile without a part", P16, nullptr, 5, rng);
            check_fill("16 tiles of 4 x 4 blocks", make_plan(irrev, sdx, sdy, true, 0, 2), nullptr, 3, rng, true);
            check_fill("one tile of 4 x 4 blocks", make_plan(irrev, sdx, sdy, false, 0, 2), win4, -1, rng, true);
            check_fill("BYPASS | TERMALL, 4 x 4 blocks", make_plan(irrev, sdx, sdy, true, GK_STY_LAZY | GK_STY_TERMALL, 2), nullptr, -1, rng, true);
            check_needed(P16, rng);
            check_needed(P1, rng);
            check_rects(P16);
            check_rects(P1);
        }
    {   // (no subsampling)
        const Plan P = make_plan(0, 1, 1, true, 0);
        check_fill("16 tiles, one grid", P, nullptr, -1, rng);
        check_needed(P, rng);
        check_rects(P);
    }
    check_solo(rng);
    check_lanes(rng);
    printf("decode stages ok\n");
    return 0;
}
