// Host-only check of the encode core's stages (gk_engine.cpp: enc_range, range_blocks,
// weight_order, cut_fractions / chunk_cuts, bisect_notch, chain_packets_serial /
// chain_packets_by_band, layout_packets / layout_packets_parallel, layout_segments) on small plans
// with generated T1 results (info words and pass records from a fixed seed, as tools/pcrd_bench.cpp
// makes them); every stream is read back through the engine's own reader (parse_header, the SOT
// walk, t2_parse_part).  No GPU call is made.
// Build: as tools/decode_stages_check.cpp (tests/test_encode_stages.py); run with no arguments.
// Exits non-zero with a message on the first failure.
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

// 200 x 150 at canvas origin (3, 5), 3 components (1 and 2 subsampled sd x sd), 3 resolutions;
// tiled: 64 x 48 tiles (16, partial at two edges), else one tile; cb 4: 16 x 16 code-blocks, 2: 4 x 4
struct Case {
    const char* name;
    uint32_t sd; bool tiled; uint32_t cb, sty, layers, prog, sop_eph; bool plt, tlm; char tp_div;
};
static Plan make_plan(const Case& k) {
    Plan P;
    P.w = 200; P.h = 150; P.x0 = 3; P.y0 = 5; P.nc = 3; P.prec = 8; P.sgnd = 0;
    P.cdx = {1, (uint8_t)k.sd, (uint8_t)k.sd}; P.cdy = {1, (uint8_t)k.sd, (uint8_t)k.sd};
    P.p.numres = 3; P.p.cbw = k.cb; P.p.cbh = k.cb; P.p.irrev = 0; P.p.mct = 0; P.p.cblk_sty = k.sty;
    P.p.nlayers = k.layers; P.p.prog = k.prog; P.p.sop_eph = k.sop_eph; P.p.plt = k.plt; P.p.tlm = k.tlm; P.p.tp_div = k.tp_div;
    if (k.tiled) { P.p.tw = 64; P.p.th = 48; }
    for (int i = 0; i < GK_MAXRLVLS; ++i) { P.p.prcw[i] = 15; P.p.prch[i] = 15; }
    build_plan(P);
    CHECK(P.tiles.size() == (k.tiled ? 16u : 1u), "%s: %zu tiles", k.name, P.tiles.size());
    return P;
}
// T1 results as a coder might leave them: numbps, npasses (0 included), bytes, pass offset (HT:
// one pass, info[3] the MagSgn bytes) and cumulative pass records
struct T1Synth { std::vector<uint32_t> info; std::vector<GkPass> passes; };
static T1Synth gen_t1(const Plan& P, std::mt19937& rng) {
    const uint32_t nb = (uint32_t)P.blocks.size();
    const bool ms = (P.p.cblk_sty & (GK_STY_LAZY | GK_STY_TERMALL)) != 0;
    T1Synth S;
    S.info.assign(4 * (size_t)nb + 16, 0);
    for (uint32_t b = 0; b < nb; ++b) {
        const uint32_t bnb = P.blocks[b].band_numbps;
        const uint32_t nbps = rng() % 6 == 0 ? 0 : std::min<uint32_t>(bnb, 1 + rng() % 6);
        const uint32_t np = !nbps ? 0 : P.p.ht() ? 1 : 3 * nbps - 2;
        S.info[4 * b] = nbps; S.info[4 * b + 1] = np; S.info[4 * b + 3] = (uint32_t)S.passes.size();
        uint32_t r = 0;
        double d = 0;
        for (uint32_t q = 0; q < np; ++q) {
            // (at most 16 passes of 5 bytes: within the smallest slot; a terminated pass has bytes)
            const uint32_t dr = !ms && rng() % 4 == 0 ? 0 : 1 + rng() % 5;
            r += dr; d += 1000.0 * dr;
            if (!P.p.ht()) S.passes.push_back({r, dr, d});
        }
        if (P.p.ht()) { r = np ? 2 + rng() % 40 : 0; S.info[4 * b + 3] = np ? rng() % (r - 1) : 0; }   // (a tail of at least 2 bytes)
        S.info[4 * b + 2] = r;
    }
    return S;
}

// ---- 1. enc_range and range_blocks against a direct recomputation
static void check_range(const Plan& P) {
    const uint32_t nt = (uint32_t)P.tiles.size(), nb = (uint32_t)P.blocks.size();
    for (uint32_t tb = 0; tb < nt; ++tb)
        for (uint32_t te = tb + 1; te <= nt; ++te) {
            const EncRange R = enc_range(P, tb, te);
            uint32_t b0 = nb, b1 = 0, y0 = ~0u, y1 = 0;
            for (uint32_t t = tb; t < te; ++t) {
                b0 = std::min(b0, P.tiles[t].b0); b1 = std::max(b1, P.tiles[t].b1);
                y0 = std::min(y0, P.tiles[t].y0 - P.y0); y1 = std::max(y1, P.tiles[t].y1 - P.y0);
            }
            CHECK(R.tb == tb && R.te == te && R.b0 == b0 && R.b1 == b1 && R.nbr == b1 - b0, "[%u, %u): blocks [%u, %u), expected [%u, %u)", tb, te, R.b0, R.b1, b0, b1);
            CHECK(R.ry0 == y0 && R.ry1 == y1 && R.RG.y0 == y0 && R.RG.h == y1 - y0 && R.RG.w == P.w, "[%u, %u): rows [%u, %u), expected [%u, %u)", tb, te, R.ry0, R.ry1, y0, y1);
            uint64_t span = 0;
            for (uint32_t b = b0; b < b1; ++b) span = std::max<uint64_t>(span, P.blocks[b].data_off + P.blocks[b].data_cap);
            CHECK(R.slot0 == P.blocks[b0].data_off && R.slot0 + R.slot_span >= span && R.slot0 + R.slot_span <= P.slot_bytes, "[%u, %u): slots", tb, te);
            if (b1 < nb) CHECK(R.slot0 + R.slot_span == P.blocks[b1].data_off, "[%u, %u): the slots end where the next tile's begin", tb, te);
            std::vector<GkBlock> hb(R.nbr + 1);
            std::vector<uint64_t> hso(R.nbr + 1);
            range_blocks(P, R, nullptr, hb.data(), hso.data());
            for (uint32_t i = 0; i < R.nbr; ++i) {
                const GkBlock& G = hb[i];
                const uint64_t lo = 2 * (uint64_t)G.comp * R.RG.plane, hi = lo + 2 * (uint64_t)R.RG.plane;
                CHECK(G.stride == R.RG.stride && G.band_off >= lo && G.band_off + (uint64_t)(G.h - 1) * G.stride + G.w <= hi,
                      "[%u, %u): block %u of component %u at %llu outside its work planes [%llu, %llu)", tb, te, R.b0 + i, G.comp,
                      (unsigned long long)G.band_off, (unsigned long long)lo, (unsigned long long)hi);
                CHECK(G.data_off + G.data_cap <= R.slot_span, "[%u, %u): block %u's slot outside the range's", tb, te, R.b0 + i);
            }
            CHECK(hso[0] == 0 && hso[R.nbr] == P.sym_off[b1] - P.sym_off[b0], "[%u, %u): symbol offsets", tb, te);
        }
}

// ---- 2, 3. weight_order and chunk_cuts
static void check_order_and_cuts(std::mt19937& rng) {
    for (uint32_t n : {1u, 255u, 8192u, 8193u, 49152u}) {
        std::vector<uint32_t> w(n), ord(n, ~0u), seen(n, 0);
        uint32_t wmax = 1;
        for (uint32_t& v : w) { v = rng() % 3 == 0 ? rng() % 7 : rng() % 100000; wmax = std::max(wmax, v); }
        weight_order(w.data(), n, ord.data());
        auto key = [&](uint32_t i) { return 4095 - (uint32_t)(((uint64_t)w[i] * 4095) / wmax); };
        for (uint32_t j = 0; j < n; ++j) {
            CHECK(ord[j] < n && !seen[ord[j]]++, "weight_order(%u): entry %u is no permutation", n, j);
            if (!j) continue;
            CHECK(key(ord[j - 1]) <= key(ord[j]), "weight_order(%u): bucket keys decrease at %u", n, j);
            CHECK(key(ord[j - 1]) != key(ord[j]) || ord[j - 1] < ord[j], "weight_order(%u): not index order within a bucket at %u", n, j);
        }
        for (const char* list : {"0.125,0.375", "0.08,0.25", "0.5", "0.9,0.1,x,2"}) {
            const std::vector<double> fr = cut_fractions(list);
            CHECK(fr.size() <= 3, "cut_fractions(%s): %zu fractions", list, fr.size());
            for (double f : fr) CHECK(f > 0 && f < 1, "cut_fractions(%s): %g", list, f);
            const std::vector<uint32_t> cut = chunk_cuts(n, fr);
            CHECK(cut.size() >= 2 && cut.size() <= 5 && cut.front() == 0 && cut.back() == n, "chunk_cuts(%u, %s): ends", n, list);
            for (size_t k = 1; k < cut.size(); ++k) {
                CHECK(cut[k] > cut[k - 1], "chunk_cuts(%u, %s): not increasing at %zu", n, list, k);
                if (k + 1 < cut.size()) CHECK(cut[k] % 256 == 0, "chunk_cuts(%u, %s): cut %u is no multiple of 256", n, list, cut[k]);
            }
        }
    }
    const std::vector<uint32_t> c0 = chunk_cuts(8192, cut_fractions("0.125,0.375")), c1 = chunk_cuts(8192, cut_fractions("0.08,0.25"));
    CHECK(c0 == (std::vector<uint32_t>{0, 1024, 3072, 8192}) && c1 == (std::vector<uint32_t>{0, 512, 2048, 8192}), "the default cuts of 8,192 blocks");
}

// ---- 4. bisect_notch on monotone and non-monotone length tables
static void check_bisect(std::mt19937& rng) {
    for (uint32_t prec : {8u, 12u, 16u}) {
        const uint32_t top = 8 * (prec - 1);
        uint32_t maxp = 0;
        while ((1u << maxp) < top + 2) ++maxp;   // ceil(log2(top + 2))
        for (int it = 0; it < 400; ++it) {
            std::vector<uint64_t> len(top + 1);
            uint64_t v = 1000000;
            for (uint32_t n = 0; n <= top; ++n) {
                len[n] = v;
                v = it % 2 ? v - std::min<uint64_t>(v, rng() % 30000) : (v * (90 + rng() % 15)) / 100;   // monotone / not
            }
            const uint64_t target = it % 7 == 0 ? 0 : it % 7 == 1 ? ~0ull : rng() % 1100000;
            uint32_t probes = 0, lastp = ~0u;
            const NotchSearch s = bisect_notch(top, target, [&](uint32_t n) { ++probes; lastp = n; return len[n]; });
            CHECK(s.hi == s.lo + 1 && s.lo >= -1 && s.hi <= (int64_t)top + 1, "prec %u: [%lld, %lld] is no adjacent pair", prec, (long long)s.lo, (long long)s.hi);
            CHECK(s.lo < 0 || len[s.lo] > target, "prec %u: lo %lld does not overshoot", prec, (long long)s.lo);
            CHECK(s.hi > (int64_t)top || len[s.hi] <= target, "prec %u: hi %lld does not fit", prec, (long long)s.hi);
            CHECK(probes <= maxp && probes >= 1, "prec %u: %u probes, at most %u", prec, probes, maxp);
            CHECK(s.last == (int64_t)lastp, "prec %u: last probe %u reported as %lld", prec, lastp, (long long)s.last);
            if (s.lo >= 0) CHECK(s.over == len[s.lo], "prec %u: the coarsest overshooting estimate", prec);
        }
    }
}

// ---- 5, 6. the chain builders against each other, the layout arms against each other
static bool same(const ChainOut& a, const ChainOut& b) {
    return a.phdr == b.phdr && a.bsegs == b.bsegs && a.pk.size() == b.pk.size() &&
           (a.pk.empty() || !memcmp(a.pk.data(), b.pk.data(), a.pk.size() * sizeof(Pk)));
}
static void check_t2(const Case& k, std::mt19937& rng) {
    const Plan P = make_plan(k);
    const uint32_t nt = (uint32_t)P.tiles.size();
    const T1Synth S = gen_t1(P, rng);
    const T1Out F{const_cast<uint32_t*>(S.info.data()), P.p.ht() ? nullptr : S.passes.data(), (uint32_t)S.passes.size()};
    const EncRange R = enc_range(P, 0, 0);
    T2Enc T2(P, F.hinfo, F.hpasses, 0, nt);
    const std::vector<T2Enc::Swallow> tsw = allocate_layers(P, T2, F, 0, nt, 200);
    CHECK(tsw.size() == nt, "%s: %zu swallow records", k.name, tsw.size());
    if (nt == 1) {
        const std::vector<PkChain> chains = tile_chains(P, P.tiles[0]);
        const std::vector<ChainOut> a = chain_packets_serial(T2, P.tiles[0], chains), b = chain_packets_by_band(T2, P.tiles[0], chains);
        CHECK(a.size() == chains.size() && b.size() == chains.size(), "%s: chain counts", k.name);
        for (size_t q = 0; q < chains.size(); ++q) CHECK(same(a[q], b[q]), "%s: chain %zu differs between the serial and the by-band builder", k.name, q);
    }
    const TilePartSplit TPS = tile_part_split(P);
    std::vector<TileOut> tout(nt);
    for (uint32_t t = 0; t < nt; ++t) build_tile_packets(P, T2, t, tsw[t], TPS, nt == 1, tout[t]);
    if (!P.p.ht() && nt == 1) {   // the two arms over every tile part of the tile
        EncLayout A, B;
        A.slot_span = B.slot_span = R.slot_span;
        for (uint32_t part = 0; part < TPS.n; ++part) {
            layout_packets(A, P, R, F.hinfo, tout[0], tout[0].pk_first[part], tout[0].pk_first[part + 1]);
            layout_packets_parallel(B, P, R, tout[0], tout[0].pk_first[part], tout[0].pk_first[part + 1]);
        }
        CHECK(A.seg == B.seg && A.hdrs == B.hdrs && A.pos == B.pos, "%s: the serial and the per-packet parallel layout differ", k.name);
    }
    std::vector<uint8_t> H;
    const std::vector<uint8_t> J;   // (a raw codestream: the reader below starts at SOC)
    size_t tlm_pos = 0;
    write_main_header(H, P, &tlm_pos);
    EncReq req;
    const EncLayout Y = layout_segments(P, R, F.hinfo, tout, TPS.n, J, H, tlm_pos, req, nullptr);
    // the destination ranges tile [0, total); every source lies in a block's slot or in the host bytes
    std::vector<std::pair<uint64_t, uint32_t>> slots;   // (slot start, block)
    for (uint32_t b = R.b0; b < R.b1; ++b) slots.push_back({P.blocks[b].data_off - R.slot0, b});
    uint64_t at = 0;
    for (size_t i = 0; i < Y.seg.size(); i += 3) {
        const uint64_t so = Y.seg[i], n = Y.seg[i + 2];
        CHECK(Y.seg[i + 1] == at && n > 0, "%s: segment %zu starts at %llu, the stream is at %llu", k.name, i / 3, (unsigned long long)Y.seg[i + 1], (unsigned long long)at);
        at += n;
        if (so >= R.slot_span) { CHECK(so + n <= R.slot_span + Y.hdrs.size(), "%s: segment %zu past the host bytes", k.name, i / 3); continue; }
        auto it = std::upper_bound(slots.begin(), slots.end(), std::make_pair(so, ~0u));
        CHECK(it != slots.begin(), "%s: segment %zu before the first slot", k.name, i / 3);
        const uint32_t b = (--it)->second;
        const GkBlock& G = P.blocks[b];
        CHECK(so + n <= it->first + G.data_cap, "%s: segment %zu leaves block %u's slot", k.name, i / 3, b);
        if (P.p.ht()) {   // the head or the tail of the slot
            const uint32_t head = F.hinfo[4 * (size_t)b + 3], len = F.hinfo[4 * (size_t)b + 2];
            CHECK((so == it->first && n == head) || (so + n == it->first + G.data_cap && n == len - head), "%s: HT block %u: neither head nor tail", k.name, b);
        }
    }
    CHECK(at == Y.pos, "%s: the segments end at %llu, the stream at %llu", k.name, (unsigned long long)at, (unsigned long long)Y.pos);

    // ---- 7. the stream, resolved from a random byte arena, through the engine's own reader
    std::vector<uint8_t> arena(R.slot_span + Y.hdrs.size()), cs(Y.pos);
    for (uint8_t& v : arena) v = (uint8_t)rng();
    memcpy(arena.data() + R.slot_span, Y.hdrs.data(), Y.hdrs.size());
    for (size_t i = 0; i < Y.seg.size(); i += 3) memcpy(cs.data() + Y.seg[i + 1], arena.data() + Y.seg[i], Y.seg[i + 2]);
    ByteSrc BS;
    BS.host = cs.data(); BS.len = cs.size();
    Header Hd;
    parse_header(BS, Hd);   // (a host source: the tile parts come from the SOT walk)
    CHECK(Hd.first_sot == H.size() && Hd.parts.size() == (size_t)nt * TPS.n, "%s: first SOT at %zu of %zu, %zu tile parts of %u", k.name, Hd.first_sot, H.size(), Hd.parts.size(), nt * TPS.n);
    uint64_t psum = 0;
    for (const TilePart& TP : Hd.parts) psum += TP.end - TP.sot;
    CHECK(psum == cs.size() - H.size() - 2 && cs[cs.size() - 2] == 0xff && cs[cs.size() - 1] == 0xd9, "%s: Psot sums to %llu of %zu bytes between the main header and EOC", k.name, (unsigned long long)psum, cs.size() - H.size() - 2);
    if (P.p.tlm) {
        CHECK(Hd.tlm.size() == Hd.parts.size(), "%s: %zu TLM entries for %zu tile parts", k.name, Hd.tlm.size(), Hd.parts.size());
        for (size_t q = 0; q < Hd.parts.size(); ++q)
            CHECK(Hd.tlm[q].first == Hd.parts[q].tile && Hd.tlm[q].second == Hd.parts[q].end - Hd.parts[q].sot, "%s: TLM entry %zu is not its tile part's Psot", k.name, q);
    }
    std::vector<std::vector<uint32_t>> plt(nt);
    if (P.p.plt) {   // the PLT markers of the tile-part headers, read here (the SOT walk of a host source skips them):
                     // Zplt, then 7-bit groups MSB first, bit 7 = continuation
        for (const TilePart& TP : Hd.parts)
            for (size_t j = TP.sot + 12; j + 4 <= TP.data - 2; j += 2 + ((size_t)cs[j + 2] << 8 | cs[j + 3])) {
                if (cs[j] != 0xff || cs[j + 1] != 0x58) continue;
                uint32_t v = 0;
                for (size_t q = j + 5; q < j + 2 + ((size_t)cs[j + 2] << 8 | cs[j + 3]); ++q) {
                    v = (v << 7) | (cs[q] & 0x7fu);
                    if (!(cs[q] & 0x80)) { plt[TP.tile].push_back(v); v = 0; }
                }
            }
        for (uint32_t t = 0; t < nt; ++t) {
            CHECK(plt[t].size() == tout[t].pk.size(), "%s: tile %u: %zu PLT lengths for %zu packets", k.name, t, plt[t].size(), tout[t].pk.size());
            for (size_t q = 0; q < plt[t].size(); ++q) CHECK(plt[t][q] == tout[t].pk[q].len, "%s: tile %u packet %zu: PLT %u, length %u", k.name, t, q, plt[t][q], tout[t].pk[q].len);
        }
    }
    merge_tile_parts(Hd);
    CHECK(Hd.parts.size() == nt, "%s: %zu tiles after the merge", k.name, Hd.parts.size());
    const uint32_t L = P.p.nlayers;
    for (const TilePart& TP : Hd.parts) {
        const TileG& T = P.tiles[TP.tile];
        const std::vector<uint8_t> need(T.b1 - T.b0, 1);
        PartState st;
        t2_parse_part(P, TP, need, 0, 0, BS, st);
        if (P.p.plt) {
            // the PLT lengths against what the reader found: laid end to end over the tile parts' packet
            // bytes they end each part exactly, every body chunk lies inside one packet, and a packet
            // that has bodies ends with its last one
            std::vector<std::pair<size_t, size_t>> rg(1, {TP.data, TP.end});
            rg.insert(rg.end(), TP.more.begin(), TP.more.end());
            std::vector<size_t> pend;   // each packet's end in the stream
            size_t ri = 0, cur = rg[0].first;
            for (uint32_t len : plt[TP.tile]) {
                cur += len;
                CHECK(ri < rg.size() && cur <= rg[ri].second, "%s: tile %u: the PLT lengths leave tile part %zu", k.name, TP.tile, ri);
                pend.push_back(cur);
                if (cur == rg[ri].second && ++ri < rg.size()) cur = rg[ri].first;
            }
            CHECK(ri == rg.size(), "%s: tile %u: the PLT lengths end in tile part %zu of %zu", k.name, TP.tile, ri, rg.size());
            size_t pk = 0, last_end = 0;
            for (const Chunk& c : st.chunks) {
                while (pk < pend.size() && pend[pk] <= c.pos) {
                    CHECK(!last_end || last_end == pend[pk], "%s: tile %u packet %zu: its bodies end at %zu, its PLT length at %zu", k.name, TP.tile, pk, last_end, pend[pk]);
                    ++pk; last_end = 0;
                }
                CHECK(pk < pend.size() && c.pos + c.len <= pend[pk], "%s: tile %u: a body chunk at %llu crosses the end of packet %zu", k.name, TP.tile, (unsigned long long)c.pos, pk);
                last_end = c.pos + c.len;
            }
            CHECK(!last_end || last_end == pend[pk], "%s: tile %u: the last packet with bodies ends at %zu, its PLT length at %zu", k.name, TP.tile, last_end, pend[pk]);
        }
        for (uint32_t b = T.b0; b < T.b1; ++b) {
            uint32_t tot = 0;
            for (uint32_t l = 0; l < L; ++l) tot += T2.lnp[(size_t)b * L + l];
            const uint32_t lb = b - T.b0, len = tot ? T2.rate(b, tot - 1) : 0;
            CHECK(tot == F.hinfo[4 * (size_t)b + 1], "%s: block %u: %u of %u passes in layers", k.name, b, tot, F.hinfo[4 * (size_t)b + 1]);
            CHECK((st.included[lb] != 0) == (tot != 0) && st.npasses[lb] == tot && st.len[lb] == len,
                  "%s: block %u read back as included %u, %u passes, %u bytes; written %u passes, %u bytes", k.name, b, st.included[lb], st.npasses[lb], st.len[lb], tot, len);
            if (tot) CHECK(st.numbps[lb] == F.hinfo[4 * (size_t)b], "%s: block %u: %u bit-planes read, %u coded", k.name, b, st.numbps[lb], F.hinfo[4 * (size_t)b]);
            if (P.p.cblk_sty & (GK_STY_LAZY | GK_STY_TERMALL)) {
                uint32_t sum = 0;
                for (uint32_t v : st.seglens[lb]) sum += v;
                CHECK(sum == len, "%s: block %u: segment lengths sum to %u of %u bytes", k.name, b, sum, len);
            }
        }
    }
}

int main() {
    std::mt19937 rng(20);
    check_range(make_plan({"16 tiles", 1, true, 4, 0, 1, 0, 0, false, false, 0}));
    check_range(make_plan({"16 tiles, chroma 2 x 2", 2, true, 4, 0, 1, 0, 0, false, false, 0}));
    check_order_and_cuts(rng);
    check_bisect(rng);
    for (uint32_t sd : {1u, 2u})
        for (int tiled = 0; tiled < 2; ++tiled)
            for (uint32_t cb : {4u, 2u})
                for (uint32_t sty : {0u, (uint32_t)(GK_STY_LAZY | GK_STY_TERMALL), (uint32_t)GK_STY_HT}) {
                    const bool t = tiled != 0;
                    check_t2({"plain", sd, t, cb, sty, 1, 0, 0, false, false, 0}, rng);
                    check_t2({"three layers, RPCL", sd, t, cb, sty, 3, 2, 0, false, false, 0}, rng);
                    check_t2({"SOP + EPH, PLT, TLM", sd, t, cb, sty, 1, 0, 6, true, true, 0}, rng);
                    check_t2({"three layers, markers, tile parts by resolution", sd, t, cb, sty, 3, 0, 6, true, true, 'R'}, rng);
                    check_t2({"RPCL, tile parts by resolution", sd, t, cb, sty, 1, 2, 0, false, true, 'R'}, rng);
                }
    printf("encode stages ok\n");
    return 0;
}
