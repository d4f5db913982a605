// geom_rate.cpp -- host-only replay of one tile's two-layer rate allocation
// (t2.cpp rate_allocate, -r a,1) from the pass records the encoder computed
// for it: tests/golden/geom_rate_*.txt hold three tiles of the geometry sweep
// (tests/golden/manifest_geom.json geom_000 tile 14, geom_001 tile 6,
// geom_002 tile 2), 2 or 3 samples wide, whose first layer has
// j2k_update_rates' floor of 30 bytes.  Each has a band without samples in
// which the reference keeps a code-block without samples; its packet
// simulation counts a bit for it, and that bit decides the probe that lands on
// the budget (t2.cpp packet_header<SIM>).  Prints every block's layer records.
//
//   g++ -O2 -std=c++17 -I<csrc> geom_rate.cpp <csrc>/t2.cpp <csrc>/codestream.cpp -lpthread
//   ./a.out FILE
// FILE: numcomps x0 y0 x1 y1 prec numres log2(cblkw) log2(cblkh) irrev mct tdx
// tdy tx0 ty0 tw th prog tileno main-header-bytes ratio nblocks, then per
// code-block in for_each_cblk order: numbps numpasses and per pass its
// cumulative rate and cumulative distortion decrease (%la).
#include <float.h>
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include "t2.h"
using namespace grkgpu;
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "r");
    const bool slopes = argc > 2 ? atoi(argv[2]) != 0 : true;  // per-block slope extremes precomputed
    if (!f) return 2;
    CodingParams cp;
    uint32_t x0, y0, x1, y1, prec, tileno, hdr, nblk;
    double ratio;
    if (fscanf(f, "%u %u %u %u %u %u %u %u %u %d %d %u %u %u %u %u %u %u %u %u %lf %u", &cp.numcomps, &x0, &y0, &x1, &y1, &prec, &cp.numres,
           &cp.cblkw, &cp.cblkh, &cp.irrev, &cp.mct, &cp.tdx, &cp.tdy, &cp.tx0, &cp.ty0, &cp.tw, &cp.th, &cp.prog, &tileno, &hdr, &ratio, &nblk) != 22) return 2;
    cp.image = {x0, y0, x1, y1};
    for (uint32_t k = 0; k < cp.numcomps; ++k) { cp.prec[k] = prec; cp.shift[k] = 1 << (prec - 1); }
    cp.numlayers = 2;
    for (uint32_t r = 0; r < cp.numres; ++r) cp.prcw[r] = cp.prch[r] = 15;
    cp.disto_alloc = 1;
    generate_qcd(cp);
    Tile tile;
    tile.index = tileno;
    tile.r = tile_rect(cp, tileno);
    tile.comps.resize(cp.numcomps);
    for (uint32_t k = 0; k < cp.numcomps; ++k) build_tilecomp(tile.comps[k], tile.r, cp, k, true);
    std::vector<EncCblkState> cst;
    std::vector<EncPass> passes;
    double distotile = 0;
    uint32_t got = 0;
    for (auto &tc : tile.comps)
        for (auto &res : tc.res)
            for (uint32_t b = 0; b < res.numbands; ++b)
                for (auto &pr : res.bands[b].precs)
                    for (auto &c : pr.cblks) {
                        c.gidx = (uint32_t)cst.size();
                        EncCblkState s;
                        if (fscanf(f, "%u %u", &s.numbps, &s.numpasses) != 2) { printf("short of blocks at %u\n", got); return 3; }
                        ++got;
                        s.pass0 = (uint32_t)passes.size();
                        uint32_t prev = 0;
                        for (uint32_t k = 0; k < s.numpasses; ++k) {
                            EncPass p{};
                            if (fscanf(f, "%u %la", &p.rate, &p.dd) != 2) return 3;
                            p.len = p.rate - prev; prev = p.rate;
                            p.term = k + 1 == s.numpasses;
                            passes.push_back(p);
                        }
                        block_slopes(s, passes.data() + s.pass0);
                        if (s.numpasses) distotile += passes.back().dd;
                        cst.push_back(s);
                    }
    if (got != nblk) { printf("blocks %u of %u\n", got, nblk); return 3; }
    // tile_rates (codec.cpp), two layers, the last lossless
    const double npix = (double)tile.r.w() * tile.r.h();
    double r0 = ((double)cp.numcomps * prec * npix) / (ratio * 8.0);
    const double sot = npix * hdr / ((double)(x1 - x0) * (y1 - y0));
    r0 -= sot;
    if (r0 < 30.0f) r0 = 30.0f;
    uint64_t ts = 0;
    for (uint32_t k = 0; k < cp.numcomps; ++k) ts += (uint64_t)cp.tdx * cp.tdy * prec;
    ts = (uint64_t)((double)ts * 0.1625);
    ts += 12 + (uint64_t)(cp.numcomps - 1) * 11 * 2 + 4 + 9;
    if (ts < 256ull * cp.numcomps) ts = 256ull * cp.numcomps;
    const uint64_t bound = ts - 12 - 4;
    std::vector<EncLayer> layers((size_t)cst.size() * 2);
    TileEnc te;
    te.tile = &tile; te.cblk = &cst; te.passes = passes.data(); te.layers = &layers; te.slopes = slopes;
    init_enc_pocs(cp, te);
    te.distotile = distotile;
    CodingParams cpt = cp;
    cpt.rates[0] = r0; cpt.rates[1] = 0;
    RateStats rs;
    if (!rate_allocate(cpt, te, bound, &rs)) { printf("failed\n"); return 1; }
    printf("tile %u rect %u %u %u %u rate0 %.3f bound %llu probes %u skipped %u\n", tileno, tile.r.x0, tile.r.y0, tile.r.x1, tile.r.y1, r0,
           (unsigned long long)bound, rs.probes, rs.skipped);
    uint64_t l0 = 0;
    for (size_t i = 0; i < cst.size(); ++i) {
        printf("blk %zu passes %u: L0 %u passes %u bytes | L1 %u passes %u bytes\n", i, cst[i].numpasses, layers[2 * i].numpasses,
               layers[2 * i].numpasses ? layers[2 * i].len : 0, layers[2 * i + 1].numpasses, layers[2 * i + 1].numpasses ? layers[2 * i + 1].len : 0);
        if (layers[2 * i].numpasses) l0 += layers[2 * i].len;
    }
    printf("layer 0 body bytes %llu\n", (unsigned long long)l0);
    return 0;
}
