// t1_walk_fused_sim.cpp -- host analysis of the T1 decoder's column step (not
// a test; scripts/t1_walk_fused_sim.py drives it), beside t1_walk_sim.cpp.
// Codes each block with the C oracle's T1 encoder, decodes it with the GPU
// decoder's walk compiled for the host while the T1_WALK / T1_TRACE hooks
// count, per column, all decisions and those that are not sign decisions,
// then replays wavefronts of 64 consecutive blocks under the nested walk
// (passes, stripes and column steps in lock step; a column step lasts as long
// as its slowest lane's column) with two column loops:
//   symbol   one loop iteration per MQ decision (a column: 1..9 iterations)
//   sample   one iteration per sample or run symbol, the sign decision in the
//            iteration of the decision that leads to it (d3_column as built)
// Output, per pass type: decisions, wave steps of both loops, column steps.
//
// input (stdin, binary little-endian): n, then per block: w, h, orient,
// qmfbid, inv_step (int32 each) and w*h int32 coefficients.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

struct Ev {
    uint8_t kind;  // 0 pass, 1 stripe, 2 column
    uint16_t v;
    uint32_t nsym, nsign;  // decisions after this event until the next one; the sign decisions among them
};
static std::vector<Ev> *g_ev;
#define T1_WALK(e, val) g_ev->push_back(Ev{(uint8_t)(e), (uint16_t)(val), 0, 0})
#define T1_TRACE(cx, bit, a, c) (g_ev->back().nsym++, g_ev->back().nsign += ((cx) >= 9 && (cx) < 14))

#include "../../grokimagecompression_amd/csrc/t1_flat.h"
#include "../../oracle/grk_oracle.h"

using namespace grkgpu;
static const uint32_t kTab[47] = GRK_MQ_TABLE_INIT;
static uint32_t kDecTab[MQ_DEC_WORDS];
static T1Scratch scr;

struct Col { uint32_t n, nf; };  // decisions; decisions that are not sign decisions
struct Stripe_ { std::vector<Col> cols; uint32_t lead; };
struct Pass_ { uint32_t type; std::vector<Stripe_> stripes; };
struct Blk { std::vector<Pass_> passes; };

int main() {
    uint32_t n;
    if (fread(&n, 4, 1, stdin) != 1) return 1;
    for (uint32_t i = 0; i < MQ_DEC_WORDS; ++i) kDecTab[i] = mq_dec_table_entry(kTab, i);
    static uint8_t zc[2048], scw[256];
    for (uint32_t i = 0; i < 2048; ++i) zc[i] = zc_lut_entry(i >> 9, i & 511);
    for (uint32_t i = 0; i < 256; ++i) scw[i] = sc_win_entry(i);
    std::vector<Blk> blks;
    std::vector<Ev> ev;
    g_ev = &ev;
    for (uint32_t b = 0; b < n; ++b) {
        int32_t hdr[5];
        if (fread(hdr, 4, 5, stdin) != 5) return 2;
        const uint32_t w = hdr[0], h = hdr[1], orient = hdr[2];
        std::vector<int32_t> coef((size_t)w * h);
        if (fread(coef.data(), 4, coef.size(), stdin) != coef.size()) return 3;
        std::vector<uint8_t> obuf(w * h * 8 + 64, 0);
        orc_pass op[100];
        uint32_t onb = 0, olen = 0;
        const int onp = orc_t1_encode_cblk(coef.data(), w, w, h, orient, hdr[3], hdr[4], obuf.data() + 1,
                                           (uint32_t)obuf.size() - 1, op, &onb, &olen);
        Blk bk;
        if (onp > 0) {
            std::vector<uint32_t> words(unstuff_word_cap(olen) + 16, 0), carr(unstuff_carry_cap(olen) + 4, 0);
            uint32_t *wp = (uint32_t *)(((uintptr_t)words.data() + 15) & ~(uintptr_t)15);
            uint32_t ncar = 0;
            const uint32_t nw = t1_unstuff(obuf.data() + 1, olen, wp, carr.data(), &ncar);
            const DecTables DT{zc + orient * 512, scw, kDecTab};
            uint32_t cx4[32], ring[FB_RING];
            ev.clear();
            ev.push_back(Ev{9, 0, 0, 0});
            t1_decode_v5(wp, nw, carr.data(), (uint32_t)onp, onb, w, h, scr.st, DT, cx4, scr.pa, scr.pb, ring, 0);
            for (const Ev &e : ev) {
                if (e.kind == 0) bk.passes.push_back(Pass_{e.v, {}});
                else if (e.kind == 1) bk.passes.back().stripes.push_back(Stripe_{{}, e.nsym});
                else if (e.kind == 2) bk.passes.back().stripes.back().cols.push_back(Col{e.nsym, e.nsym - e.nsign});
            }
        }
        blks.push_back(std::move(bk));
    }
    uint64_t dec[3] = {}, sign[3] = {}, st_symbol[3] = {}, st_sample[3] = {}, colsteps[3] = {};
    for (auto &bk : blks)
        for (auto &ps : bk.passes)
            for (auto &sp : ps.stripes) {
                dec[ps.type] += sp.lead;
                for (const Col &c : sp.cols) { dec[ps.type] += c.n; sign[ps.type] += c.n - c.nf; }
            }
    for (size_t w0 = 0; w0 < blks.size(); w0 += 64) {
        const size_t w1 = std::min(blks.size(), w0 + 64);
        size_t maxp = 0;
        for (size_t i = w0; i < w1; ++i) maxp = std::max(maxp, blks[i].passes.size());
        for (size_t p = 0; p < maxp; ++p) {
            size_t maxs = 0;
            uint32_t t = 0;
            for (size_t i = w1; i-- > w0;)
                if (p < blks[i].passes.size()) { maxs = std::max(maxs, blks[i].passes[p].stripes.size()); t = blks[i].passes[p].type; }
            for (size_t k = 0; k < maxs; ++k) {
                size_t maxc = 0;
                uint32_t maxlead = 0;
                for (size_t i = w0; i < w1; ++i) {
                    if (p >= blks[i].passes.size() || k >= blks[i].passes[p].stripes.size()) continue;
                    const Stripe_ &s = blks[i].passes[p].stripes[k];
                    maxc = std::max(maxc, s.cols.size());
                    maxlead = std::max(maxlead, s.lead);
                }
                colsteps[t] += maxc;
                st_symbol[t] += maxlead;
                st_sample[t] += maxlead;
                for (size_t j = 0; j < maxc; ++j) {
                    uint32_t m = 0, mf = 0;
                    for (size_t i = w0; i < w1; ++i) {
                        if (p >= blks[i].passes.size() || k >= blks[i].passes[p].stripes.size()) continue;
                        const Stripe_ &s = blks[i].passes[p].stripes[k];
                        if (j < s.cols.size()) { m = std::max(m, s.cols[j].n); mf = std::max(mf, s.cols[j].nf); }
                    }
                    st_symbol[t] += m;
                    st_sample[t] += mf;
                }
            }
        }
    }
    printf("{\"blocks\": %zu, \"passes\": [", blks.size());
    for (int t = 0; t < 3; ++t)
        printf("%s{\"type\": %d, \"decisions\": %llu, \"sign_decisions\": %llu, \"ideal_steps\": %llu, \"symbol_steps\": %llu, "
               "\"sample_steps\": %llu, \"column_steps\": %llu}", t ? ", " : "", t, (unsigned long long)dec[t],
               (unsigned long long)sign[t], (unsigned long long)(dec[t] / 64), (unsigned long long)st_symbol[t],
               (unsigned long long)st_sample[t], (unsigned long long)colsteps[t]);
    printf("]}\n");
    return 0;
}
