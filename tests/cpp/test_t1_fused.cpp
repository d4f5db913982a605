// Host-side check of the T1 decoder's column step (t1_dec.h d3_column: one
// step per sample, the zero-coding or run decision and the sign decision of
// the sample it makes significant in the same step) -- the device code of
// t1_dec.h / t1_flat.h compiled for the host, against the C oracle's decode.
//
//   block sizes  64x64, 1x64, 64x1, 3x5, 4x4, 33x7 (w x h): stripes of fewer
//                than four rows, one-column stripes
//   content      every sample significant in one plane, alternating and random
//                signs (cleanup columns of 4 ZC + 4 SC); a seed in the top
//                plane and every other sample in one low plane (the same in a
//                significance propagation pass -- a raw one under BYPASS);
//                isolated single samples (AGG, UNI, UNI, SC); empty blocks;
//                uniform noise
//   styles       0, VSC, BYPASS, RESET, TERMALL, SEGSYM, and all six switches
//
// Style 0: the oracle's own bytes through the single-segment entry
// (t1_decode_v5).  Every style, 0 included: the block coded with the style by
// the host build of the encoder, split into codeword segments, each unstuffed
// into its own region and decoded over the segment cursor (k_t1_decode_ub's
// codestream path).  Mode switches change the bytes, never the fully decoded
// coefficients, so both must equal, sample for sample, the oracle's decode of
// the oracle's cblksty == 0 encode of the block.
// The walk hooks count each column's decisions by context, and the run fails
// unless the columns the step was rewritten for did occur.
// Buffers are sized as the GPU path sizes them; tests/test_t1_fused_host.py
// builds this program a second time under AddressSanitizer + UBSan.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

// one column's decisions by kind, flushed at the next column / stripe / pass
static uint32_t g_zc, g_sc, g_agg, g_uni, g_pass, g_incol;
static uint32_t seen_44[3], seen_run, seen_run_after, seen_cols;
static void col_flush() {
    if (g_incol) {
        seen_cols++;
        if (g_zc == 4 && g_sc == 4) seen_44[g_pass]++;
        if (g_agg == 1 && g_uni == 2 && g_sc >= 1) seen_run++;
        if (g_agg == 1 && g_uni == 2 && g_zc >= 1) seen_run_after++;
    }
    g_zc = g_sc = g_agg = g_uni = g_incol = 0;
}
#define T1_WALK(e, val) (col_flush(), (e) == 0 ? (void)(g_pass = (val)) : (e) == 2 ? (void)(g_incol = 1) : (void)0)
#define T1_TRACE(cx, bit, a, c) ((cx) < 9 ? g_zc++ : (cx) < 14 ? g_sc++ : (cx) == 17 ? g_agg++ : (cx) == 18 ? g_uni++ : 0u)

#include "../../grokimagecompression_amd/csrc/t1_flat.h"
#include "../../oracle/grk_oracle.h"

using namespace grkgpu;
static const uint32_t kTab[47] = GRK_MQ_TABLE_INIT;
static uint32_t kDecTab[MQ_DEC_WORDS];

static uint64_t rng = 0xD1B54A32D192ED03ull;
static uint32_t rnd() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (uint32_t)rng; }

static T1Scratch scr;

// grk_device.h t1_unstuff_region_words: header {nwords, ncarry, -, -}, words, carries
static uint32_t region_words(uint32_t len) { return 4 + unstuff_word_cap(len) + unstuff_carry_cap(len); }

struct Seg { uint32_t off, len, npasses; };

// a segment ends at every terminated pass (t1_pass_term) and at the last pass
static std::vector<Seg> split_segments(uint32_t sty, uint32_t numbps, uint32_t np, const uint32_t *rate) {
    std::vector<Seg> segs;
    uint32_t start = 0, first = 0;
    for (uint32_t k = 0; k < np; ++k) {
        int32_t bp; int pt;
        pass_info(k, numbps, &bp, &pt);
        if (t1_pass_term(sty, bp, pt, numbps) || k + 1 == np) {
            segs.push_back({start, rate[k] - start, k + 1 - first});
            start = rate[k];
            first = k + 1;
        }
    }
    return segs;
}

enum { C_ALT, C_RND, C_SPP, C_SINGLE, C_EMPTY, C_NOISE, NUM_CONTENT };
static const char *kContent[] = {"alt", "rnd", "spp", "single", "empty", "noise"};

static std::vector<int32_t> make_block(int content, uint32_t w, uint32_t h) {
    std::vector<int32_t> c(w * h, 0);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            int32_t v = 0;
            switch (content) {
            case C_ALT: v = ((x + y) & 1) ? -512 : 512; break;                                 // one plane, alternating signs
            case C_RND: v = (int32_t)(512 + rnd() % 512) * ((rnd() & 1) ? -1 : 1); break;       // one plane, random signs
            case C_SPP: v = (int32_t)(8 + rnd() % 8) * ((rnd() & 1) ? -1 : 1); break;           // plane 3, found by its SPP
            case C_NOISE: v = (int32_t)(rnd() % 2047) - 1023; break;
            default: break;
            }
            c[y * w + x] = v;
        }
    if (content == C_SPP) c[0] = (rnd() & 1) ? -1024 : 1024;  // the seed the propagation starts from
    if (content == C_SINGLE)  // no two in each other's neighbourhood: every one is found by a run
        for (uint32_t y = rnd() % std::min(3u, h); y < h; y += 3 + rnd() % 4)
            for (uint32_t x = rnd() % std::min(3u, w); x < w; x += 3 + rnd() % 6)
                c[y * w + x] = (int32_t)(1 + rnd() % 1023) * ((rnd() & 1) ? -1 : 1);
    return c;
}

int main() {
    int fails = 0, blocks = 0, decodes = 0, empties = 0;
    for (uint32_t i = 0; i < MQ_DEC_WORDS; ++i) kDecTab[i] = mq_dec_table_entry(kTab, i);
    static uint8_t zc[2048], sc[256], scw[256];
    for (uint32_t i = 0; i < 2048; ++i) zc[i] = zc_lut_entry(i >> 9, i & 511);
    for (uint32_t i = 0; i < 256; ++i) sc[i] = sc_lut_entry(i);
    for (uint32_t i = 0; i < 256; ++i) scw[i] = sc_win_entry(i);
    static const uint32_t SHAPES[][2] = {{64, 64}, {1, 64}, {64, 1}, {3, 5}, {4, 4}, {33, 7}};
    static const uint32_t STYLES[] = {0, CBLKSTY_VSC, CBLKSTY_LAZY, CBLKSTY_RESET, CBLKSTY_TERMALL, CBLKSTY_SEGSYM, 63};
    for (const auto &shape : SHAPES)
        for (int content = 0; content < NUM_CONTENT; ++content)
            for (int rep = 0; rep < 4; ++rep) {
                const uint32_t w = shape[0], h = shape[1], orient = (uint32_t)rep;
                const std::vector<int32_t> coef = make_block(content, w, h);
                ++blocks;
                // the reference: the oracle's decode of its own cblksty == 0 encode
                std::vector<uint8_t> obuf(w * h * 8 + 64, 0);
                orc_pass op[100];
                uint32_t onb = 0, olen = 0;
                const int onp = orc_t1_encode_cblk(coef.data(), w, w, h, orient, 1, 0, obuf.data() + 1,
                                                   (uint32_t)obuf.size() - 1, op, &onb, &olen);
                if ((content == C_EMPTY) != (onp == 0)) {
                    printf("PASSES %s w=%u h=%u: %d passes\n", kContent[content], w, h, onp);
                    fails++;
                }
                std::vector<int32_t> od(w * h, 0);
                if (onp > 0) {
                    std::vector<uint8_t> data(obuf.begin() + 1, obuf.begin() + 1 + olen);
                    data.push_back(0); data.push_back(0);
                    orc_t1_decode_cblk(data.data(), olen, (uint32_t)onp, onb, w, h, orient, od.data());
                }
                const DecTables DT{zc + orient * 512, scw, kDecTab};
                auto dirty = [&] {  // the kernel clears the state rows itself, never the bit-plane rows
                    std::fill(scr.pa, scr.pa + 32 * 64, ~0ull);
                    std::fill(scr.pb, scr.pb + 32 * 64, ~0ull);
                    for (int i = 0; i < 66; ++i) scr.st.sig[i] = scr.st.neg[i] = scr.st.vis[i] = scr.st.ref[i] = ~0ull;
                };
                auto check = [&](const char *what, uint32_t sty, uint32_t np, uint32_t nb) {
                    col_flush();
                    const DecodedPlanes dp = decoded_planes(np, nb);
                    for (uint32_t y = 0; y < h; ++y)
                        for (uint32_t x = 0; x < w; ++x) {
                            const int32_t got = t1_rebuild(x, y, dp, scr.pa, scr.pb, scr.st.neg[y + 1]);
                            if (got != od[y * w + x]) {
                                printf("DEC MISMATCH %s %s sty=%u w=%u h=%u orient=%u first (x,y)=(%u,%u) %d/%d\n", what,
                                       kContent[content], sty, w, h, orient, x, y, got, od[y * w + x]);
                                fails++;
                                return;
                            }
                        }
                    ++decodes;
                };
                if (onp > 0) {  // style 0, the oracle's bytes, the single-segment entry
                    std::vector<uint32_t> words(unstuff_word_cap(olen) + 8, 0), carr(unstuff_carry_cap(olen), 0);
                    uint32_t *wp = (uint32_t *)(((uintptr_t)words.data() + 15) & ~(uintptr_t)15);
                    uint32_t ncar = 0, cxw[32], ring[FB_RING];
                    const uint32_t nw = t1_unstuff(obuf.data() + 1, olen, wp, carr.data(), &ncar);
                    dirty();
                    t1_decode_v5(wp, nw, carr.data(), (uint32_t)onp, onb, w, h, scr.st, DT, cxw, scr.pa, scr.pb, ring, 0);
                    check("v5", 0, (uint32_t)onp, onb);
                }
                for (const uint32_t sty : STYLES) {
                    // encode with the style: prep, per-plane context modelling, the MQ / raw coder
                    const uint32_t lnb = t1_prep_serial(coef.data(), w, w, h, 1, 0, scr.st, scr.pa);
                    t1_prep_above(h, lnb, scr.pa, scr.pb);
                    const uint32_t slot = sym_slot_bytes(w, h);
                    std::vector<uint32_t> sym(((size_t)lnb * slot + 256) / 4, 0);
                    uint64_t tmp[128];
                    for (uint32_t p = 0; p < lnb; ++p) {
                        uint32_t *base = sym.data() + (size_t)p * slot / 4;
                        const uint64_t *ref = p + 1 < lnb ? scr.pb + (p + 1) * 64 : scr.pb;
                        t1_model_plane<const uint64_t *, uint64_t *>(w, h, orient, scr.pa + p * 64, scr.pb + p * 64, ref,
                                                                     p + 1 < lnb, scr.st.neg, tmp, sc, base, scr.cnt + p * 4,
                                                                     sty, t1_pass_raw(sty, (int32_t)p, 0, lnb));
                    }
                    const uint32_t slab = t1_enc_slab_bytes(w, h, sty, lnb);
                    const size_t obytes = ((size_t)slab + 15) & ~(size_t)15;
                    std::vector<uint32_t> sbuf((16 + obytes) / 4, 0);
                    uint32_t *sout = sbuf.data() + 4;
                    uint32_t srate[100], slen = 0, cx[32];
                    const uint32_t snp = (sty & CBLKSTY_LAZY)
                                             ? t1_mq_block<true>(lnb, sym.data(), slot / 4, scr.cnt, kTab, cx, sout, srate, &slen, sty)
                                             : t1_mq_block<false>(lnb, sym.data(), slot / 4, scr.cnt, kTab, cx, sout, srate, &slen, sty);
                    if (lnb != onb || (int)snp != onp || slen > slab) {
                        printf("ENCODE %s sty=%u w=%u h=%u np %u/%d nb %u/%u len %u slab %u\n", kContent[content], sty, w, h,
                               snp, onp, lnb, onb, slen, slab);
                        fails++;
                        continue;
                    }
                    if (onp == 0) { empties++; continue; }  // no pass: the kernel leaves the block alone
                    const uint8_t *bytes = (const uint8_t *)sout;
                    const std::vector<Seg> segs = split_segments(sty, lnb, snp, srate);
                    std::vector<std::vector<uint8_t>> sdata;
                    std::vector<DecSeg> ds(segs.size());
                    uint64_t uwords = 0;
                    for (size_t q = 0; q < segs.size(); ++q) {
                        sdata.emplace_back(bytes + segs[q].off, bytes + segs[q].off + segs[q].len);
                        ds[q] = DecSeg{0, segs[q].len, segs[q].npasses, (uint32_t)(uwords / 4), 0};
                        uwords += region_words(segs[q].len);
                    }
                    const size_t ubytes = uwords * 4 + 256;
                    uint32_t *ubuf = (uint32_t *)aligned_alloc(16, ubytes);
                    memset(ubuf, 0xA5, ubytes);
                    for (size_t q = 0; q < segs.size(); ++q) {
                        uint32_t *region = ubuf + (size_t)ds[q].ub_off * 4;
                        uint32_t *words = region + 4, *carries = words + unstuff_word_cap(ds[q].len);
                        uint32_t nc = 0;
                        region[0] = t1_unstuff(sdata[q].data(), ds[q].len, words, carries, &nc);
                        region[1] = nc;
                    }
                    dirty();
                    uint32_t cxw[32], ring[FB_RING];
                    auto run = [&](auto &d) {
                        const uint32_t *region = ubuf + (size_t)ds[0].ub_off * 4;
                        for (uint32_t y = 0; y < h + 2; ++y) { scr.st.sig[y] = 0; scr.st.neg[y] = 0; scr.st.vis[y] = 0; scr.st.ref[y] = 0; }
                        mq_reset_words_dec(cxw, DT.mq);
                        d.set_ring(ring, 0);
                        d.init(region + 4, region[0], region + 4 + unstuff_word_cap(ds[0].len));
                        SegCursor cur{ds.data(), ubuf, (uint32_t)ds.size(), 0, ds[0].npasses};
                        t1_decode_passes(d, snp, lnb, w, h, scr.st, DT, cxw, scr.pa, scr.pb, sty, cur, 0u);
                    };
                    if (sty & CBLKSTY_LAZY) { BitDecT<true> d; run(d); }
                    else { BitDecT<false> d; run(d); }
                    check("segments", sty, snp, lnb);
                    free(ubuf);
                }
            }
    // the columns the step was rewritten for: 4 ZC + 4 SC in a significance
    // propagation and in a cleanup pass, a run (AGG, UNI, UNI, SC) that ends
    // the column and one followed by plain ZC rows
    if (!seen_44[0] || !seen_44[2] || !seen_run || !seen_run_after || !empties) {
        printf("COVERAGE columns %u: 4 ZC + 4 SC in SPP %u, in cleanup %u; runs %u, runs with ZC rows after %u; empty %d\n", seen_cols,
               seen_44[0], seen_44[2], seen_run, seen_run_after, empties);
        fails++;
    }
    printf("%s: %d failures / %d blocks, %d decodes (columns of 4 ZC + 4 SC: SPP %u, cleanup %u; run columns %u)\n",
           fails ? "FAIL" : "OK", fails, blocks, decodes, seen_44[0], seen_44[2], seen_run);
    return fails ? 1 : 0;
}
