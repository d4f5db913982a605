// Host-side check of the encoder's context modelling (t1_lane.h
// t1_model_plane, the code of k_t1_model compiled for the host) against a
// plain per-sample modeller of one bit-plane written here: the stripe /
// column / row scan of ISO 15444-1 D.3 with per-sample neighbour lookups, no
// row masks, no bit slices, no packing.  For every block and plane the symbol
// bytes (context | decision << 5) and the three pass counts must be equal.
// Shapes: widths {1..5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64} x heights
// {1, 3, 4, 5, 8, 61, 63, 64} x four orientations; contents: dense noise of 1
// to 16 planes, sparse, all zero, a single nonzero sample (corners, columns
// 7/8, 15/16, 31/32, 63), full magnitude (every refinement column has all
// four rows), alternating-sign checkerboards; styles 0, VSC, SEGSYM,
// VSC|SEGSYM, BYPASS (raw SPP signs).  Every plane's symbol slot is an
// allocation of exactly sym_slot_bytes(w, h), so the AddressSanitizer build
// (tests/test_t1_model_host.py) reports a write past it.
//   test_t1_model [stride]   every stride-th (w, h) pair (default 1: all)
//   test_t1_model --encode IN OUT STY   the whole block encoder, file to file
//   test_t1_model --sweep [rule]        the MQ slab rule against the encoder's len
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../grokimagecompression_amd/csrc/t1_flat.h"

using namespace grkgpu;

static uint64_t rng = 0x243F6A8885A308D3ull;
static uint32_t rnd() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (uint32_t)rng; }

static uint32_t seen_sc[5][2], seen_full_mrp, seen_agg[3], seen_raw;

struct Plain {
    int w, h;
    uint32_t orient;
    bool vsc;
    std::vector<uint8_t> sig, vis, neg;
    bool S(int x, int y) const { return x >= 0 && y >= 0 && x < w && y < h && sig[y * w + x]; }
    bool N(int x, int y) const { return S(x, y) && neg[y * w + x]; }
    // the row below a stripe's last row is out of sight under VSC
    bool below(int y) const { return !(vsc && (y & 3) == 3); }
    bool nbr(int x, int y) const {
        return S(x - 1, y) || S(x + 1, y) || S(x - 1, y - 1) || S(x, y - 1) || S(x + 1, y - 1) ||
               (below(y) && (S(x - 1, y + 1) || S(x, y + 1) || S(x + 1, y + 1)));
    }
    uint32_t zc(int x, int y) const {
        const bool b = below(y);
        const int hh = S(x - 1, y) + S(x + 1, y), vv = S(x, y - 1) + (b && S(x, y + 1));
        const int dd = S(x - 1, y - 1) + S(x + 1, y - 1) + (b && S(x - 1, y + 1)) + (b && S(x + 1, y + 1));
        return (uint32_t)zc_ctx(hh, vv, dd, orient);
    }
    uint32_t sc(int x, int y, bool raw) const {
        const bool b = below(y);
        uint32_t xr;
        const int cx = sc_ctx(S(x - 1, y), S(x + 1, y), S(x, y - 1), b && S(x, y + 1), N(x - 1, y), N(x + 1, y),
                              N(x, y - 1), b && N(x, y + 1), &xr);
        seen_sc[cx - CX_SC][xr]++;
        const uint32_t ng = neg[y * w + x];
        return (uint32_t)cx | ((raw ? ng : ng ^ xr) << 5);
    }
};

// plane p of magnitudes mag (sign in neg): the symbol bytes and the counts
static void plain_plane(int w, int h, uint32_t orient, const std::vector<uint32_t> &mag, const std::vector<uint8_t> &neg,
                        uint32_t p, uint32_t sty, bool raw_spp, std::vector<uint8_t> &out, uint32_t *cnt) {
    Plain s{w, h, orient, (sty & CBLKSTY_VSC) != 0, {}, {}, neg};
    s.sig.assign(w * h, 0);
    s.vis.assign(w * h, 0);
    std::vector<uint8_t> before(w * h);
    for (int i = 0; i < w * h; ++i) before[i] = s.sig[i] = (mag[i] >> (p + 1)) != 0;
    auto bit = [&](int x, int y) { return (mag[y * w + x] >> p) & 1u; };
    out.clear();
    for (int k = 0; k < h; k += 4)
        for (int x = 0; x < w; ++x)
            for (int y = k; y < k + 4 && y < h; ++y) {
                if (s.sig[y * w + x] || !s.nbr(x, y)) continue;
                out.push_back((uint8_t)(s.zc(x, y) | bit(x, y) << 5));
                s.vis[y * w + x] = 1;
                if (bit(x, y)) {
                    out.push_back((uint8_t)s.sc(x, y, raw_spp));
                    seen_raw += raw_spp;
                    s.sig[y * w + x] = 1;
                }
            }
    cnt[0] = (uint32_t)out.size();
    for (int k = 0; k < h; k += 4)
        for (int x = 0; x < w; ++x) {
            int members = 0;
            for (int y = k; y < k + 4 && y < h; ++y) {
                if (!before[y * w + x]) continue;
                ++members;
                const uint32_t cx = (mag[y * w + x] >> (p + 2)) ? CX_MAG + 2 : (s.nbr(x, y) ? CX_MAG + 1 : CX_MAG);
                out.push_back((uint8_t)(cx | bit(x, y) << 5));
            }
            seen_full_mrp += members == 4;
        }
    cnt[1] = (uint32_t)out.size() - cnt[0];
    for (int k = 0; k < h; k += 4)
        for (int x = 0; x < w; ++x) {
            int y0 = k;
            bool run_row = false;
            if (k + 3 < h) {
                bool agg = true;
                for (int y = k; y < k + 4; ++y) agg = agg && !s.sig[y * w + x] && !s.vis[y * w + x] && !s.nbr(x, y);
                if (agg) {
                    int run = 0;
                    while (run < 4 && !bit(x, k + run)) ++run;
                    seen_agg[run == 4 ? 0 : run == 0 ? 1 : 2]++;
                    if (run == 4) {
                        out.push_back(CX_AGG);
                        continue;
                    }
                    out.push_back(CX_AGG | 1u << 5);
                    out.push_back((uint8_t)(CX_UNI | (uint32_t)(run >> 1) << 5));
                    out.push_back((uint8_t)(CX_UNI | (uint32_t)(run & 1) << 5));
                    y0 = k + run;
                    run_row = true;
                }
            }
            for (int y = y0; y < k + 4 && y < h; ++y) {
                if (s.sig[y * w + x] || s.vis[y * w + x]) continue;
                if (!(run_row && y == y0)) out.push_back((uint8_t)(s.zc(x, y) | bit(x, y) << 5));
                if (bit(x, y)) {
                    out.push_back((uint8_t)s.sc(x, y, false));
                    s.sig[y * w + x] = 1;
                }
            }
        }
    if (sty & CBLKSTY_SEGSYM) {
        out.push_back(CX_UNI | 1u << 5);
        out.push_back(CX_UNI);
        out.push_back(CX_UNI | 1u << 5);
        out.push_back(CX_UNI);
    }
    cnt[2] = (uint32_t)out.size() - cnt[0] - cnt[1];
}

// --encode IN OUT STY: the host build of the whole block encoder (prep,
// t1_model_plane per plane, t1_mq_block) with code-block style STY, for
// tests/test_gpu_t1_model.py -- the reference of a style the oracle's block
// encoder does not have.  IN: u32 n, then per block u32 w, h, orient, qmfbid,
// i32 inv_step, i32 coef[w * h]; OUT: per block u32 numbps, numpasses, len,
// rate[96], then len bytes.
static const uint32_t kTab[47] = GRK_MQ_TABLE_INIT;
static T1Scratch scr;

// --sweep [rule]: t1_enc_slab_bytes against the host encoder's len on the
// blocks where the terminations, not the samples, decide the size: every
// style 0..63 x the shapes below x depths 1..26 x five contents, 5/3 and 9/7
// (inv_step 6553).  Each block goes through t1_prep_serial from coefficients
// where a coefficient of that depth exists (5/3: up to 25 planes, 9/7 at this
// step: up to 19; a magnitude of more bits is no int32 coefficient), and the
// 26-plane blocks from the rows the prep would leave (pa / pb / neg written
// directly).  Any len above the rule is reported with its case and fails the
// run; the largest len / rule per style is printed.  Without `rule` the
// output buffer is far larger than any block's bytes, so the check does not
// depend on what lies after a slab; with it every block's buffer is an
// allocation of exactly the 16 bytes of headroom plus the rule rounded up to
// 4, for the AddressSanitizer build (tests/test_t1_slab_host.py).
static uint64_t srng = 0xD1B54A32D192ED03ull;
static uint32_t srnd() { srng ^= srng << 13; srng ^= srng >> 7; srng ^= srng << 17; return (uint32_t)srng; }

static const int kSweepShapes[][2] = {{1, 1}, {1, 2}, {2, 1}, {1, 3}, {3, 1}, {2, 2}, {1, 4}, {4, 1}, {3, 3}, {4, 4},
                                      {5, 3}, {1, 8}, {2, 8}, {1, 16}, {16, 1}, {1, 64}, {64, 1}, {4, 64}, {64, 64}};  // (h, w)
static const char *const kSweepKinds[] = {"full", "random", "alt5555", "single", "staircase"};

// magnitudes of exactly nb bits (in some sample) and signs
static void sweep_content(int kind, uint32_t n, uint32_t nb, std::vector<uint32_t> &mag, std::vector<uint8_t> &neg) {
    const uint32_t top = 1u << (nb - 1), all = (uint32_t)(((uint64_t)1 << nb) - 1);
    mag.assign(n, 0);
    neg.assign(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
        if (kind == 0) mag[i] = all;
        if (kind == 1) { mag[i] = top | (srnd() & all); neg[i] = srnd() & 1; }
        if (kind == 2) { mag[i] = top | (0x55555555u & all); neg[i] = 1; }
        if (kind == 4) mag[i] = top >> (i % nb);  // one more sample turns significant at every plane
    }
    if (kind == 3) mag[n / 2] = all;
}

static int sweep(bool rule_sized) {
    int fails = 0;
    uint64_t blocks = 0, past_area = 0;  // past_area: blocks longer than w * h * 4 + 64
    double worst[64];
    uint32_t wcase[64][5];
    for (int s = 0; s < 64; ++s) worst[s] = 0;
    std::vector<uint32_t> mag;
    std::vector<uint8_t> neg;
    std::vector<uint32_t> sym;
    std::vector<uint32_t> big((16 + 64 * 64 * 16 + 65536) / 4);
    for (size_t si = 0; si < sizeof kSweepShapes / sizeof kSweepShapes[0]; ++si) {
        const uint32_t h = (uint32_t)kSweepShapes[si][0], w = (uint32_t)kSweepShapes[si][1];
        for (uint32_t nb = 1; nb <= T1_MAX_ENC_BPS; ++nb)
            for (int kind = 0; kind < 5; ++kind)
                for (int qmfbid = 1; qmfbid >= 0; --qmfbid) {
                    const uint32_t orient = (uint32_t)(si + kind) % 4;
                    sweep_content(kind, w * h, nb, mag, neg);
                    uint32_t lnb = nb;
                    if (qmfbid == 0 && nb > 19) continue;  // no such int32 coefficient at this step
                    if (qmfbid == 1 && nb > 25) {
                        // the rows t1_prep_serial leaves for these magnitudes
                        memset(&scr.st, 0, sizeof scr.st);
                        for (uint32_t p = 0; p < nb; ++p)
                            for (uint32_t y = 0; y < h; ++y) {
                                uint64_t row = 0;
                                for (uint32_t x = 0; x < w; ++x) row |= (uint64_t)((mag[y * w + x] >> p) & 1u) << x;
                                scr.pa[p * 64 + y] = row;
                            }
                        for (uint32_t i = 0; i < w * h; ++i)
                            if (neg[i]) scr.st.neg[i / w + 1] |= (uint64_t)1 << (i % w);
                    } else {
                        std::vector<int32_t> coef(w * h);
                        for (uint32_t i = 0; i < w * h; ++i) {
                            // 9/7: the coefficient whose quantised magnitude (6 fraction bits) is mag.100000b or just under it
                            const int64_t v = qmfbid ? (int64_t)mag[i] : mag[i] ? ((((int64_t)mag[i] << 6) | 32) << 18) / 6553 : 0;
                            coef[i] = (int32_t)(neg[i] ? -v : v);
                        }
                        lnb = t1_prep_serial(coef.data(), w, w, h, qmfbid, 6553, scr.st, scr.pa);
                    }
                    if (lnb != nb) {
                        printf("DEPTH h=%u w=%u nb=%u kind=%s qmfbid=%d: numbps %u\n", h, w, nb, kSweepKinds[kind], qmfbid, lnb);
                        return 1;
                    }
                    t1_prep_above(h, nb, scr.pa, scr.pb);
                    const uint32_t slot = sym_slot_bytes(w, h);
                    sym.assign(((size_t)nb * slot + 256) / 4, 0);
                    // the symbols depend on BYPASS, VSC and SEGSYM only: modelled once for the
                    // eight styles that differ in RESET, TERMALL and PTERM
                    for (uint32_t mv = 0; mv < 8; ++mv) {
                        const uint32_t msty = (mv & 1 ? CBLKSTY_LAZY : 0) | (mv & 2 ? CBLKSTY_VSC : 0) | (mv & 4 ? CBLKSTY_SEGSYM : 0);
                        uint64_t tmp[128];
                        for (uint32_t p = 0; p < nb; ++p) {
                            const uint64_t *ref = p + 1 < nb ? scr.pb + (p + 1) * 64 : scr.pb;
                            t1_model_plane<const uint64_t *, uint64_t *>(w, h, orient, scr.pa + p * 64, scr.pb + p * 64, ref,
                                                                         p + 1 < nb, scr.st.neg, tmp, nullptr,
                                                                         sym.data() + (size_t)p * slot / 4, scr.cnt + p * 4, msty,
                                                                         t1_pass_raw(msty, (int32_t)p, 0, nb));
                        }
                        for (uint32_t cv = 0; cv < 8; ++cv) {
                            const uint32_t sty = msty | (cv & 1 ? CBLKSTY_RESET : 0) | (cv & 2 ? CBLKSTY_TERMALL : 0) |
                                                 (cv & 4 ? CBLKSTY_PTERM : 0);
                            const uint32_t rule = t1_enc_slab_bytes(w, h, sty, nb);
                            uint32_t *buf = rule_sized ? (uint32_t *)malloc(16 + ((rule + 3) & ~3u)) : big.data();
                            uint32_t rate[96], cx[32], slen = 0;
                            if (sty & CBLKSTY_LAZY) t1_mq_block<true>(nb, sym.data(), slot / 4, scr.cnt, kTab, cx, buf + 4, rate, &slen, sty);
                            else t1_mq_block<false>(nb, sym.data(), slot / 4, scr.cnt, kTab, cx, buf + 4, rate, &slen, sty);
                            if (rule_sized) free(buf);
                            ++blocks;
                            past_area += slen > w * h * 4 + 64;
                            if (slen > rule) {
                                if (fails < 40)
                                    printf("OVER sty=%u h=%u w=%u nb=%u kind=%s %s len=%u rule=%u\n", sty, h, w, nb, kSweepKinds[kind],
                                           qmfbid ? "5/3" : "9/7", slen, rule);
                                ++fails;
                            }
                            const double q = (double)slen / rule;
                            if (q > worst[sty]) {
                                worst[sty] = q;
                                const uint32_t c[5] = {h, w, nb, slen, rule};
                                memcpy(wcase[sty], c, sizeof c);
                            }
                        }
                    }
                }
    }
    for (int s = 0; s < 64; ++s)
        printf("MAX sty=%d len/rule=%.3f (%ux%u, %u planes: %u of %u)\n", s, worst[s], wcase[s][0], wcase[s][1], wcase[s][2],
               wcase[s][3], wcase[s][4]);
    printf("blocks past w*h*4+64: %llu\n", (unsigned long long)past_area);
    printf("%s: %d over the rule / %llu blocks\n", fails ? "FAIL" : "OK", fails, (unsigned long long)blocks);
    return fails ? 1 : 0;
}

static int encode_file(const char *in, const char *outp, uint32_t sty) {
    FILE *fi = fopen(in, "rb"), *fo = fopen(outp, "wb");
    uint32_t n = 0;
    if (!fi || !fo || fread(&n, 4, 1, fi) != 1) return 2;
    for (uint32_t b = 0; b < n; ++b) {
        uint32_t hd[5];
        if (fread(hd, 4, 5, fi) != 5) return 2;
        const uint32_t w = hd[0], h = hd[1], orient = hd[2];
        std::vector<int32_t> coef(w * h);
        if (fread(coef.data(), 4, w * h, fi) != w * h) return 2;
        const uint32_t lnb = t1_prep_serial(coef.data(), w, w, h, (int)hd[3], (int32_t)hd[4], scr.st, scr.pa);
        t1_prep_above(h, lnb, scr.pa, scr.pb);
        const uint32_t slot = sym_slot_bytes(w, h);
        std::vector<uint32_t> sym(((size_t)lnb * slot + 256) / 4, 0);
        uint64_t tmp[128];
        for (uint32_t p = 0; p < lnb; ++p) {
            const uint64_t *ref = p + 1 < lnb ? scr.pb + (p + 1) * 64 : scr.pb;
            t1_model_plane<const uint64_t *, uint64_t *>(w, h, orient, scr.pa + p * 64, scr.pb + p * 64, ref, p + 1 < lnb,
                                                         scr.st.neg, tmp, nullptr, sym.data() + (size_t)p * slot / 4,
                                                         scr.cnt + p * 4, sty, t1_pass_raw(sty, (int32_t)p, 0, lnb));
        }
        const size_t obytes = ((size_t)t1_enc_slab_bytes(w, h, sty, lnb) + 15) & ~(size_t)15;
        std::vector<uint32_t> sbuf((16 + obytes) / 4, 0);
        uint32_t rec[3 + 96] = {0}, cx[32], slen = 0;
        rec[0] = lnb;
        rec[1] = (sty & CBLKSTY_LAZY)
                     ? t1_mq_block<true>(lnb, sym.data(), slot / 4, scr.cnt, kTab, cx, sbuf.data() + 4, rec + 3, &slen, sty)
                     : t1_mq_block<false>(lnb, sym.data(), slot / 4, scr.cnt, kTab, cx, sbuf.data() + 4, rec + 3, &slen, sty);
        rec[2] = slen;
        fwrite(rec, 4, 3 + 96, fo);
        fwrite(sbuf.data() + 4, 1, slen, fo);
    }
    fclose(fi);
    return fclose(fo) ? 2 : 0;
}

int main(int argc, char **argv) {
    if (argc == 5 && !strcmp(argv[1], "--encode")) return encode_file(argv[2], argv[3], (uint32_t)atoi(argv[4]));
    if (argc >= 2 && !strcmp(argv[1], "--sweep")) return sweep(argc > 2 && !strcmp(argv[2], "rule"));
    const int stride = argc > 1 ? atoi(argv[1]) : 1;
    static const int W[] = {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64};
    static const int H[] = {1, 3, 4, 5, 8, 61, 63, 64};
    static const uint32_t STY[] = {0, CBLKSTY_VSC, CBLKSTY_SEGSYM, CBLKSTY_VSC | CBLKSTY_SEGSYM, CBLKSTY_LAZY};
    static const int SX[] = {0, -1, 0, -1, 7, 8, 15, 16, 31, 32, 63};  // -1: the last column
    static const int SY[] = {0, 0, -1, -1, 1, 2, 3, 0, 1, 2, 3};       // -1: the last row
    static uint32_t ctab[512];
    for (uint32_t i = 0; i < 256; ++i) compact_sel(i, &ctab[2 * i], &ctab[2 * i + 1]);
    int fails = 0, blocks = 0, planes = 0, pair = 0;
    uint32_t it = 0;
    for (int w : W)
        for (int h : H) {
            if (pair++ % stride) continue;
            for (int kind = 0; kind < 6; ++kind)
                for (uint32_t orient = 0; orient < 4; ++orient, ++it) {
                    const uint32_t sty = STY[it % 5];
                    uint32_t nb = 1 + it % 16;
                    std::vector<uint32_t> mag(w * h, 0);
                    std::vector<uint8_t> neg(w * h, 0);
                    for (int i = 0; i < w * h; ++i) {
                        const int x = i % w, y = i / w;
                        neg[i] = rnd() & 1;
                        if (kind == 0) mag[i] = rnd() & ((1u << nb) - 1);
                        if (kind == 1) mag[i] = (rnd() % 8) ? 0 : rnd() & ((1u << nb) - 1);
                        if (kind == 4) mag[i] = (1u << nb) - 1;
                        if (kind == 5) {  // checkerboards, column and row stripes of sign
                            mag[i] = (it & 4) ? rnd() & ((1u << nb) - 1) : (1u << nb) - 1 - (rnd() & 1);
                            neg[i] = (orient == 0 ? x + y : orient == 1 ? x : orient == 2 ? y : x + y / 2) & 1;
                        }
                    }
                    if (kind == 3) {
                        const uint32_t q = (it / 4) % 11;
                        int x = SX[q] < 0 ? w - 1 : SX[q], y = SY[q] < 0 ? h - 1 : SY[q];
                        if (x >= w) x = w - 1;
                        if (y >= h) y = h - 1;
                        mag[y * w + x] = 1u << (nb - 1) | (rnd() & ((1u << nb) - 1));
                    }
                    uint32_t orv = 0;
                    for (uint32_t m : mag) orv |= m;
                    nb = 0;
                    while (orv >> nb) ++nb;
                    ++blocks;
                    // the rows k_t1_prep leaves: the plane's bits, the significance
                    // before it, the signs at index y + 1
                    std::vector<uint64_t> bits(nb * 64 + 64, 0), above((nb + 1) * 64 + 64, 0), negr(72, 0);
                    for (int y = 0; y < h; ++y)
                        for (int x = 0; x < w; ++x) {
                            const uint32_t m = mag[y * w + x];
                            if (m && neg[y * w + x]) negr[y + 1] |= 1ull << x;
                            for (uint32_t p = 0; p < nb; ++p) {
                                if ((m >> p) & 1) bits[p * 64 + y] |= 1ull << x;
                                if (m >> (p + 1)) above[p * 64 + y] |= 1ull << x;
                            }
                        }
                    const uint32_t slot = sym_slot_bytes((uint32_t)w, (uint32_t)h);
                    for (uint32_t p = 0; p < nb; ++p, ++planes) {
                        const bool raw = t1_pass_raw(sty, (int32_t)p, 0, nb);
                        std::vector<uint8_t> want;
                        uint32_t wc[3], gc[4] = {0, 0, 0, 0};
                        plain_plane(w, h, orient, mag, neg, p, sty, raw, want, wc);
                        uint32_t *sym = (uint32_t *)malloc(slot);  // exactly the slot
                        uint64_t tmp[128];
                        const uint64_t *ref = above.data() + (p + 1) * 64;
                        t1_model_plane<const uint64_t *, uint64_t *>((uint32_t)w, (uint32_t)h, orient, bits.data() + p * 64,
                                                                     above.data() + p * 64, ref, p + 1 < nb, negr.data(), tmp,
                                                                     nullptr, sym, gc, sty, raw, nullptr,
                                                                     (it & 1) ? ctab : nullptr);
                        const bool okc = gc[0] == wc[0] && gc[1] == wc[1] && gc[2] == wc[2];
                        if (want.size() > slot || !okc || memcmp(sym, want.data(), want.size())) {
                            size_t bad = 0;
                            while (bad < want.size() && bad < slot && ((uint8_t *)sym)[bad] == want[bad]) ++bad;
                            if (fails < 20)
                                printf("MISMATCH w=%d h=%d orient=%u kind=%d sty=%u nb=%u p=%u cnt %u %u %u / %u %u %u first byte %zu "
                                       "%02x/%02x slot %u\n", w, h, orient, kind, sty, nb, p, gc[0], gc[1], gc[2], wc[0], wc[1], wc[2],
                                       bad, bad < slot ? ((uint8_t *)sym)[bad] : 0, bad < want.size() ? want[bad] : 0, slot);
                            ++fails;
                        }
                        free(sym);
                    }
                }
        }
    if (stride == 1) {
        // the draw covers what it is meant to: every sign context with both
        // prediction bits (context 9 has no prediction), all-member refinement
        // columns, the three kinds of aggregation column, raw signs
        bool cov = seen_sc[0][0] && seen_full_mrp && seen_agg[0] && seen_agg[1] && seen_agg[2] && seen_raw;
        for (int c = 1; c < 5; ++c) cov = cov && seen_sc[c][0] && seen_sc[c][1];
        if (!cov) {
            printf("COVERAGE sc %u | %u %u | %u %u | %u %u | %u %u mrp4 %u agg %u %u %u raw %u\n", seen_sc[0][0], seen_sc[1][0],
                   seen_sc[1][1], seen_sc[2][0], seen_sc[2][1], seen_sc[3][0], seen_sc[3][1], seen_sc[4][0], seen_sc[4][1],
                   seen_full_mrp, seen_agg[0], seen_agg[1], seen_agg[2], seen_raw);
            ++fails;
        }
    }
    printf("%s: %d failures / %d blocks (%d planes)\n", fails ? "FAIL" : "OK", fails, blocks, planes);
    return fails ? 1 : 0;
}
