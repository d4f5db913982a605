// Host-side check of the T1 coders' code-block mode switches (cblksty 1..63:
// BYPASS, RESET, TERMALL, VSC, PTERM, SEGSYM in every combination) -- the
// device code of t1_lane.h / t1_dec.h / t1_flat.h compiled for the host, block
// by block: encode with the style (k_t1_model + k_t1_mq), split the bytes
// into codeword segments, unstuff each into its own region (k_t1_unstuff) and
// decode over a segment cursor (k_t1_decode_ub's codestream path).  Mode
// switches change the bytes, never the fully decoded coefficients, so the
// result must equal the oracle's decode of its own cblksty == 0 encode of the
// block, for all passes and for a truncated pass count cut at the same pass.
// One exception, by the standard itself: VSC takes the row below a stripe out
// of the significance neighbourhood, so a sample may be coded by the cleanup
// pass instead of the significance propagation pass of its plane -- a stream
// cut inside a bit-plane then holds other samples than the style-0 stream cut
// at that pass.  For VSC styles the truncated reference is therefore
// plain_truncated() below, a per-sample restatement of which pass codes which
// sample, formed from the oracle's full decode; with the VSC rule off it must
// reproduce the oracle's truncated decode, and that is checked for every
// block of every style.
// At fixed iterations the blocks are 1x1, 1x2, 2x1 and 2x2 of 17 or more
// planes under TERMALL without PTERM or BYPASS: dozens of segments of a byte
// or two, more bytes than w * h * 4 + 64 (t1_enc_slab_bytes).
// Buffers are sized as the GPU path sizes them (codec.cpp), so that an access
// outside them is a finding in the shared code: built a second time under
// AddressSanitizer + UBSan by tests/test_host_build.py (no GPU needed).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "../../grokimagecompression_amd/csrc/t1_flat.h"
#include "../../oracle/grk_oracle.h"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
constexpr uint32_t kGapWords = 4;  // a poisoned 16-byte unit between two segments' regions
#else
#define POISON(p, n) ((void)0)
#define UNPOISON(p, n) ((void)0)
constexpr uint32_t kGapWords = 0;
#endif

using namespace grkgpu;
static const uint32_t kTab[47] = GRK_MQ_TABLE_INIT;
static uint32_t kDecTab[MQ_DEC_WORDS];

static uint64_t rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (uint32_t)rng; }

static T1Scratch scr;

// grk_device.h t1_unstuff_region_words: header {nwords, ncarry, -, -}, words, carries
static uint32_t region_words(uint32_t len) { return 4 + unstuff_word_cap(len) + unstuff_carry_cap(len); }

struct Seg { uint32_t off, len, npasses; };

// The codeword segments of the first np passes: a segment ends at every
// terminated pass (t1_pass_term) and at the last pass taken.
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

// What a decode of the first np passes yields, from the full decode `full`
// (|v| = magnitude << 1 | 1, the half-LSB of t1_decode_cblk), sample by
// sample (ISO 15444-1 D.3): plane by plane from the top, the significance
// propagation pass visits, in stripe / column / row order, every
// insignificant sample with a significant 8-neighbour (VSC: the row below a
// stripe's last row counts as insignificant), the refinement pass every
// sample significant before the plane, the cleanup pass the rest.  A sample
// counts as significant once the pass that found it is among the np taken,
// with the refinement bits of the refinement passes taken below it.
static std::vector<int32_t> plain_truncated(const std::vector<int32_t> &full, uint32_t w, uint32_t h, uint32_t numbps,
                                            uint32_t np, bool vsc) {
    const int W = (int)w, H = (int)h, top = (int)numbps - 1;
    std::vector<uint32_t> mag(w * h);
    std::vector<int> sigpass(w * h, -1), sigplane(w * h, -1);
    std::vector<uint8_t> sig(w * h, 0), vis(w * h, 0);
    for (uint32_t i = 0; i < w * h; ++i) mag[i] = (uint32_t)(full[i] < 0 ? -(int64_t)full[i] : full[i]) >> 1;
    auto S = [&](int x, int y) { return x >= 0 && y >= 0 && x < W && y < H && sig[y * W + x]; };
    auto nbr = [&](int x, int y) {
        const bool below = !(vsc && (y & 3) == 3);
        return S(x - 1, y) || S(x + 1, y) || S(x - 1, y - 1) || S(x, y - 1) || S(x + 1, y - 1) ||
               (below && (S(x - 1, y + 1) || S(x, y + 1) || S(x + 1, y + 1)));
    };
    for (int p = top; p >= 0; --p) {
        const int spp = 1 + 3 * (top - 1 - p), cup = p == top ? 0 : spp + 2;
        std::fill(vis.begin(), vis.end(), 0);
        if (p < top)
            for (int k = 0; k < H; k += 4)
                for (int x = 0; x < W; ++x)
                    for (int y = k; y < k + 4 && y < H; ++y) {
                        const int i = y * W + x;
                        if (sig[i] || !nbr(x, y)) continue;
                        vis[i] = 1;
                        if ((mag[i] >> p) & 1u) { sig[i] = 1; sigpass[i] = spp; sigplane[i] = p; }
                    }
        for (int i = 0; i < W * H; ++i)
            if (!sig[i] && !vis[i] && ((mag[i] >> p) & 1u)) { sig[i] = 1; sigpass[i] = cup; sigplane[i] = p; }
    }
    std::vector<int32_t> out(w * h, 0);
    for (uint32_t i = 0; i < w * h; ++i) {
        if (sigpass[i] < 0 || (uint32_t)sigpass[i] >= np) continue;
        int ql = sigplane[i];
        for (int q = sigplane[i] - 1; q >= 0 && (uint32_t)(1 + 3 * (top - 1 - q) + 1) < np; --q) ql = q;
        const int32_t m = (int32_t)(((mag[i] >> ql) << (ql + 1)) | (1u << ql));
        out[i] = full[i] < 0 ? -m : m;
    }
    return out;
}

int main(int argc, char **argv) {
    int iters = argc > 1 ? atoi(argv[1]) : 400;
    int fails = 0;
    for (uint32_t i = 0; i < MQ_DEC_WORDS; ++i) kDecTab[i] = mq_dec_table_entry(kTab, i);
    static uint8_t zc[2048], sc[256], scw[256];
    for (uint32_t i = 0; i < 2048; ++i) zc[i] = zc_lut_entry(i >> 9, i & 511);
    for (uint32_t i = 0; i < 256; ++i) sc[i] = sc_lut_entry(i);
    for (uint32_t i = 0; i < 256; ++i) scw[i] = sc_win_entry(i);
    uint32_t seen_w1 = 0, seen_w63 = 0, seen_w64 = 0, seen_hodd = 0, seen_sty[64] = {0}, decoded = 0, multiseg = 0, vsc_cut = 0;
    uint32_t seen_tiny = 0, tiny_over = 0;  // tiny blocks whose bytes outgrow w * h * 4 + 64 (the terminations decide their size)
    for (int it = 0; it < iters; ++it) {
        // shapes, amplitudes and kinds as test_t1_core.cpp draws them, with the
        // edge widths and stripe-remainder heights at fixed iterations
        uint32_t w = 1 + rnd() % 64, h = 1 + rnd() % 64;
        if (it % 3 == 0) { w = 64; h = 64; }
        if (it % 12 == 1) w = 1;
        if (it % 12 == 5) w = 63;
        if (it % 12 == 7) { w = 64; h = 1 + rnd() % 64; if (h % 4 == 0) h -= 1; }
        uint32_t orient = rnd() % 4;
        int qmfbid = rnd() % 2;
        int32_t inv_step = 1000 + rnd() % 20000;
        uint32_t amp = 1u << (rnd() % (qmfbid ? 15 : 24));
        int kind = rnd() % 4;
        uint32_t sty = 1 + rnd() % 63;
        // blocks of one to four samples, 17 to 19 planes deep, every sample with
        // the top plane's bit, every pass terminated with the long (not the
        // predictable) termination: one to two bytes a pass (mqel_flush's two
        // BYTEOUTs and its bp++ unless the byte is 0xFF, less mqel_restart's
        // step back) for 48 to 54 passes, against w * h * 4 + 64 <= 80 bytes
        // for the samples (t1_enc_slab_bytes).  Most, not all, of these blocks
        // outgrow that figure; the count is checked below.
        const bool tiny = it % 12 == 10;
        if (tiny) {
            static const uint32_t TW[] = {1, 2, 1, 2}, TH[] = {1, 1, 2, 2}, TS[] = {4, 6, 12, 14, 36, 38, 44, 46};
            const uint32_t q = (uint32_t)it / 12;
            w = TW[q % 4]; h = TH[q % 4];
            sty = TS[(q / 4 + q) % 8];
            qmfbid = 1;
            amp = 1u << (16 + q % 3);
            kind = 0;
        }
        std::vector<int32_t> coef(w * h);
        for (uint32_t i = 0; i < w * h; ++i) {
            int32_t v = (int32_t)(rnd() % (2 * amp + 1)) - (int32_t)amp;
            if (kind == 1 && (rnd() % 8)) v = 0;           // sparse
            if (kind == 2) v = (int32_t)(i % w) - (int32_t)(w / 2);  // ramps
            coef[i] = v;
        }
        if (tiny)  // every sample has the top plane's bit
            for (uint32_t i = 0; i < w * h; ++i) coef[i] = coef[i] < 0 ? coef[i] - (int32_t)amp : coef[i] + (int32_t)amp;
        seen_w1 += w == 1; seen_w63 += w == 63; seen_w64 += w == 64; seen_hodd += (h & 3) != 0;
        seen_sty[sty]++;
        // oracle: the cblksty == 0 encode
        std::vector<uint8_t> obuf(w * h * 8 + 64, 0);
        orc_pass op[100];
        uint32_t onb = 0, olen = 0;
        const int onp = orc_t1_encode_cblk(coef.data(), w, w, h, orient, qmfbid, inv_step, obuf.data() + 1,
                                           (uint32_t)obuf.size() - 1, op, &onb, &olen);
        // encode with the style: prep, per-plane context modelling with cblksty
        // and the raw flag as k_t1_model passes them, then the MQ / raw coder
        const uint32_t lnb = t1_prep_serial(coef.data(), w, w, h, qmfbid, inv_step, scr.st, scr.pa);
        t1_prep_above(h, lnb, scr.pa, scr.pb);
        const uint32_t slot = sym_slot_bytes(w, h);
        // the symbol slab: numbps slots, 256 bytes of slack at its end (codec.cpp c->sym)
        std::vector<uint32_t> sym(((size_t)lnb * slot + 256) / 4, 0);
        uint64_t tmp[128];
        for (uint32_t p = 0; p < lnb; ++p) {
            uint32_t *base = sym.data() + (size_t)p * slot / 4;
            const uint64_t *ref = p + 1 < lnb ? scr.pb + (p + 1) * 64 : scr.pb;
            t1_model_plane<const uint64_t *, uint64_t *>(w, h, orient, scr.pa + p * 64, scr.pb + p * 64, ref, p + 1 < lnb,
                                                         scr.st.neg, tmp, sc, base, scr.cnt + p * 4, sty,
                                                         t1_pass_raw(sty, (int32_t)p, 0, lnb));
        }
        // the MQ output: 16 bytes of headroom (the pad byte's commit lands in
        // the dword before the output), then t1_enc_slab_bytes rounded to 16
        // (codec.cpp out_off / out_total)
        const uint32_t slab = t1_enc_slab_bytes(w, h, sty, lnb);
        const size_t obytes = ((size_t)slab + 15) & ~(size_t)15;
        std::vector<uint32_t> sbuf((16 + obytes) / 4, 0);
        uint32_t *sout = sbuf.data() + 4;
        uint32_t srate[100], slen = 0, cx[32];
        const uint32_t snp = (sty & CBLKSTY_LAZY)
                                 ? t1_mq_block<true>(lnb, sym.data(), slot / 4, scr.cnt, kTab, cx, sout, srate, &slen, sty)
                                 : t1_mq_block<false>(lnb, sym.data(), slot / 4, scr.cnt, kTab, cx, sout, srate, &slen, sty);
        if (lnb != onb || (int)snp != onp) {
            printf("PASS COUNT it=%d sty=%u w=%u h=%u np %u/%d nb %u/%u\n", it, sty, w, h, snp, onp, lnb, onb);
            fails++;
            continue;
        }
        if (onp == 0) continue;
        bool mono = slen <= slab;
        for (uint32_t k = 0; mono && k < snp; ++k) mono = srate[k] <= slen && (k == 0 || srate[k] >= srate[k - 1]);
        if (!mono) {
            printf("RATES it=%d sty=%u w=%u h=%u len %u\n", it, sty, w, h, slen);
            fails++;
            continue;
        }
        if (onb > T1_MAX_DEC_BPS) continue;  // refused by the decoder's host side
        if (tiny && (lnb < 17 || !(sty & CBLKSTY_TERMALL))) {
            printf("TINY it=%d sty=%u w=%u h=%u nb %u\n", it, sty, w, h, lnb);
            fails++;
        }
        seen_tiny += tiny;
        tiny_over += tiny && slen > w * h * 4 + 64;
        ++decoded;
        const uint8_t *bytes = (const uint8_t *)sout;
        const uint32_t tnp = (uint32_t)(1 + rnd() % onp);  // the truncated pass count
        std::vector<int32_t> full;                         // the oracle's decode of all passes
        for (int trunc = 0; trunc < 2; ++trunc) {
            const uint32_t np = trunc ? tnp : (uint32_t)onp;
            // reference: the oracle's decode of its own style-0 stream, cut at the same pass
            const uint32_t len0 = op[np - 1].rate;
            std::vector<uint8_t> data(obuf.begin() + 1, obuf.begin() + 1 + len0);
            data.push_back(0); data.push_back(0);
            std::vector<int32_t> od(w * h);
            orc_t1_decode_cblk(data.data(), len0, np, onb, w, h, orient, od.data());
            if (!trunc) full = od;
            if (plain_truncated(full, w, h, onb, np, false) != od) {  // the restatement itself, against the oracle
                printf("PLAIN REFERENCE it=%d w=%u h=%u np=%u/%d nb=%u\n", it, w, h, np, onp, onb);
                fails++;
                continue;
            }
            if (trunc && (sty & CBLKSTY_VSC)) { od = plain_truncated(full, w, h, onb, np, true); vsc_cut += od != full; }

            const std::vector<Seg> segs = split_segments(sty, lnb, np, srate);
            uint32_t sum = 0, npsum = 0;
            for (const Seg &s : segs) { sum += s.len; npsum += s.npasses; }
            bool ok = sum == srate[np - 1] && npsum == np;
            if (!trunc) ok = ok && sum == slen;                         // the segments are the whole stream
            if (sty & CBLKSTY_TERMALL) ok = ok && segs.size() == np;    // every pass ends a segment
            if (!ok) {
                printf("SEGMENTS it=%d sty=%u w=%u h=%u np=%u segs %zu sum %u rate %u len %u\n", it, sty, w, h, np,
                       segs.size(), sum, srate[np - 1], slen);
                fails++;
                continue;
            }
            multiseg += segs.size() > 1;
            // every segment's bytes in an allocation of exactly its length, its
            // unstuffed stream in a region of t1_unstuff_region_words words at
            // ub_off 16-byte units (codec.cpp: regions back to back, 256 bytes
            // of slack after the last)
            std::vector<std::vector<uint8_t>> sdata;
            std::vector<DecSeg> ds(segs.size());
            uint64_t uwords = 0;
            for (size_t q = 0; q < segs.size(); ++q) {
                sdata.emplace_back(bytes + segs[q].off, bytes + segs[q].off + segs[q].len);
                ds[q] = DecSeg{0, segs[q].len, segs[q].npasses, (uint32_t)(uwords / 4), 0};
                uwords += region_words(segs[q].len) + kGapWords;
            }
            const size_t ubytes = uwords * 4 + 256;
            uint32_t *ubuf = (uint32_t *)aligned_alloc(16, ubytes);
            memset(ubuf, 0xA5, ubytes);
            for (size_t q = 0; q < segs.size(); ++q) {
                uint32_t *region = ubuf + (size_t)ds[q].ub_off * 4;
                uint32_t *words = region + 4, *carries = words + unstuff_word_cap(ds[q].len);
                POISON(region + region_words(ds[q].len), kGapWords * 4);
                uint32_t nc = 0;
                region[0] = t1_unstuff(sdata[q].data(), ds[q].len, words, carries, &nc);
                region[1] = nc;
                if (region[0] > unstuff_word_cap(ds[q].len) || nc + 1 > unstuff_carry_cap(ds[q].len)) {
                    printf("UNSTUFF CAP it=%d sty=%u len %u words %u carries %u\n", it, sty, ds[q].len, region[0], nc);
                    fails++;
                }
            }
            // the decoder as k_t1_decode_ub sets it up for a block with segments;
            // the bit-plane rows start as garbage (the kernel does not clear them)
            std::fill(scr.pa, scr.pa + 32 * 64, ~0ull);
            std::fill(scr.pb, scr.pb + 32 * 64, ~0ull);
            for (int i = 0; i < 66; ++i) { scr.st.sig[i] = scr.st.neg[i] = scr.st.vis[i] = scr.st.ref[i] = ~0ull; }
            const DecTables DT{zc + orient * 512, scw, kDecTab};
            uint32_t cxw[32], ring[FB_RING];
            auto run = [&](auto &d) {
                const uint32_t *region = ubuf + (size_t)ds[0].ub_off * 4;
                for (uint32_t y = 0; y < h + 2; ++y) { scr.st.sig[y] = 0; scr.st.neg[y] = 0; scr.st.vis[y] = 0; scr.st.ref[y] = 0; }
                mq_reset_words_dec(cxw, DT.mq);
                d.set_ring(ring, 0);
                d.init(region + 4, region[0], region + 4 + unstuff_word_cap(ds[0].len));
                SegCursor cur{ds.data(), ubuf, (uint32_t)ds.size(), 0, ds[0].npasses};
                t1_decode_passes(d, np, lnb, w, h, scr.st, DT, cxw, scr.pa, scr.pb, sty, cur, 0u);
            };
            if (sty & CBLKSTY_LAZY) { BitDecT<true> d; run(d); }
            else { BitDecT<false> d; run(d); }
            const DecodedPlanes dp = decoded_planes(np, lnb);
            std::vector<int32_t> got(w * h);
            for (uint32_t y = 0; y < h; ++y)
                for (uint32_t x = 0; x < w; ++x) got[y * w + x] = t1_rebuild(x, y, dp, scr.pa, scr.pb, scr.st.neg[y + 1]);
            if (od != got) {
                uint32_t bad = 0;
                while (od[bad] == got[bad]) ++bad;
                printf("DEC MISMATCH it=%d sty=%u w=%u h=%u np=%u/%d nb=%u orient=%u segs=%zu first (x,y)=(%u,%u) %d/%d\n", it,
                       sty, w, h, np, onp, lnb, orient, segs.size(), bad % w, bad / w, got[bad], od[bad]);
                fails++;
            }
            for (size_t q = 0; q < segs.size(); ++q)
                UNPOISON(ubuf + (size_t)ds[q].ub_off * 4 + region_words(ds[q].len), kGapWords * 4);
            free(ubuf);
        }
    }
    // the draw covers what it is meant to (a run of a few hundred blocks)
    if (iters >= 300) {
        uint32_t nsty = 0;
        for (int s = 1; s < 64; ++s) nsty += seen_sty[s] != 0;
        if (!seen_w1 || !seen_w63 || !seen_w64 || !seen_hodd || nsty < 60 || decoded * 2 < (uint32_t)iters || !multiseg || !vsc_cut ||
            seen_tiny < 24 || tiny_over * 2 < seen_tiny) {
            printf("COVERAGE w1 %u w63 %u w64 %u h%%4 %u styles %u decoded %u multi-segment %u tiny blocks past w*h*4+64 %u / %u\n", seen_w1,
                   seen_w63, seen_w64, seen_hodd, nsty, decoded, multiseg, tiny_over, seen_tiny);
            fails++;
        }
    }
    printf("%s: %d failures / %d blocks (%u decoded, %u decodes over several segments, %u tiny blocks past w*h*4+64)\n",
           fails ? "FAIL" : "OK", fails, iters, decoded, multiseg, tiny_over);
    return fails ? 1 : 0;
}
