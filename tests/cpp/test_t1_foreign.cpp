// Host-side check of the T1 decoder's input side on code-block bytes that no
// Grok encoder writes: a marker inside a segment, a segment shorter than the
// decoder consumes, a segment ending in 0xFF, FF 80..8F pairs at any density.
// The device code of t1_flat.h / t1_dec.h compiled for the host (t1_unstuff,
// t1_decode_v5, t1_rebuild) against the oracle's orc_t1_decode_cblk, case by
// case.  The cases come from a file that tests/foreign_bytes.py writes
// (write_host_cases); the four byte families and the three edits are restated
// here, and every case's bytes must equal the restatement.  The segment sits
// at the case's alignment mod 16 in an allocation of exactly its length, the
// unstuffed words and the carry events in allocations of exactly
// unstuff_word_cap / unstuff_carry_cap words, so that an access outside them is
// a finding: built a second time under AddressSanitizer + UBSan by
// tests/test_host_build.py (no GPU needed).
//   test_t1_foreign <cases file>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "../../grokimagecompression_amd/csrc/t1_flat.h"
#include "../../oracle/grk_oracle.h"

using namespace grkgpu;
static const uint32_t kTab[47] = GRK_MQ_TABLE_INIT;
static uint32_t kDecTab[MQ_DEC_WORDS];
static T1Scratch scr;

// tests/foreign_bytes.py Gen: xorshift64, eight bytes per step, least significant first
struct Gen {
    uint64_t s;
    uint32_t have = 0;
    uint64_t cur = 0;
    explicit Gen(uint32_t seed) : s(((uint64_t)seed + 1) * 0x9E3779B97F4A7C15ull) {
        if (!s) s = 88172645463325252ull;
    }
    uint8_t byte() {
        if (!have) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; cur = s; have = 8; }
        const uint8_t b = (uint8_t)cur;
        cur >>= 8;
        --have;
        return b;
    }
};

enum { UNIFORM, FFDENSE, CARRYMAX, STUFFED, TRIM, MARKER_AT, END_FF, NKINDS };

static std::vector<uint8_t> restate(uint32_t kind, uint32_t seed, uint32_t param, const std::vector<uint8_t> &base,
                                    uint32_t len) {
    Gen g(seed);
    std::vector<uint8_t> o(len);
    switch (kind) {
    case UNIFORM:
        for (auto &b : o) b = g.byte();
        break;
    case FFDENSE:  // 1/4 FF, 1/4 80..8F, the rest uniform
        for (auto &b : o) { const uint8_t a = g.byte(), c = g.byte(); b = (a & 3) == 0 ? 0xFF : (a & 3) == 1 ? (0x80 | (c & 15)) : c; }
        break;
    case CARRYMAX:  // FF 8x FF 8x ...
        for (uint32_t i = 0; i < len; ++i) { const uint8_t a = g.byte(); o[i] = i % 2 == 0 ? 0xFF : (0x80 | (a & 15)); }
        break;
    case STUFFED:  // 00..7F with 1/16 FF, never two in a row
        for (uint32_t i = 0; i < len; ++i) {
            const uint8_t a = g.byte(), c = g.byte();
            o[i] = ((a & 15) == 0 && !(i && o[i - 1] == 0xFF)) ? 0xFF : (c & 0x7F);
        }
        break;
    case TRIM:  // the last param bytes dropped
        o.assign(base.begin(), base.end() - param);
        break;
    case MARKER_AT:  // FF 90 at param, param + 1
        o = base;
        o[param] = 0xFF;
        o[param + 1] = 0x90;
        break;
    case END_FF:
        o = base;
        o.back() = 0xFF;
        break;
    }
    return o;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    for (uint32_t i = 0; i < MQ_DEC_WORDS; ++i) kDecTab[i] = mq_dec_table_entry(kTab, i);
    static uint8_t zc[2048], scw[256];
    for (uint32_t i = 0; i < 2048; ++i) zc[i] = zc_lut_entry(i >> 9, i & 511);
    for (uint32_t i = 0; i < 256; ++i) scw[i] = sc_win_entry(i);
    uint32_t n = 0, fails = 0, seen[NKINDS] = {0}, markers = 0, maxcarry = 0, nonzero = 0;
    if (fread(&n, 4, 1, f) != 1) return 2;
    for (uint32_t it = 0; it < n; ++it) {
        uint32_t hd[11];
        if (fread(hd, 4, 11, f) != 11) return 2;
        const uint32_t kind = hd[0], seed = hd[1], param = hd[2], blen = hd[3], len = hd[4], nb = hd[5], np = hd[6],
                       w = hd[7], h = hd[8], orient = hd[9], align = hd[10];
        std::vector<uint8_t> base(blen), seg(len);
        if (blen && fread(base.data(), 1, blen, f) != blen) return 2;
        if (len && fread(seg.data(), 1, len, f) != len) return 2;
        // the entry points' contract
        if (kind >= NKINDS || !len || len > 64 * 64 * 4 + 64 || nb < 1 || nb > 30 || np < 1 || np > 3 * nb - 2 || w < 1 ||
            w > 64 || h < 1 || h > 64 || orient > 3 || align > 15) {
            printf("BAD CASE it=%u\n", it);
            return 2;
        }
        seen[kind]++;
        if (restate(kind, seed, param, base, len) != seg) {
            printf("BYTES it=%u kind=%u seed=%u len=%u: the file's bytes are not the restatement's\n", it, kind, seed, len);
            fails++;
            continue;
        }
        // the oracle (2 writable bytes after len: its fake FF FF)
        std::vector<uint8_t> data(seg);
        data.push_back(0); data.push_back(0);
        std::vector<int32_t> od(w * h, 0x5A5A5A5A);
        orc_t1_decode_cblk(data.data(), len, np, nb, w, h, orient, od.data());
        // the segment at its alignment, the last byte of the allocation its last byte
        void *raw = nullptr;
        if (posix_memalign(&raw, 16, (size_t)align + len)) return 2;
        uint8_t *lp = (uint8_t *)raw + align;
        memcpy(lp, seg.data(), len);
        const uint32_t wcap = unstuff_word_cap(len), ccap = unstuff_carry_cap(len);
        uint32_t *words = (uint32_t *)aligned_alloc(16, (size_t)wcap * 4);
        uint32_t *carr = (uint32_t *)aligned_alloc(16, (size_t)ccap * 4);
        memset(words, 0xA5, (size_t)wcap * 4);
        memset(carr, 0xA5, (size_t)ccap * 4);
        uint32_t ncar = 0;
        const uint32_t nw = t1_unstuff(lp, len, words, carr, &ncar);
        if (nw > wcap || ncar + 1 > ccap) {
            printf("UNSTUFF CAP it=%u kind=%u len %u words %u / %u carries %u / %u\n", it, kind, len, nw, wcap, ncar + 1, ccap);
            fails++;
        }
        bool mk = false;
        for (uint32_t i = 1; i < len && !mk; ++i) mk = seg[i - 1] == 0xFF && seg[i] > 0x8F;
        markers += mk;
        if (ncar == len / 2 && len >= 2) maxcarry++;
        // the bit-plane rows and the state start as garbage (the kernel does not clear them)
        std::fill(scr.pa, scr.pa + 32 * 64, ~0ull);
        std::fill(scr.pb, scr.pb + 32 * 64, ~0ull);
        for (int i = 0; i < 66; ++i) { scr.st.sig[i] = scr.st.neg[i] = scr.st.vis[i] = scr.st.ref[i] = ~0ull; }
        const DecTables DT{zc + orient * 512, scw, kDecTab};
        uint32_t cx[32], ring[FB_RING];
        t1_decode_v5(words, nw, carr, np, nb, w, h, scr.st, DT, cx, scr.pa, scr.pb, ring, 0);
        const DecodedPlanes dp = decoded_planes(np, nb);
        std::vector<int32_t> got(w * h);
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) got[y * w + x] = t1_rebuild(x, y, dp, scr.pa, scr.pb, scr.st.neg[y + 1]);
        if (od != got) {
            uint32_t bad = 0;
            while (od[bad] == got[bad]) ++bad;
            printf("DEC MISMATCH it=%u kind=%u seed=%u len=%u align=%u w=%u h=%u np=%u nb=%u orient=%u first (x,y)=(%u,%u) %d/%d\n",
                   it, kind, seed, len, align, w, h, np, nb, orient, bad % w, bad / w, got[bad], od[bad]);
            fails++;
        }
        nonzero += std::any_of(od.begin(), od.end(), [](int32_t v) { return v != 0; });
        free(raw);
        free(words);
        free(carr);
    }
    fclose(f);
    // the list covers what it is meant to
    bool cov = markers > 0 && maxcarry > 0 && nonzero * 2 > n;
    for (uint32_t k = 0; k < NKINDS; ++k) cov = cov && seen[k] > 0;
    if (!cov) {
        printf("COVERAGE markers %u full-carry %u non-zero decodes %u\n", markers, maxcarry, nonzero);
        fails++;
    }
    printf("%s: %u failures / %u cases (%u with a marker, %u with len / 2 carry events, %u non-zero)\n", fails ? "FAIL" : "OK",
           fails, n, markers, maxcarry, nonzero);
    return fails ? 1 : 0;
}
