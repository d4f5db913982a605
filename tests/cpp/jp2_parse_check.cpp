// jp2_parse_check.cpp -- the JP2 box reader (csrc/jp2.cpp) over damaged files,
// as a stand-alone program so that it can run under AddressSanitizer / UBSan
// (tests/test_jp2_host.py builds it that way): every truncation of each file
// and 5,000 seeded random corruptions of its first 600 bytes.  Each parse must
// return without touching memory it does not own, a refusal must carry a
// message, and a palette the parser accepts must lie inside the table it
// reports.
//   jp2_parse_check FILE.jp2...
#include <stdio.h>

#include <string>
#include <vector>

#include "codestream.h"
#include "jp2.h"

using namespace grkgpu;

static int check(const std::vector<uint8_t> &file, size_t len, unsigned &ok, unsigned &refused) {
    // a buffer of exactly len bytes: a read past the end is the sanitizer's to find
    std::vector<uint8_t> buf(file.begin(), file.begin() + len);
    Jp2Boxes b;
    std::string err;
    Jp2Status st = jp2_read_boxes(buf.data(), buf.size(), b, err);
    CodingParams cp;
    if (st == JP2_OK) {
        if (b.cs_off > buf.size() || b.cs_len > buf.size() - b.cs_off) { fprintf(stderr, "codestream outside the file\n"); return 1; }
        if (b.icc_len && (b.icc_off > buf.size() || b.icc_len > buf.size() - b.icc_off)) { fprintf(stderr, "ICC profile outside the file\n"); return 1; }
        size_t sot = 0;
        if (!parse_main_header(buf.data() + b.cs_off, (size_t)b.cs_len, cp, sot, err)) st = JP2_UNSUPPORTED;
    }
    Jp2Channels ch;
    if (st == JP2_OK) st = jp2_resolve_channels(b, cp.numcomps, cp.prec, cp.sgnd, cp.dx, cp.dy, 16, ch, err);
    if (st != JP2_OK) {
        if (err.empty()) { fprintf(stderr, "refusal without a message\n"); return 1; }
        ++refused;
        return 0;
    }
    ++ok;
    if (ch.ch.empty() || ch.ch.size() > 16) { fprintf(stderr, "bad channel count\n"); return 1; }
    if (ch.palette && (b.ne < 1 || b.ne > 1024 || b.npc < 1 || b.npc > 16 || b.entries.size() != (size_t)b.ne * b.npc)) {
        fprintf(stderr, "palette table of a wrong size\n");
        return 1;
    }
    for (const Jp2Channel &c : ch.ch) {
        if (c.comp >= cp.numcomps || c.pcol >= (int32_t)(ch.palette ? b.npc : 0)) { fprintf(stderr, "channel outside the table\n"); return 1; }
        if (c.pcol >= 0 && (c.prec < 1 || c.prec > 16)) { fprintf(stderr, "looked-up channel wider than 16 bits\n"); return 1; }
    }
    return 0;
}

int main(int argc, char **argv) {
    for (int a = 1; a < argc; ++a) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> file;
        uint8_t tmp[4096];
        for (size_t n; (n = fread(tmp, 1, sizeof(tmp), f)) > 0;) file.insert(file.end(), tmp, tmp + n);
        fclose(f);
        unsigned ok = 0, refused = 0;
        if (check(file, file.size(), ok, refused) || ok != 1) { fprintf(stderr, "%s: the file itself is refused\n", argv[a]); return 1; }
        for (size_t len = 0; len < file.size(); ++len)
            if (check(file, len, ok, refused)) return 1;
        const size_t span = file.size() < 600 ? file.size() : 600;
        uint32_t s = 0x9E3779B9u ^ (uint32_t)a;
        auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
        for (int it = 0; it < 5000; ++it) {
            std::vector<uint8_t> d = file;
            const int nb = 1 + (int)(rnd() % 3);
            for (int j = 0; j < nb; ++j) d[rnd() % span] = (uint8_t)rnd();
            if (check(d, d.size(), ok, refused)) return 1;
        }
        printf("%s: %zu bytes, %u accepted, %u refused\n", argv[a], file.size(), ok, refused);
    }
    return 0;
}
