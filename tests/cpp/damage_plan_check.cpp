// The decoder's host half (DecHost::begin / parse_tiles / finish, decode_packet,
// walk_tile_parts) on damaged streams, built with AddressSanitizer and UBSan
// (tests/test_damage_host.py test_sanitized_plan_check).  Host code only: no
// device call is made.
//
//   damage_plan_check CASES.bin
// CASES.bin (little-endian, written by the test from
// tests/golden/manifest_damage.json): u32 streams; per stream u32 len,
// u32 subsampled, u32 cases, the stream's bytes, then per case u32 patches and
// (u32 offset, u32 value) each.
//
// Every case is applied to a malloc copy of exactly the stream's length (a
// read one byte past it is a report) and goes through the batch plan
// (grkgpu_batch_convert_plan for a subsampled stream, which grkgpu_batch_plan
// refuses) and through grkgpu_dec_tables_of, whose tables are read end to
// end; then the same copies go through the plan in lists of 16, a clean copy
// in every fourth place.  An item's status must be the same alone, in its
// list and in the export.  Prints "cases N refused R mismatches M"; exit
// status 1 when M != 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "grk_mi355x.h"

static uint32_t rd32(FILE *f) {
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) { fprintf(stderr, "short case file\n"); exit(2); }
    return b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24);
}

static int plan(grkgpu_batch_item *items, uint32_t n, bool subs) {
    grkgpu_batch_info info;
    return subs ? grkgpu_batch_convert_plan(items, nullptr, n, nullptr, &info) : grkgpu_batch_plan(items, n, nullptr, &info);
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const uint32_t nstreams = rd32(f);
    uint64_t ncases = 0, refused = 0, mismatches = 0, sum = 0;
    for (uint32_t s = 0; s < nstreams; ++s) {
        const uint32_t len = rd32(f), subs = rd32(f), nc = rd32(f);
        std::vector<uint8_t> clean(len);
        if (fread(clean.data(), 1, len, f) != len) return 2;
        std::vector<uint8_t *> copies;
        std::vector<int> alone;
        for (uint32_t c = 0; c < nc; ++c, ++ncases) {
            uint8_t *cs = (uint8_t *)malloc(len);
            memcpy(cs, clean.data(), len);
            for (uint32_t np = rd32(f); np; --np) {
                const uint32_t off = rd32(f), val = rd32(f);
                if (off >= len) return 2;
                cs[off] = (uint8_t)val;
            }
            grkgpu_batch_item it;
            memset(&it, 0, sizeof(it));
            it.cs = cs;
            it.len = len;
            const int rc = plan(&it, 1, subs != 0);
            if (rc != it.status) ++mismatches;
            grkgpu_dec_tables t;
            const int trc = grkgpu_dec_tables_of(cs, len, nullptr, &t);
            if (trc != rc) {
                fprintf(stderr, "stream %u case %u: plan %d, tables %d\n", s, c, rc, trc);
                ++mismatches;
            }
            if (!trc) {  // every entry read
                for (uint32_t i = 0; i < t.n_blocks; ++i)
                    sum += t.blocks[i].data_off + t.blocks[i].dst_off + t.blocks[i].len + t.style[i] + t.seg_first[i] +
                           (t.roi ? t.roi[i] : 0);
                sum += t.seg_first[t.n_blocks];
                for (uint32_t i = 0; i < t.n_segs; ++i) {
                    sum += t.segs[i].len + t.segs[i].npasses;
                    if (t.segs[i].data_off + t.segs[i].len > t.data_bytes) ++mismatches;
                    // the bytes a segment inside the stream points at
                    if (t.segs[i].len && t.segs[i].data_off + t.segs[i].len <= len)
                        sum += cs[t.segs[i].data_off] + cs[t.segs[i].data_off + t.segs[i].len - 1];
                }
                grkgpu_dec_tables_free(&t);
            } else {
                ++refused;
            }
            copies.push_back(cs);
            alone.push_back(rc);
        }
        // lists of 16, good and bad mixed
        for (size_t c0 = 0; c0 < copies.size(); c0 += 12) {
            grkgpu_batch_item items[16];
            int want[16];
            memset(items, 0, sizeof(items));
            size_t c = c0;
            uint32_t n = 0;
            for (; n < 16 && (n % 4 == 3 || c < copies.size()); ++n) {
                if (n % 4 == 3) {
                    items[n].cs = clean.data();
                    want[n] = 0;
                } else {
                    items[n].cs = copies[c];
                    want[n] = alone[c++];
                }
                items[n].len = len;
            }
            int first = 0;
            for (uint32_t i = 0; i < n && !first; ++i) first = want[i];
            if (plan(items, n, subs != 0) != first) ++mismatches;
            for (uint32_t i = 0; i < n; ++i)
                if (items[i].status != want[i]) {
                    fprintf(stderr, "stream %u list at %zu item %u: %d in the list, %d alone\n", s, c0, i, items[i].status,
                            want[i]);
                    ++mismatches;
                }
        }
        for (uint8_t *p : copies) free(p);
    }
    fclose(f);
    printf("cases %llu refused %llu mismatches %llu (checksum %llu)\n", (unsigned long long)ncases,
           (unsigned long long)refused, (unsigned long long)mismatches, (unsigned long long)sum);
    return mismatches ? 1 : 0;
}
