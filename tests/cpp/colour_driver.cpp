// tests/cpp/colour_driver.cpp -- fixture driver around the reference's colour
// step: scripts/make_golden_colour.py links it with the reference's own
// bin/common/color.cpp (compiled as it stands) and libgrok into oracle/_ref/
// to record what color_esycc_to_rgb / color_cmyk_to_rgb make of the inputs of
// tests/colour_fixtures.py (nothing compiled is committed).
//
//   colour_driver eycc|cmyk IN.i32 OUT.i32 N prec,prec,... sgnd,sgnd,...
//       IN: numcomps planes of N int32 samples (little-endian), one after the
//       other, all on one grid; OUT: the planes the conversion leaves (CMYK:
//       one fewer); stdout: "comp prec sgnd" per output component.  A
//       conversion the reference refuses prints "error" and exits 1.
#include <grok.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "color.h"

static std::vector<uint32_t> parse_list(const char *s) {
    std::vector<uint32_t> out;
    while (*s) {
        out.push_back((uint32_t)strtoul(s, (char **)&s, 10));
        if (*s == ',') s++;
        else break;
    }
    return out;
}

int main(int argc, char **argv) {
    if (argc != 7) { fprintf(stderr, "usage: colour_driver eycc|cmyk IN OUT N precs sgnds\n"); return 2; }
    const bool cmyk = !strcmp(argv[1], "cmyk");
    const uint32_t n = (uint32_t)strtoul(argv[4], nullptr, 10);
    const std::vector<uint32_t> prec = parse_list(argv[5]), sgnd = parse_list(argv[6]);
    const uint32_t nc = (uint32_t)prec.size();
    if (!nc || sgnd.size() != nc || !n) return 2;
    std::vector<grk_image_cmptparm> cp(nc);
    for (uint32_t k = 0; k < nc; ++k) {
        memset(&cp[k], 0, sizeof(cp[k]));
        cp[k].dx = cp[k].dy = 1;
        cp[k].w = n;
        cp[k].h = 1;
        cp[k].prec = prec[k];
        cp[k].sgnd = sgnd[k];
    }
    grk_image *img = grk_image_create(nc, cp.data(), GRK_CLRSPC_UNKNOWN);
    if (!img) return 2;
    img->x0 = img->y0 = 0;
    img->x1 = n;
    img->y1 = 1;
    FILE *f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    for (uint32_t k = 0; k < nc; ++k)
        if (fread(img->comps[k].data, 4, n, f) != n) { perror(argv[2]); return 2; }
    fclose(f);
    const bool ok = cmyk ? color_cmyk_to_rgb(img) : color_esycc_to_rgb(img);
    if (!ok) { printf("error\n"); return 1; }
    f = fopen(argv[3], "wb");
    if (!f) { perror(argv[3]); return 2; }
    for (uint32_t k = 0; k < img->numcomps; ++k) {
        if (fwrite(img->comps[k].data, 4, n, f) != n) { perror(argv[3]); return 2; }
        printf("comp %u %u\n", img->comps[k].prec, img->comps[k].sgnd);
    }
    fclose(f);
    grk_image_destroy(img);
    return 0;
}
