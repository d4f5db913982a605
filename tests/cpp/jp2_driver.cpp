// tests/cpp/jp2_driver.cpp -- JP2 fixture driver over the public grk_* C API
// (grok.h) only: built against the reference's libgrok by
// scripts/make_golden_jp2.py to make and check tests/golden/jp2_*, and
// against this project's libgrok.so (-DJP2_DRIVER_GRK_API_H -Iinclude) by
// tests/test_gpu_jp2.py, which must reproduce those fixtures through grk_*.
//
//   jp2_driver enc IN.i32 OUT.jp2 W H C BITS SGND -cs COLOURSPACE [-icc FILE] [-alpha a,b,...]
//              [-prec a,b,...] [-sgnd a,b,...] [-sub dx,dy/dx,dy/...] [-I] [-n res] [-t tw,th] [-d x0,y0] [-Y mct]
//       planes (planar int32 little-endian, each component on its own grid)
//       -> a .jp2 file, as grk_compress does for an image with that colour
//       space (GRK_COLOR_SPACE value), ICC profile and per-component alpha
//       types: grk_create_compress(GRK_CODEC_JP2) -> grk_setup_encoder ->
//       grk_start_compress -> grk_encode -> grk_end_compress.
//   jp2_driver dec IN.jp2 OUT.i32 [-r reduce] [-l layers] [-d x0,y0,x1,y1]
//       .jp2 file -> planes, the ICC profile bytes in OUT.i32.icc, and on stdout
//         image x0 y0 x1 y1 numcomps colour_space icc_len
//         comp w h dx dy prec sgnd alpha          (one line per component)
//       A file the library refuses prints "error" and exits 1.
#ifdef JP2_DRIVER_GRK_API_H  // this project's own header (include/grk_api.h) for its libgrok.so
#include "grk_api.h"
#define GRK_JP2_FMT GRKP_JP2_FMT
#else
#include <grok.h>
#endif
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

static std::vector<uint8_t> read_file(const char *p) {
    std::vector<uint8_t> v;
    FILE *f = fopen(p, "rb");
    if (!f) { perror(p); exit(2); }
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize((size_t)n);
    if (n && fread(v.data(), 1, (size_t)n, f) != (size_t)n) { perror(p); exit(2); }
    fclose(f);
    return v;
}

static void write_file(const std::string &p, const void *d, size_t n) {
    FILE *f = fopen(p.c_str(), "wb");
    if (!f || (n && fwrite(d, 1, n, f) != n)) { perror(p.c_str()); exit(2); }
    fclose(f);
}

static std::vector<uint32_t> parse_list(const char *s) {
    std::vector<uint32_t> out;
    while (*s) {
        out.push_back((uint32_t)strtoul(s, (char **)&s, 10));
        if (*s == ',') s++;
        else break;
    }
    return out;
}

static uint32_t cdivu(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

static int enc(int argc, char **argv) {
    if (argc < 9) return 2;
    const uint32_t w = (uint32_t)atoi(argv[4]), h = (uint32_t)atoi(argv[5]), c = (uint32_t)atoi(argv[6]);
    const uint32_t bits = (uint32_t)atoi(argv[7]), sgnd = (uint32_t)atoi(argv[8]);
    grk_cparameters p;
    grk_set_default_encoder_parameters(&p);
    int mct = -1;
    uint32_t cs = GRK_CLRSPC_UNKNOWN;
    std::vector<uint32_t> alpha, prec, sg;
    std::vector<std::pair<uint32_t, uint32_t>> sub;
    std::vector<uint8_t> icc;
    for (int i = 9; i < argc; ++i) {
        const std::string a = argv[i];
        const char *v = i + 1 < argc ? argv[i + 1] : "";
        if (a == "-I") { p.irreversible = true; continue; }
        ++i;
        if (a == "-cs") cs = (uint32_t)atoi(v);
        else if (a == "-icc") icc = read_file(v);
        else if (a == "-alpha") alpha = parse_list(v);
        else if (a == "-prec") prec = parse_list(v);
        else if (a == "-sgnd") sg = parse_list(v);
        else if (a == "-n") p.numresolution = (uint32_t)atoi(v);
        else if (a == "-Y") mct = atoi(v);
        else if (a == "-t") { if (sscanf(v, "%u,%u", &p.cp_tdx, &p.cp_tdy) != 2) return 2; p.tile_size_on = true; }
        else if (a == "-d") { if (sscanf(v, "%u,%u", &p.image_offset_x0, &p.image_offset_y0) != 2) return 2; }
        else if (a == "-sub") {
            const char *s = v;
            uint32_t dx, dy;
            while (sscanf(s, "%u,%u", &dx, &dy) == 2) {
                sub.push_back({dx, dy});
                while (*s && *s != '/') s++;
                if (!*s) break;
                s++;
            }
        } else { fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
    }
    p.tcp_rates[0] = 0;  // one lossless-rate layer, grk_compress's default
    p.tcp_numlayers = 1;
    p.cp_disto_alloc = 1;
    p.tcp_mct = (uint8_t)(mct >= 0 ? mct : (c >= 3 ? 1 : 0));
    p.cod_format = GRK_JP2_FMT;
    std::vector<grk_image_cmptparm> cm(c);
    memset(cm.data(), 0, c * sizeof(grk_image_cmptparm));
    size_t need = 0;
    for (uint32_t k = 0; k < c; ++k) {
        cm[k].prec = k < prec.size() ? prec[k] : bits;
        cm[k].sgnd = k < sg.size() ? sg[k] : sgnd;
        cm[k].dx = k < sub.size() ? sub[k].first : 1;
        cm[k].dy = k < sub.size() ? sub[k].second : 1;
        cm[k].w = cdivu(p.image_offset_x0 + w, cm[k].dx) - cdivu(p.image_offset_x0, cm[k].dx);
        cm[k].h = cdivu(p.image_offset_y0 + h, cm[k].dy) - cdivu(p.image_offset_y0, cm[k].dy);
        cm[k].x0 = cdivu(p.image_offset_x0, cm[k].dx);
        cm[k].y0 = cdivu(p.image_offset_y0, cm[k].dy);
        need += (size_t)cm[k].w * cm[k].h * 4;
    }
    const std::vector<uint8_t> in = read_file(argv[2]);
    if (in.size() != need) { fprintf(stderr, "input size mismatch\n"); return 2; }
    grk_initialize(nullptr, 0);
    grk_image *img = grk_image_create(c, cm.data(), (GRK_COLOR_SPACE)cs);
    if (!img) return 1;
    img->x0 = p.image_offset_x0;
    img->y0 = p.image_offset_y0;
    img->x1 = p.image_offset_x0 + w;
    img->y1 = p.image_offset_y0 + h;
    size_t off = 0;
    for (uint32_t k = 0; k < c; ++k) {
        const size_t n = (size_t)cm[k].w * cm[k].h;
        memcpy(img->comps[k].data, in.data() + off, n * 4);
        off += n * 4;
        img->comps[k].alpha = (uint16_t)(k < alpha.size() ? alpha[k] : 0);
    }
    if (!icc.empty()) {  // (the encoder copies it)
        img->icc_profile_buf = icc.data();
        img->icc_profile_len = (uint32_t)icc.size();
    }
    const size_t cap = need + (1 << 20);
    std::vector<uint8_t> buf(cap);
    grk_stream *st = grk_stream_create_mem_stream(buf.data(), cap, false, false);
    grk_codec *codec = grk_create_compress(GRK_CODEC_JP2, st);
    const bool ok = codec && grk_setup_encoder(codec, &p, img) && grk_start_compress(codec, img) && grk_encode(codec) &&
                    grk_end_compress(codec);
    if (ok) write_file(argv[3], buf.data(), grk_stream_get_write_mem_stream_length(st));
    if (codec) grk_destroy_codec(codec);
    grk_stream_destroy(st);
    img->icc_profile_buf = nullptr;
    img->icc_profile_len = 0;
    grk_image_destroy(img);
    grk_deinitialize();
    if (!ok) printf("error\n");
    return ok ? 0 : 1;
}

static int dec(int argc, char **argv) {
    grk_dparameters dp;
    grk_set_default_decoder_parameters(&dp);
    uint32_t area[4] = {0, 0, 0, 0};
    for (int i = 4; i + 1 < argc; i += 2) {
        const std::string a = argv[i];
        if (a == "-r") dp.cp_reduce = (uint32_t)atoi(argv[i + 1]);
        else if (a == "-l") dp.cp_layer = (uint32_t)atoi(argv[i + 1]);
        else if (a == "-d") {
            if (sscanf(argv[i + 1], "%u,%u,%u,%u", &area[0], &area[1], &area[2], &area[3]) != 4) return 2;
        } else return 2;
    }
    std::vector<uint8_t> file = read_file(argv[2]);
    grk_initialize(nullptr, 0);
    grk_stream *st = grk_stream_create_mem_stream(file.data(), file.size(), false, true);
    grk_codec *codec = grk_create_decompress(GRK_CODEC_JP2, st);
    grk_header_info hi;
    memset(&hi, 0, sizeof(hi));
    grk_image *img = nullptr;
    bool ok = codec && grk_setup_decoder(codec, &dp) && grk_read_header(codec, &hi, &img);
    if (ok) ok = grk_set_decode_area(codec, img, area[0], area[1], area[2], area[3]);
    if (ok) ok = grk_decode(codec, nullptr, img) && grk_end_decompress(codec);
    if (ok)
        for (uint32_t k = 0; k < img->numcomps; ++k) ok = ok && img->comps[k].data;
    if (!ok) {
        printf("error\n");
        return 1;
    }
    std::vector<int32_t> out;
    for (uint32_t k = 0; k < img->numcomps; ++k) {
        const grk_image_comp &cm = img->comps[k];
        out.insert(out.end(), cm.data, cm.data + (size_t)cm.w * cm.h);
    }
    write_file(argv[3], out.data(), out.size() * 4);
    write_file(std::string(argv[3]) + ".icc", img->icc_profile_buf, img->icc_profile_buf ? img->icc_profile_len : 0);
    printf("image %u %u %u %u %u %d %u\n", img->x0, img->y0, img->x1, img->y1, img->numcomps, (int)img->color_space,
           img->icc_profile_buf ? img->icc_profile_len : 0);
    for (uint32_t k = 0; k < img->numcomps; ++k) {
        const grk_image_comp &cm = img->comps[k];
        printf("comp %u %u %u %u %u %u %u\n", cm.w, cm.h, cm.dx, cm.dy, cm.prec, cm.sgnd, (unsigned)cm.alpha);
    }
    grk_image_destroy(img);
    grk_destroy_codec(codec);
    grk_stream_destroy(st);
    grk_deinitialize();
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: see tests/cpp/jp2_driver.cpp\n");
        return 2;
    }
    const std::string mode = argv[1];
    if (mode == "enc") return enc(argc, argv);
    if (mode == "dec") return dec(argc, argv);
    return 2;
}
