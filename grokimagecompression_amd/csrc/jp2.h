// jp2.h -- the JP2 file format's box layer (ISO/IEC 15444-1 Annex I), host
// code only: the reader and writer of Grok's codestream/jp2.cpp restated, and
// the channel list jp2_decode leaves behind (jp2_check_color, jp2_apply_pclr,
// jp2_apply_cdef) worked out without touching a sample.  No device, no HIP.
#pragma once
#include <stdint.h>
#include <stddef.h>

#include <string>
#include <vector>

namespace grkgpu {

// what a refusal is: the reference refuses the file too (JP2_CORRUPT), or it
// decodes it and this decoder deliberately does not (JP2_UNSUPPORTED)
enum Jp2Status { JP2_OK = 0, JP2_CORRUPT = 1, JP2_UNSUPPORTED = 2 };

// GRK_CLRSPC_* (grok.h), as jp2_decode sets image->color_space
enum Jp2ColourSpace : uint32_t {
    JP2_CS_UNKNOWN = 0, JP2_CS_UNSPECIFIED = 1, JP2_CS_SRGB = 2, JP2_CS_GRAY = 3, JP2_CS_SYCC = 4, JP2_CS_EYCC = 5,
    JP2_CS_CMYK = 6, JP2_CS_DEFAULT_CIE = 7, JP2_CS_CUSTOM_CIE = 8, JP2_CS_ICC = 9
};

struct Jp2Cmap { uint16_t cmp; uint8_t mtyp, pcol; };
struct Jp2Cdef { uint16_t cn, typ, asoc; };

// the boxes of a file, as jp2_read_header_procedure leaves the grk_jp2
struct Jp2Boxes {
    uint64_t cs_off = 0, cs_len = 0;  // the jp2c payload
    // ihdr / bpcc (informational: the geometry comes from SIZ)
    bool have_ihdr = false;
    uint32_t w = 0, h = 0, numcomps = 0, bpc = 0, C = 0, UnkC = 0, IPR = 0;
    std::vector<uint8_t> bpcc;
    // colr (the first one; METH > 2 leaves have_colr false)
    bool have_colr = false;
    uint32_t meth = 0, precedence = 0, approx = 0, enumcs = 0;
    uint64_t icc_off = 0;   // METH 2: the profile inside the file
    uint32_t icc_len = 0;
    uint32_t ncielab = 0;   // EnumCS 14: 2 (default) or 9 words, as jp2_read_colr builds them
    uint32_t cielab[9] = {};
    // pclr / cmap
    bool have_pclr = false, have_cmap = false;
    uint32_t ne = 0, npc = 0;
    std::vector<uint8_t> pal_size, pal_sign;  // per column: bits, sign flag
    std::vector<uint32_t> entries;            // ne x npc, row-major
    std::vector<Jp2Cmap> cmap;                // npc entries
    // cdef
    bool have_cdef = false;
    std::vector<Jp2Cdef> cdef;
};

// Box walk of a whole file.  JP2_CORRUPT where the reference's
// jp2_read_header fails before it reaches the codestream.
Jp2Status jp2_read_boxes(const uint8_t *file, size_t len, Jp2Boxes &b, std::string &err);

// one output channel of the decoded image
struct Jp2Channel {
    uint32_t comp = 0;   // codestream component that feeds it
    int32_t pcol = -1;   // palette column looked up with that component's sample, or -1: the sample itself
    uint32_t prec = 0;
    int32_t sgnd = 0;
    uint32_t alpha = 0;  // grk_image_comp::alpha: the cdef Typ (0 colour, 1 opacity, 2 premultiplied opacity, 65535)
    uint32_t dx = 1, dy = 1;
};
struct Jp2Channels {
    uint32_t colour_space = JP2_CS_UNKNOWN;
    std::vector<Jp2Channel> ch;
    bool palette = false;  // a pclr + cmap pair is applied (b.have_pclr alone is not: Part 1, I.5.3.4)
    bool mapped = false;   // the channels are not the components in order (palette or a cdef swap)
};
// jp2_decode's steps after the codestream: jp2_check_color (which may repair
// b.cmap), the colour space, jp2_apply_pclr, jp2_apply_cdef -- on the SIZ
// components (prec, sgnd, dx, dy).  JP2_UNSUPPORTED with the narrowings listed
// in DESIGN.md.
Jp2Status jp2_resolve_channels(Jp2Boxes &b, uint32_t numcomps, const uint32_t *prec, const int32_t *sgnd,
                               const uint32_t *dx, const uint32_t *dy, uint32_t max_channels, Jp2Channels &out,
                               std::string &err);

// Writer (jp2_setup_encoder + jp2_setup_header_writing's procedures): every box
// up to and including the jp2c box header, whose LBox is left 0 at
// out.size() - 8 for the caller to set to 8 + the codestream's length.
struct Jp2WriteParams {
    uint32_t w = 0, h = 0, numcomps = 0;
    uint32_t prec[16] = {};
    int32_t sgnd[16] = {};
    uint32_t alpha[16] = {};  // grk_image_comp::alpha of each component
    uint32_t colour_space = JP2_CS_UNKNOWN;
    const uint8_t *icc = nullptr;  // JP2_CS_ICC: the profile (METH 2)
    uint32_t icc_len = 0;
};
bool jp2_write_boxes(const Jp2WriteParams &p, std::vector<uint8_t> &out, std::string &err);

}  // namespace grkgpu
