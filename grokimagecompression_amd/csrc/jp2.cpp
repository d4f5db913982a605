// jp2.cpp -- JP2 boxes on the host (see jp2.h).  Line references are to Grok
// v5.1.0, src/lib/jp2/codestream/jp2.cpp.  The reader keeps the reference's
// order of checks, so a file is refused where the reference refuses it.
#include "jp2.h"

#include <string.h>

#include <algorithm>

namespace grkgpu {

namespace {

constexpr uint32_t BOX_JP = 0x6a502020, BOX_FTYP = 0x66747970, BOX_JP2H = 0x6a703268, BOX_IHDR = 0x69686472,
                   BOX_COLR = 0x636f6c72, BOX_JP2C = 0x6a703263, BOX_PCLR = 0x70636c72, BOX_CMAP = 0x636d6170,
                   BOX_CDEF = 0x63646566, BOX_BPCC = 0x62706363, BOX_RES = 0x72657320, BOX_RESC = 0x72657363,
                   BOX_RESD = 0x72657364, BOX_XML = 0x786d6c20, BOX_UUID = 0x75756964;
// JP2_STATE (jp2.h:100-108).  UNKNOWN has every bit set: once an unknown box
// was skipped the reference takes the header and the codestream for seen.
constexpr uint32_t ST_SIGNATURE = 1, ST_FILE_TYPE = 2, ST_HEADER = 4, ST_UNKNOWN = 0x7fffffff;
constexpr uint32_t MAX_NUM_COMPONENTS = 16384, MAX_PRECISION = 16, MAX_UUIDS = 128;
constexpr uint32_t DEFAULT_CIELAB = 0x44454600, CUSTOM_CIELAB = 0;

uint32_t be(const uint8_t *p, uint32_t n) {
    uint32_t v = 0;
    for (uint32_t i = 0; i < n; ++i) v = (v << 8) | p[i];
    return v;
}
uint64_t be64(const uint8_t *p) { return ((uint64_t)be(p, 4) << 32) | be(p + 4, 4); }

struct Reader {
    const uint8_t *file;
    size_t len;
    Jp2Boxes &b;
    std::string &err;
    uint32_t state = 0;
    uint32_t nuuid = 0;

    bool fail(const char *m) { err = m; return false; }

    // jp2_read_ihdr (:547-633)
    bool ihdr(const uint8_t *p, uint32_t n) {
        if (b.have_ihdr) return true;  // a second one is ignored
        if (n != 14) return fail("JP2: bad image header box (bad size)");
        b.h = be(p, 4);
        b.w = be(p + 4, 4);
        b.numcomps = be(p + 8, 2);
        if (b.numcomps == 0 || b.numcomps > MAX_NUM_COMPONENTS) return fail("JP2: ihdr component count out of range");
        b.have_ihdr = true;  // (jp2->comps allocated: later ihdr boxes are ignored, even if this one fails below)
        b.bpcc.assign(b.numcomps, 0);
        b.bpc = p[10];
        if (b.bpc != 0xFF && (b.bpc & 0x7F) > MAX_PRECISION - 1) return fail("JP2: ihdr bpc not supported");
        b.C = p[11];
        b.UnkC = p[12];
        if (b.UnkC > 1) return fail("JP2: ihdr UnkC does not conform");
        b.IPR = p[13];
        if (b.IPR > 1) return fail("JP2: ihdr IPR does not conform");
        return true;
    }
    // jp2_read_bpcc (:999-1025); misplaced before any ihdr it compares with 0 components
    bool bpcc(const uint8_t *p, uint32_t n) {
        if (n != b.numcomps) return fail("JP2: bad bpcc box (bad size)");
        for (uint32_t i = 0; i < n; ++i) b.bpcc[i] = p[i];
        return true;
    }
    // jp2_read_colr (:1719-1826)
    bool colr(const uint8_t *p, uint32_t n) {
        if (n < 3) return fail("JP2: bad colr box (bad size)");
        if (b.have_colr) return true;  // every colour specification box after the first is ignored
        b.meth = p[0];
        b.precedence = p[1];
        b.approx = p[2];
        if (b.meth == 1) {
            if (n < 7) return fail("JP2: bad colr box (bad size)");
            b.enumcs = be(p + 3, 4);
            if (b.enumcs == 14) {  // CIELab: the block grk_image::icc_profile_buf carries with length 0
                b.ncielab = n == 35 ? 9 : 2;
                b.cielab[0] = 14;
                b.cielab[1] = DEFAULT_CIELAB;
                if (n == 35) {
                    b.cielab[1] = CUSTOM_CIELAB;
                    for (uint32_t i = 0; i < 7; ++i) b.cielab[2 + i] = be(p + 7 + 4 * i, 4);  // rl ol ra oa rb ob il
                }
            }
            b.have_colr = true;
        } else if (b.meth == 2) {
            if (n == 3) return fail("JP2: ICC profile buffer length equals zero");
            b.icc_off = (uint64_t)(p + 3 - file);
            b.icc_len = n - 3;
            b.have_colr = true;
        }  // METH > 2: the whole box is ignored (meth stays read, as in the reference)
        return true;
    }
    // jp2_read_pclr (:1409-1509)
    bool pclr(const uint8_t *p, uint32_t n) {
        if (b.have_pclr) return fail("JP2: a second pclr box");
        if (n < 3) return fail("JP2: pclr box too short");
        const uint32_t ne = be(p, 2);
        if (ne == 0 || ne > 1024) return fail("JP2: invalid pclr box: number of entries");
        const uint32_t npc = p[2];
        if (npc == 0) return fail("JP2: invalid pclr box: 0 palette columns");
        if (n < 3 + npc) return fail("JP2: pclr box too short");
        b.have_pclr = true;
        b.have_cmap = false;
        b.ne = ne;
        b.npc = npc;
        b.pal_size.resize(npc);
        b.pal_sign.resize(npc);
        b.entries.assign((size_t)ne * npc, 0);
        for (uint32_t i = 0; i < npc; ++i) {
            b.pal_size[i] = (uint8_t)((p[3 + i] & 0x7f) + 1);
            b.pal_sign[i] = (p[3 + i] & 0x80) ? 1 : 0;
        }
        uint32_t at = 3 + npc;
        for (uint32_t j = 0; j < ne; ++j)
            for (uint32_t i = 0; i < npc; ++i) {
                uint32_t nb = (uint32_t)(b.pal_size[i] + 7) >> 3;
                if (nb > 4) nb = 4;
                if (n < at + nb) return fail("JP2: pclr box too short for its entries");
                b.entries[(size_t)j * npc + i] = be(p + at, nb);
                at += nb;
            }
        return true;
    }
    // jp2_read_cmap (:1511-1562)
    bool cmap(const uint8_t *p, uint32_t n) {
        if (!b.have_pclr) return fail("JP2: need a pclr box before the cmap box");
        if (b.have_cmap) return fail("JP2: only one cmap box is allowed");
        if (n < b.npc * 4) return fail("JP2: insufficient data for cmap box");
        b.cmap.resize(b.npc);
        for (uint32_t i = 0; i < b.npc; ++i)
            b.cmap[i] = {(uint16_t)be(p + 4 * i, 2), p[4 * i + 2], p[4 * i + 3]};
        b.have_cmap = true;
        return true;
    }
    // jp2_read_cdef (:1625-1717)
    bool cdef(const uint8_t *p, uint32_t n) {
        if (b.have_cdef) return fail("JP2: a second cdef box");
        if (n < 2) return fail("JP2: cdef box: insufficient data");
        const uint32_t N = be(p, 2);
        if (N == 0) return fail("JP2: cdef box: number of channel descriptions is zero");
        if (n < 2 + N * 6) return fail("JP2: cdef box: insufficient data");
        b.cdef.resize(N);
        b.have_cdef = true;
        for (uint32_t i = 0; i < N; ++i)
            b.cdef[i] = {(uint16_t)be(p + 2 + 6 * i, 2), (uint16_t)be(p + 4 + 6 * i, 2), (uint16_t)be(p + 6 + 6 * i, 2)};
        for (uint32_t i = 0; i < N; ++i)
            for (uint32_t j = 0; j < N; ++j) {
                if (i != j && b.cdef[i].cn == b.cdef[j].cn && b.cdef[i].typ != b.cdef[j].typ)
                    return fail("JP2: cdef box: one channel described with differing types");
            }
        for (uint32_t i = 0; i < N; ++i)
            for (uint32_t j = 0; j < N; ++j) {
                if (i != j && b.cdef[i].cn != b.cdef[j].cn && b.cdef[i].typ == b.cdef[j].typ &&
                    b.cdef[i].asoc == b.cdef[j].asoc)
                    return fail("JP2: cdef box: two channels share a type / association pair");
            }
        return true;
    }
    // jp2_read_res (:804-847): its structure decides acceptance, its values are not kept
    bool res(const uint8_t *p, uint32_t n) {
        const uint32_t nb = n / 18;
        if (nb == 0 || nb > 2 || n % 18) return fail("JP2: bad resolution box (bad size)");
        for (uint32_t i = 0; i < nb; ++i) {
            if (be(p + 18 * i, 4) != 18) return fail("JP2: bad resolution sub-box size");
            const uint32_t id = be(p + 18 * i + 4, 4);
            if (id != BOX_RESC && id != BOX_RESD) return fail("JP2: unknown resolution sub-box");
        }
        return true;
    }
    bool img_box(uint32_t type, const uint8_t *p, uint32_t n, bool &known) {
        known = true;
        switch (type) {
            case BOX_IHDR: return ihdr(p, n);
            case BOX_COLR: return colr(p, n);
            case BOX_BPCC: return bpcc(p, n);
            case BOX_PCLR: return pclr(p, n);
            case BOX_CMAP: return cmap(p, n);
            case BOX_CDEF: return cdef(p, n);
            case BOX_RES: return res(p, n);
            default: known = false; return true;
        }
    }
    static bool is_img_box(uint32_t t) {
        return t == BOX_IHDR || t == BOX_COLR || t == BOX_BPCC || t == BOX_PCLR || t == BOX_CMAP || t == BOX_CDEF ||
               t == BOX_RES;
    }
    // jp2_read_jp2h (:2854-2915) with jp2_read_box (:2917-2968)
    bool jp2h(const uint8_t *p, uint32_t n) {
        if ((state & ST_FILE_TYPE) != ST_FILE_TYPE) return fail("JP2: jp2h box before the file type box");
        int64_t left = (int64_t)n;
        bool has_ihdr = false;
        while (left) {
            if (left < 8) return fail("JP2: box of less than 8 bytes inside jp2h");
            uint64_t blen = be(p, 4);
            const uint32_t type = be(p + 4, 4);
            uint32_t hdr = 8;
            if (blen == 1) {
                if (left < 16) return fail("JP2: XL box of less than 16 bytes inside jp2h");
                blen = be64(p + 8);
                hdr = 16;
                if (blen == 0) return fail("JP2: box of undefined size inside jp2h");
            } else if (blen == 0) {
                return fail("JP2: box of undefined size inside jp2h");
            }
            if (blen < hdr) return fail("JP2: box length below its header inside jp2h");
            if (blen > (uint64_t)left) return fail("JP2: box length past the end of jp2h");
            const uint32_t dsz = (uint32_t)(blen - hdr);
            bool known;
            if (!img_box(type, p + hdr, dsz, known)) return false;
            if (type == BOX_IHDR) has_ihdr = true;
            p += blen;
            left -= (int64_t)blen;
        }
        if (!has_ihdr) return fail("JP2: no ihdr box inside jp2h");
        state |= ST_HEADER;
        return true;
    }
    // jp2_read_header_procedure (:2493-2631) with jp2_read_box_hdr (:479-520)
    Jp2Status run() {
        size_t pos = 0;
        for (;;) {
            if (len - pos < 8) break;  // end of the file: no codestream box
            uint64_t blen = be(file + pos, 4);
            const uint32_t type = be(file + pos + 4, 4);
            uint32_t nread = 8;
            pos += 8;
            if (blen == 0) {
                blen = (uint64_t)(len - pos) + 8;  // the last box
            } else {
                if (blen == 1) {
                    if (len - pos < 8) break;
                    blen = be64(file + pos);
                    pos += 8;
                    nread = 16;
                }
                if (blen < nread) { err = "JP2: invalid box size"; return JP2_CORRUPT; }
            }
            if (type == BOX_JP2C) {
                if (!(state & ST_HEADER)) { err = "JP2: codestream box before the JP2 header box"; return JP2_CORRUPT; }
                b.cs_off = pos;
                b.cs_len = std::min<uint64_t>(blen - nread, len - pos);
                return JP2_OK;
            }
            const bool top = type == BOX_JP || type == BOX_FTYP || type == BOX_JP2H || type == BOX_XML || type == BOX_UUID;
            const bool misplaced = !top && is_img_box(type);
            const uint32_t dsz = (uint32_t)(blen - nread);
            if (misplaced && !(state & ST_HEADER)) {  // ignored until the header box was read
                state |= ST_UNKNOWN;
                if (dsz > len - pos) { err = "JP2: box length past the end of the file"; return JP2_CORRUPT; }
                pos += dsz;
                continue;
            }
            if (top || misplaced) {
                if (dsz > len - pos) { err = "JP2: box length past the end of the file"; return JP2_CORRUPT; }
                const uint8_t *p = file + pos;
                bool ok = true, known;
                if (misplaced) {
                    ok = img_box(type, p, dsz, known);
                } else if (type == BOX_JP) {  // jp2_read_jp (:2735-2765)
                    if (state != 0) ok = fail("JP2: the signature box must be the first box");
                    else if (dsz != 4) ok = fail("JP2: bad signature box size");
                    else if (be(p, 4) != 0x0d0a870a) ok = fail("JP2: bad signature");
                    else state |= ST_SIGNATURE;
                } else if (type == BOX_FTYP) {  // jp2_read_ftyp (:2777-2827)
                    if (state != ST_SIGNATURE) ok = fail("JP2: the ftyp box must be the second box");
                    else if (dsz < 8 || ((dsz - 8) & 3)) ok = fail("JP2: bad ftyp box size");
                    else state |= ST_FILE_TYPE;
                } else if (type == BOX_JP2H) {
                    ok = jp2h(p, dsz);
                } else if (type == BOX_XML) {  // jp2_read_xml (:719-731): contents not kept
                    if (!dsz) ok = fail("JP2: empty xml box");
                } else {  // jp2_read_uuid (:738-760): contents not kept
                    if (dsz < 16) ok = fail("JP2: uuid box too short");
                    else if (nuuid == MAX_UUIDS) ok = fail("JP2: too many uuid boxes");
                    else ++nuuid;
                }
                if (!ok) return JP2_CORRUPT;
                pos += dsz;
            } else {
                if (!(state & ST_SIGNATURE)) { err = "JP2: first box must be the signature box"; return JP2_CORRUPT; }
                if (!(state & ST_FILE_TYPE)) { err = "JP2: second box must be the file type box"; return JP2_CORRUPT; }
                state |= ST_UNKNOWN;
                if (dsz > len - pos) break;  // (the skip fails; every state bit is set, so the walk just ends)
                pos += dsz;
            }
        }
        err = "JP2: no codestream box";
        return JP2_CORRUPT;
    }
};

}  // namespace

Jp2Status jp2_read_boxes(const uint8_t *file, size_t len, Jp2Boxes &b, std::string &err) {
    b = Jp2Boxes{};
    Reader r{file, len, b, err};
    const Jp2Status st = r.run();
    if (st == JP2_OK && b.cs_len >= (1ull << 32)) {
        err = "JP2: codestream box of 4 GiB or more is not supported";
        return JP2_UNSUPPORTED;
    }
    return st;
}

Jp2Status jp2_resolve_channels(Jp2Boxes &b, uint32_t numcomps, const uint32_t *prec, const int32_t *sgnd,
                               const uint32_t *dx, const uint32_t *dy, uint32_t max_channels, Jp2Channels &out,
                               std::string &err) {
    out = Jp2Channels{};
    auto corrupt = [&](const char *m) { err = m; return JP2_CORRUPT; };
    auto unsupported = [&](const char *m) { err = m; return JP2_UNSUPPORTED; };
    const bool pal = b.have_pclr && b.have_cmap;
    // jp2_check_color (:1167-1299)
    if (b.have_cdef) {
        uint32_t nch = pal ? b.npc : numcomps;
        for (const Jp2Cdef &d : b.cdef) {
            if (d.cn >= nch) return corrupt("JP2: cdef channel index out of range");
            if (d.asoc == 65535) continue;
            if (d.asoc > 0 && (uint32_t)(d.asoc - 1) >= nch) return corrupt("JP2: cdef association out of range");
        }
        for (; nch > 0; --nch) {
            bool found = false;
            for (const Jp2Cdef &d : b.cdef) found = found || d.cn == nch - 1;
            if (!found) return corrupt("JP2: incomplete channel definitions");
        }
    }
    if (pal) {
        const uint32_t n = b.npc;
        for (uint32_t i = 0; i < n; ++i)
            if (b.cmap[i].cmp >= numcomps) return corrupt("JP2: cmap component index out of range");
        std::vector<uint8_t> used(n, 0);
        for (uint32_t i = 0; i < n; ++i) {
            const Jp2Cmap &m = b.cmap[i];
            if (m.mtyp != 0 && m.mtyp != 1) return corrupt("JP2: unexpected cmap MTYP value");
            if (m.pcol >= n) return corrupt("JP2: cmap palette column out of range");
            if (used[m.pcol] && m.mtyp == 1) return corrupt("JP2: palette column mapped twice");
            if (m.mtyp == 0 && m.pcol != 0) return corrupt("JP2: direct use with a palette column");
            used[m.pcol] = 1;
        }
        for (uint32_t i = 0; i < n; ++i)
            if (!used[i] && b.cmap[i].mtyp != 0) return corrupt("JP2: palette column without a mapping");
        if (numcomps == 1) {  // "weird cmap" (:1272-1290): every column mapped in order from the one component
            bool all = true;
            for (uint32_t i = 0; i < n; ++i) all = all && used[i];
            if (!all)
                for (uint32_t i = 0; i < n; ++i) { b.cmap[i].mtyp = 1; b.cmap[i].pcol = (uint8_t)i; }
        }
    }
    // the colour space (jp2_decode :1843-1878)
    switch (b.enumcs) {
        case 12: out.colour_space = JP2_CS_CMYK; break;
        case 14:
            if (!b.ncielab) return corrupt("JP2: CIELab image without its parameter block");
            out.colour_space = b.cielab[1] == DEFAULT_CIELAB ? JP2_CS_DEFAULT_CIE : JP2_CS_CUSTOM_CIE;
            break;
        case 16: out.colour_space = JP2_CS_SRGB; break;
        case 17: out.colour_space = JP2_CS_GRAY; break;
        case 18: out.colour_space = JP2_CS_SYCC; break;
        case 24: out.colour_space = JP2_CS_EYCC; break;
        default: out.colour_space = JP2_CS_UNKNOWN; break;
    }
    if (b.meth == 2 && b.icc_len) out.colour_space = JP2_CS_ICC;
    // jp2_apply_pclr (:1301-1407) on the component descriptions
    std::vector<Jp2Channel> ch;
    if (pal) {
        if (b.npc > max_channels) return unsupported("JP2: palette with more columns than this decoder has channels");
        for (uint32_t i = 0; i < b.npc; ++i) {
            if (b.pal_size[i] > 16) return unsupported("JP2: palette channel wider than 16 bits");
            if (b.pal_sign[i]) return unsupported("JP2: signed palette channel");
            if (b.cmap[i].mtyp == 1 && b.cmap[i].pcol != i)
                return unsupported("JP2: cmap palette column other than the channel's own index");
            const uint32_t k = b.cmap[i].cmp;
            if (dx[k] != 1 || dy[k] != 1) return unsupported("JP2: cmap over a subsampled component");
        }
        for (uint32_t i = 0; i < b.npc; ++i) {
            Jp2Channel c;
            c.comp = b.cmap[i].cmp;
            c.pcol = b.cmap[i].mtyp == 1 ? (int32_t)b.cmap[i].pcol : -1;
            c.prec = b.pal_size[i];
            c.sgnd = b.pal_sign[i];
            c.dx = dx[c.comp];
            c.dy = dy[c.comp];
            ch.push_back(c);
        }
        out.palette = true;
    } else {
        for (uint32_t k = 0; k < numcomps; ++k) {
            Jp2Channel c;
            c.comp = k;
            c.prec = prec[k];
            c.sgnd = sgnd[k];
            c.dx = dx[k];
            c.dy = dy[k];
            ch.push_back(c);
        }
    }
    // jp2_apply_cdef (:1564-1623)
    if (b.have_cdef) {
        std::vector<Jp2Cdef> info = b.cdef;
        const uint32_t n = (uint32_t)info.size(), nch = (uint32_t)ch.size();
        for (uint32_t i = 0; i < n; ++i) {
            const uint16_t asoc = info[i].asoc, cn = info[i].cn;
            if (cn >= nch) continue;
            if (asoc == 0 || asoc == 65535) { ch[cn].alpha = info[i].typ; continue; }
            const uint16_t acn = (uint16_t)(asoc - 1);
            if (acn >= nch) continue;
            if (cn != acn && info[i].typ == 0) {
                std::swap(ch[cn], ch[acn]);
                for (uint32_t j = i + 1; j < n; ++j) {
                    if (info[j].cn == cn) info[j].cn = acn;
                    else if (info[j].cn == acn) info[j].cn = cn;
                }
            }
            ch[cn].alpha = info[i].typ;
        }
    }
    out.mapped = out.palette;
    for (uint32_t i = 0; i < ch.size(); ++i) out.mapped = out.mapped || ch[i].comp != i;
    out.ch = ch;
    return JP2_OK;
}

// ---------------------------------------------------------------------------
// writer
// ---------------------------------------------------------------------------
namespace {
void put(std::vector<uint8_t> &o, uint32_t v, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) o.push_back((uint8_t)(v >> (8 * (n - 1 - i))));
}
}  // namespace

bool jp2_write_boxes(const Jp2WriteParams &p, std::vector<uint8_t> &o, std::string &err) {
    o.clear();
    if (p.numcomps < 1 || p.numcomps > 16) { err = "JP2: 1 .. 16 components"; return false; }
    for (uint32_t i = 0; i < p.numcomps; ++i)
        if (p.prec[i] < 1 || p.prec[i] > 38) { err = "JP2: component precision out of range"; return false; }
    // jp2_setup_encoder (:2153-2387)
    const uint32_t depth0 = p.prec[0] - 1;
    uint32_t bpc = depth0 + ((p.sgnd[0] ? 1u : 0u) << 7);
    for (uint32_t i = 1; i < p.numcomps; ++i)
        if (p.prec[i] - 1 != depth0) bpc = 255;
    uint32_t meth = 1, enumcs = 0;
    if (p.colour_space == JP2_CS_ICC) {
        meth = 2;
        if (!p.icc || !p.icc_len) { err = "JP2: the ICC colour space needs a profile"; return false; }
    } else if (p.colour_space == JP2_CS_CMYK) enumcs = 12;
    else if (p.colour_space == JP2_CS_DEFAULT_CIE) enumcs = 14;
    else if (p.colour_space == JP2_CS_SRGB) enumcs = 16;
    else if (p.colour_space == JP2_CS_GRAY) enumcs = 17;
    else if (p.colour_space == JP2_CS_SYCC) enumcs = 18;
    // the channel definition box: exactly one alpha channel, behind the colour channels (:2264-2343)
    uint32_t alpha_count = 0, alpha_channel = 0, colour_channels = 0;
    for (uint32_t i = 0; i < p.numcomps; ++i)
        if (p.alpha[i]) { ++alpha_count; alpha_channel = i; }
    if (alpha_count == 1) {
        switch (enumcs) {
            case 16: case 18: colour_channels = 3; break;
            case 17: colour_channels = 1; break;
            default:
                if (p.numcomps > 1) colour_channels = p.numcomps - 1;
                else alpha_count = 0;
                break;
        }
        if (alpha_count && (p.numcomps < colour_channels + 1 || alpha_channel < colour_channels)) alpha_count = 0;
    }
    const bool cdef = alpha_count == 1;
    // jp2_write_jp, jp2_write_ftyp
    put(o, 12, 4); put(o, BOX_JP, 4); put(o, 0x0d0a870a, 4);
    put(o, 20, 4); put(o, BOX_FTYP, 4); put(o, 0x6a703220, 4); put(o, 0, 4); put(o, 0x6a703220, 4);
    // jp2_write_jp2h (:1922-2011): ihdr, bpcc, colr, cdef
    const uint32_t colr_size = 11 + (meth == 1 ? 4 : p.icc_len);
    const uint32_t jp2h_size = 8 + 22 + (bpc == 255 ? 8 + p.numcomps : 0) + colr_size + (cdef ? 10 + 6 * p.numcomps : 0);
    put(o, jp2h_size, 4); put(o, BOX_JP2H, 4);
    put(o, 22, 4); put(o, BOX_IHDR, 4); put(o, p.h, 4); put(o, p.w, 4); put(o, p.numcomps, 2);
    put(o, bpc, 1); put(o, 7, 1); put(o, 0, 1); put(o, 0, 1);
    if (bpc == 255) {
        put(o, 8 + p.numcomps, 4); put(o, BOX_BPCC, 4);
        for (uint32_t i = 0; i < p.numcomps; ++i) put(o, p.prec[i] - 1 + ((p.sgnd[i] ? 1u : 0u) << 7), 1);
    }
    put(o, colr_size, 4); put(o, BOX_COLR, 4); put(o, meth, 1); put(o, 0, 1); put(o, 0, 1);
    if (meth == 1) put(o, enumcs, 4);
    else o.insert(o.end(), p.icc, p.icc + p.icc_len);
    if (cdef) {
        put(o, 10 + 6 * p.numcomps, 4); put(o, BOX_CDEF, 4); put(o, p.numcomps, 2);
        for (uint32_t i = 0; i < p.numcomps; ++i) {
            put(o, i, 2);
            if (i < colour_channels) { put(o, 0, 2); put(o, i + 1, 2); }
            else if (p.alpha[i]) { put(o, p.alpha[i], 2); put(o, 0, 2); }
            else { put(o, 65535, 2); put(o, 65535, 2); }
        }
    }
    // jp2_write_jp2c (:2075-2116): LBox for the caller
    put(o, 0, 4); put(o, BOX_JP2C, 4);
    return true;
}

}  // namespace grkgpu
