// codec.cpp -- tile pipeline (the reference's TileProcessor, "tcd") turned into
// a HIP dispatch layer, plus the extern "C" API of include/grk_mi355x.h.
//
// Encode (TileProcessor::encode_tile, TileProcessor.cpp:951-1025):
//   H2D planes (if host) -> per tile: DC shift + MCT kernel -> per component
//   DWT levels -> ONE T1 launch over every code-block of every tile ->
//   D2H per-block results -> gather kernel packs block bytes -> D2H ->
//   host Tier-2 + headers.
// Decode (TileProcessor::decode_tile, TileProcessor.cpp:1069-1179):
//   host header + Tier-2 parse -> H2D codestream -> ONE T1 decode launch ->
//   per tile/component inverse DWT levels -> inverse MCT + DC shift.
#include <assert.h>
#include <float.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <array>
#include <chrono>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/grk_mi355x.h"
#include "codestream.h"
#include "grk_device.h"
#include "host_pool.h"
#include "jp2.h"
#include "t2.h"

using namespace grkgpu;

static thread_local std::string g_err;
static int set_err(int code, const std::string &msg) { g_err = msg; return code; }
namespace grkgpu {
int set_error(int code, const std::string &msg) { return set_err(code, msg); }  // multi.cpp
}

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return set_err(GRKGPU_EHIP, std::string(#expr ": ") + hipGetErrorString(e_));    \
    } while (0)

namespace {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) hipFree(p);
        p = nullptr; cap = 0;
        size_t nb = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, nb);
        if (e == hipSuccess) cap = nb;
        return e;
    }
    template <typename T> T *as() const { return (T *)p; }
    ~DevBuf() { if (p) hipFree(p); }
};

struct HostBuf {  // pinned host staging
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) hipHostFree(p);
        p = nullptr; cap = 0;
        size_t nb = bytes + bytes / 8 + 256;
        hipError_t e = hipHostMalloc(&p, nb, hipHostMallocDefault);
        if (e == hipSuccess) cap = nb;
        return e;
    }
    template <typename T> T *as() const { return (T *)p; }
    ~HostBuf() { if (p) hipHostFree(p); }
};

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

// The context's grow-only buffers.  None is ever cleared between calls (the
// read-before-write table in DESIGN.md says why each call may rely on that),
// so grkgpu_debug_fill must reach every one: a new buffer goes into one of
// these two structs -- never into grkgpu_ctx itself -- and into the matching
// list of ctx_buffers() below, whose static_asserts count the members.
struct CtxDevBufs {
    DevBuf img, work, coef, ll, scratch, mqout, blocks, results, gather, packed, cs, sym, symoff, dwtjobs, ubuf, segs;
    DevBuf dwtjobs53;  // decode: the 5/3 tile-components' job table when 9/7 ones share the call
    DevBuf t1order;    // encode: the MQ coder's work order (keys, permutation, bucket counters)
    // encode with rate control: the pass records formed on the device
    // (launch_pass_records): per block its distortion factor and record slots
    // (in), its summary and records (out)
    DevBuf pinfo, precs;
    DevBuf pal;  // JP2 decode: the palette table, uploaded again by every call that looks up
    DevBuf storejobs;  // batch decode: the StoreJob table and its first-workgroup arrays, uploaded by every batch
    DevBuf loadjobs;   // batch encode: the LoadJob table and its first-workgroup arrays, uploaded by every batch
};
struct CtxHostBufs {
    HostBuf h_results, h_packed, h_gather, h_blocks, h_out, h_symoff, h_dwtjobs, h_segs;
    HostBuf h_pinfo, h_psum, h_precs;
    HostBuf h_dwtjobs53;
    // grkgpu_encode_blocks output (valid until the next call on the context)
    HostBuf h_slab;
    // batch decode: the items' codestreams packed for one H2D, and the store-job table's staging
    HostBuf h_cs, h_storejobs;
    // batch encode: the load-job table's staging, and the items' host samples packed for one H2D
    HostBuf h_loadjobs, h_img;
};

struct grkgpu_ctx : CtxDevBufs, CtxHostBufs {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // encode: the pass records of the last call, kept so that a frame of the
    // same size does not zero ~20 MB again before overwriting every record
    // (kept host records like this one are dirtied by grkgpu_debug_fill too)
    std::vector<EncPass> enc_passes;
    hipEvent_t ev[8] = {};
    grkgpu_stats stats = {};
    // grkgpu_encode_blocks output (valid until the next call on the context)
    std::vector<grkgpu_block_info> bexp;
    struct CoefRec { uint32_t tileno, compno, w, h; uint64_t off; };  // coefficient arena of each tile-component
    std::vector<CoefRec> bexp_coef;
    std::vector<uint32_t> bexp_rate;
    std::vector<double> bexp_dist;
    // per-launch DWT timing (grkgpu_set_launch_timing): a start / end event per
    // launch of the last forward DWT, read after the call's final sync
    bool launch_timing = false;
    std::vector<hipEvent_t> lev;
    std::vector<grkgpu_launch_time> ltimes;
    std::vector<std::pair<uint32_t, uint32_t>> lidx;  // per logged launch: its start / end event in lev
    // guards h_out and out_spare against grkgpu_give_output from another thread
    std::mutex out_mu;
    // output buffers given back while h_out held a newer one (a caller keeping
    // several views alive): the next compress whose h_out was taken reuses one
    // instead of pinning a fresh buffer; at most OUT_SPARE, the largest kept
    std::vector<std::pair<void *, size_t>> out_spare;
};
static constexpr size_t OUT_SPARE = 4;

// Device check, cached per device index (hipGetDeviceProperties is slow and
// the stage entry points run it per call).  device < 0: the calling thread's
// current HIP device (the stage entry points work on the caller's device).
static int check_device(int device) {
    static std::mutex mu;
    static int ok[64] = {};  // 0 unknown, 1 gfx950, -1 unusable
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return set_err(GRKGPU_ENODEV, "no HIP device available (MI355X / gfx950 required; no CPU fallback)");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return set_err(GRKGPU_ENODEV, "hipGetDevice failed");
    if (device < 0 || device >= n) return set_err(GRKGPU_ENODEV, "device index out of range");
    std::lock_guard<std::mutex> lk(mu);
    if (device < 64 && ok[device] == 1) return GRKGPU_OK;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return set_err(GRKGPU_ENODEV, "hipGetDeviceProperties failed");
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
        if (device < 64) ok[device] = -1;
        return set_err(GRKGPU_ENODEV, std::string("unsupported device arch ") + prop.gcnArchName + " (gfx950 required)");
    }
    if (device < 64) ok[device] = 1;
    return GRKGPU_OK;
}

extern "C" {

const char *grkgpu_version(void) { return "grk-mi355x 0.1.0 (Grok 5.1.0 codestream-compatible)"; }
const char *grkgpu_last_error(void) { return g_err.c_str(); }

int grkgpu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int grkgpu_set_mct(grkgpu_cparams *p, const float *matrix, const int32_t *dc_shift, uint32_t n) {
    if (!p || !matrix || !dc_shift || !n || n > GRKGPU_MAX_COMPS) return set_err(GRKGPU_EINVAL, "custom MCT: 1..16 components");
    p->rsiz = (p->rsiz & RSIZ_PART2) ? (p->rsiz | RSIZ_EXT_MCT) : (RSIZ_PART2 | RSIZ_EXT_MCT);  // grok.cpp:612-617
    p->irreversible = 1;
    p->tcp_mct = 2;
    p->mct_ncomp = n;
    memcpy(p->mct_matrix, matrix, sizeof(float) * n * n);
    memcpy(p->mct_dc_shift, dc_shift, sizeof(int32_t) * n);
    return GRKGPU_OK;
}

// grk_set_default_encoder_parameters (grok.cpp) + grk_compress's defaults
void grkgpu_default_cparams(grkgpu_cparams *p) {
    memset(p, 0, sizeof(*p));
    p->numresolution = 6;
    p->cblockw_init = 64;
    p->cblockh_init = 64;
    p->irreversible = 0;
    p->tcp_mct = -1;
    p->prog_order = GRKGPU_LRCP;
    p->tcp_numlayers = 0;  // -> one lossless layer (disto_alloc set then, grk_compress.cpp:1579-1583)
}

int grkgpu_create(int device, grkgpu_ctx **out) {
    int rc = check_device(device);
    if (rc) return rc;
    HIPCHK(hipSetDevice(device));
    auto *c = new grkgpu_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return set_err(GRKGPU_EHIP, "hipStreamCreate failed");
    }
    c->own_stream = true;
    for (auto &e : c->ev) hipEventCreate(&e);
    *out = c;
    return GRKGPU_OK;
}

void grkgpu_destroy(grkgpu_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    for (auto &e : c->ev) if (e) hipEventDestroy(e);
    for (auto &e : c->lev) if (e) hipEventDestroy(e);
    if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
    for (auto &b : c->out_spare) hipHostFree(b.first);
    delete c;
}

int grkgpu_set_stream(grkgpu_ctx *c, void *stream) {
    if (!c) return set_err(GRKGPU_EINVAL, "null ctx");
    if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
    c->stream = (hipStream_t)stream;
    c->own_stream = false;
    return GRKGPU_OK;
}

}  // extern "C"

// Every buffer of CtxDevBufs / CtxHostBufs, for grkgpu_debug_fill.
namespace {
struct CtxBuffers {
    DevBuf *dev[23];
    HostBuf *host[17];
};
CtxBuffers ctx_buffers(grkgpu_ctx *c) {
    CtxBuffers b{{&c->img, &c->work, &c->coef, &c->ll, &c->scratch, &c->mqout, &c->blocks, &c->results, &c->gather,
                  &c->packed, &c->cs, &c->sym, &c->symoff, &c->dwtjobs, &c->ubuf, &c->segs, &c->dwtjobs53, &c->t1order,
                  &c->pinfo, &c->precs, &c->pal, &c->storejobs, &c->loadjobs},
                 {&c->h_results, &c->h_packed, &c->h_gather, &c->h_blocks, &c->h_out, &c->h_symoff, &c->h_dwtjobs,
                  &c->h_segs, &c->h_pinfo, &c->h_psum, &c->h_precs, &c->h_dwtjobs53, &c->h_slab, &c->h_cs,
                  &c->h_storejobs, &c->h_loadjobs, &c->h_img}};
    static_assert(sizeof(CtxDevBufs) == sizeof(b.dev) / sizeof(b.dev[0]) * sizeof(DevBuf),
                  "a DevBuf was added to CtxDevBufs: list it in ctx_buffers()");
    static_assert(sizeof(CtxHostBufs) == sizeof(b.host) / sizeof(b.host[0]) * sizeof(HostBuf),
                  "a HostBuf was added to CtxHostBufs: list it in ctx_buffers()");
    return b;
}
}  // namespace

extern "C" int grkgpu_debug_fill(grkgpu_ctx *c, int byte, size_t *filled) {
    if (!c) return set_err(GRKGPU_EINVAL, "null ctx");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int v = byte & 0xff;
    size_t n = 0;
    const CtxBuffers b = ctx_buffers(c);
    for (DevBuf *d : b.dev) {
        if (!d->p || !d->cap) continue;
        HIPCHK(hipMemsetAsync(d->p, v, d->cap, c->stream));
        n += d->cap;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    {
        // h_out and the spares given back are the context's; a buffer taken
        // with grkgpu_take_output is the caller's until it comes back
        std::lock_guard<std::mutex> lk(c->out_mu);
        for (HostBuf *h : b.host) {
            if (!h->p || !h->cap) continue;
            memset(h->p, v, h->cap);
            n += h->cap;
        }
        for (auto &sp : c->out_spare) {
            memset(sp.first, v, sp.second);
            n += sp.second;
        }
    }
    // kept host records: the pass records keep their count (the encode reuses
    // them without clearing), everything a getter hands out becomes empty
    if (!c->enc_passes.empty()) {
        memset((void *)c->enc_passes.data(), v, c->enc_passes.size() * sizeof(EncPass));
        n += c->enc_passes.size() * sizeof(EncPass);
    }
    c->bexp.clear();
    c->bexp_coef.clear();
    c->bexp_rate.clear();
    c->bexp_dist.clear();
    c->ltimes.clear();
    c->lidx.clear();
    if (filled) *filled = n;
    return GRKGPU_OK;
}

namespace grkgpu {
static DwtOptions g_dwt_opts;
const DwtOptions &dwt_options() { return g_dwt_opts; }

// Codec calls in progress in this process.  A call that has the GPU to itself
// (a lone frame: grk_decompress of one image) cannot fill the chip with its
// T1 lanes packed 64 blocks to a wavefront (24,669 blocks of an 8K frame =
// 386 wavefronts for 1,024 SIMDs), so it spreads them (lone_bpw) and orders
// them by work; concurrent calls (frame batches) keep full wavefronts.
static std::atomic<int> g_active_calls{0};
struct ActiveCall {
    ActiveCall() { g_active_calls.fetch_add(1); }
    ~ActiveCall() { g_active_calls.fetch_sub(1); }
};
// t1_lone forces the choice either way (the parity suite's handle on the batch kernels).
static bool lone_call() { return g_dwt_opts.t1_lone ? g_dwt_opts.t1_lone > 0 : g_active_calls.load() <= 1; }
}  // namespace grkgpu

extern "C" {

void grkgpu_get_dwt_options(grkgpu_dwt_options *out) {
    if (!out) return;
    out->fuse_level0 = g_dwt_opts.fuse_level0;
    out->f01_rows = g_dwt_opts.f01_rows;
    out->f01_min_samples = g_dwt_opts.f01_min_samples;
    out->f01_small_min_samples = g_dwt_opts.f01_small_min_samples;
    out->inv01 = g_dwt_opts.inv01;
    out->pair_group = g_dwt_opts.pair_group;
    out->inv01_min_samples = g_dwt_opts.inv01_min_samples;
    out->f64_lift = g_dwt_opts.f64_lift;
    out->t1_dec_sort = g_dwt_opts.t1_dec_sort;
    out->t1_dec_bpw = g_dwt_opts.t1_dec_bpw;
    out->mid_th = g_dwt_opts.mid_th;
    out->t1_enc_bpw = g_dwt_opts.t1_enc_bpw;
    out->t1_enc_sort = g_dwt_opts.t1_enc_sort;
    out->pair_kernel = g_dwt_opts.pair_kernel;
    out->pair_rows = g_dwt_opts.pair_rows;
    out->pair_waves = g_dwt_opts.pair_waves;
    out->pair_min_samples = g_dwt_opts.pair_min_samples;
    out->t1_lone = g_dwt_opts.t1_lone;
    out->pad_ = 0;
}

int grkgpu_set_dwt_options(const grkgpu_dwt_options *o) {
    if (!o) {
        g_dwt_opts = DwtOptions();
        return GRKGPU_OK;
    }
    if (o->fuse_level0 < -1 || o->fuse_level0 > 1) return set_err(GRKGPU_EINVAL, "fuse_level0 must be -1, 0 or 1");
    if (o->f01_rows != 0 && o->f01_rows != 2 && o->f01_rows != 4 && o->f01_rows != 6)
        return set_err(GRKGPU_EINVAL, "f01_rows must be 0, 2, 4 or 6");
    if (o->inv01 != 0 && o->inv01 != 2 && o->inv01 != 4) return set_err(GRKGPU_EINVAL, "inv01 must be 0, 2 or 4");
    if (o->pair_group < 0 || o->pair_group > 4096) return set_err(GRKGPU_EINVAL, "pair_group must be 0 .. 4096");
    if (o->f64_lift != 0 && o->f64_lift != 1) return set_err(GRKGPU_EINVAL, "f64_lift must be 0 or 1");
    if (o->t1_dec_sort < -1 || o->t1_dec_sort > 1) return set_err(GRKGPU_EINVAL, "t1_dec_sort must be -1, 0 or 1");
    if (o->t1_dec_bpw < 0 || o->t1_dec_bpw > 64 || (o->t1_dec_bpw & (o->t1_dec_bpw - 1)))
        return set_err(GRKGPU_EINVAL, "t1_dec_bpw must be 0 or a power of two <= 64");
    if (o->mid_th != 0 && o->mid_th != 8 && o->mid_th != 16 && o->mid_th != 24)
        return set_err(GRKGPU_EINVAL, "mid_th must be 0, 8, 16 or 24");
    if (o->t1_enc_bpw < 0 || o->t1_enc_bpw > 64 || (o->t1_enc_bpw & (o->t1_enc_bpw - 1)))
        return set_err(GRKGPU_EINVAL, "t1_enc_bpw must be 0 or a power of two <= 64");
    if (o->t1_enc_sort != 0 && o->t1_enc_sort != 1) return set_err(GRKGPU_EINVAL, "t1_enc_sort must be 0 or 1");
    if (o->pair_kernel < 0 || o->pair_kernel > 2) return set_err(GRKGPU_EINVAL, "pair_kernel must be 0, 1 or 2");
    if (o->pair_rows < 0 || o->pair_rows > 65536 || (o->pair_rows & 1))
        return set_err(GRKGPU_EINVAL, "pair_rows must be 0 or an even count <= 65536");
    if (o->pair_waves != 0 && o->pair_waves != 3 && o->pair_waves != 4)
        return set_err(GRKGPU_EINVAL, "pair_waves must be 0, 3 or 4");
    if (o->t1_lone < -1 || o->t1_lone > 1) return set_err(GRKGPU_EINVAL, "t1_lone must be -1, 0 or 1");
    g_dwt_opts.t1_lone = o->t1_lone;
    g_dwt_opts.pair_kernel = o->pair_kernel;
    g_dwt_opts.pair_rows = o->pair_rows;
    g_dwt_opts.pair_waves = o->pair_waves;
    g_dwt_opts.pair_min_samples = o->pair_min_samples;
    g_dwt_opts.t1_enc_sort = o->t1_enc_sort;
    g_dwt_opts.t1_enc_bpw = o->t1_enc_bpw;
    g_dwt_opts.f64_lift = o->f64_lift;
    g_dwt_opts.t1_dec_sort = o->t1_dec_sort;
    g_dwt_opts.t1_dec_bpw = o->t1_dec_bpw;
    g_dwt_opts.mid_th = o->mid_th;
    g_dwt_opts.inv01 = o->inv01;
    g_dwt_opts.pair_group = o->pair_group;
    g_dwt_opts.inv01_min_samples = o->inv01_min_samples;
    g_dwt_opts.fuse_level0 = o->fuse_level0;
    g_dwt_opts.f01_rows = o->f01_rows;
    g_dwt_opts.f01_min_samples = o->f01_min_samples;
    g_dwt_opts.f01_small_min_samples = o->f01_small_min_samples;
    return GRKGPU_OK;
}

int grkgpu_take_output(grkgpu_ctx *c, void **buf, size_t *cap) {
    if (!c || !buf || !cap) return set_err(GRKGPU_EINVAL, "null arg");
    std::lock_guard<std::mutex> lk(c->out_mu);
    *buf = c->h_out.p;
    *cap = c->h_out.cap;
    c->h_out.p = nullptr;
    c->h_out.cap = 0;
    return GRKGPU_OK;
}

int grkgpu_give_output(grkgpu_ctx *c, void *buf, size_t cap) {
    if (!buf) return GRKGPU_OK;
    if (!c) {
        hipHostFree(buf);
        return GRKGPU_OK;
    }
    std::lock_guard<std::mutex> lk(c->out_mu);
    if (cap > c->h_out.cap) std::swap(buf, c->h_out.p), std::swap(cap, c->h_out.cap);
    if (!buf) return GRKGPU_OK;
    if (c->out_spare.size() < OUT_SPARE) {
        c->out_spare.push_back({buf, cap});
        return GRKGPU_OK;
    }
    auto small = std::min_element(c->out_spare.begin(), c->out_spare.end(),
                                  [](const auto &a, const auto &b) { return a.second < b.second; });
    if (cap > small->second) std::swap(buf, small->first), std::swap(cap, small->second);
    hipHostFree(buf);
    return GRKGPU_OK;
}

void grkgpu_free_output(void *buf) {
    if (buf) hipHostFree(buf);
}

int grkgpu_set_launch_timing(grkgpu_ctx *c, int on) {
    if (!c) return set_err(GRKGPU_EINVAL, "null ctx");
    c->launch_timing = on != 0;
    c->ltimes.clear();
    c->lidx.clear();
    return GRKGPU_OK;
}

int grkgpu_get_launch_times(grkgpu_ctx *c, grkgpu_launch_time *out, uint32_t max, uint32_t *n) {
    if (!c || !n || (max && !out)) return set_err(GRKGPU_EINVAL, "null arg");
    *n = (uint32_t)c->ltimes.size();
    for (uint32_t i = 0; i < max && i < c->ltimes.size(); ++i) out[i] = c->ltimes[i];
    return GRKGPU_OK;
}

int grkgpu_get_stats(grkgpu_ctx *c, grkgpu_stats *out) {
    if (!c || !out) return set_err(GRKGPU_EINVAL, "null arg");
    *out = c->stats;
    return GRKGPU_OK;
}

void grkgpu_free(void *p) { free(p); }

// Per-block scratch of the T1 stage entry points (per record; the records are
// the block count rounded up to 64): encode -- the encoder's interleaved rows
// for 32 planes, then 32 symbol-stream slots; decode -- the block state, then
// the unstuffed-stream region of a segment of up to GRKGPU_T1_MAX_SEG bytes.
static uint32_t t1_stage_dec_words() { return t1_unstuff_region_words(GRKGPU_T1_MAX_SEG); }
size_t grkgpu_t1_scratch_bytes(void) {
    return std::max<size_t>(t1e_scratch_bytes(64, 32) / 64 + 32 * (size_t)sym_slot_bytes(64, 64),
                            sizeof(T1Scratch) + (size_t)t1_stage_dec_words() * 4);
}
size_t grkgpu_t1_enc_out_bytes(uint32_t w, uint32_t h, uint32_t cblk_sty) {
    if (w > 64 || h > 64) return 0;
    return t1_enc_slab_bytes(w, h, cblk_sty & 0x3Fu, T1_MAX_ENC_BPS);
}
size_t grkgpu_t1_scratch_bytes_n(uint32_t nblocks) {
    return (((size_t)nblocks + 63) & ~(size_t)63) * grkgpu_t1_scratch_bytes();
}

}  // extern "C"

// ---------------------------------------------------------------------------
// shared helpers
// ---------------------------------------------------------------------------
static bool cinema_compliant(const grkgpu_image_desc *img, uint32_t rsiz) {
    // J2KProfile::is_cinema_compliant (j2kprofile.cpp:1083-1135)
    if (img->numcomps != 3) return false;
    for (uint32_t k = 0; k < 3; ++k)
        if (img->prec[k] != 12 || img->sgnd[k]) return false;
    const uint32_t w = img->x1 - img->x0, h = img->y1 - img->y0;
    if (rsiz == GRKGPU_PROFILE_CINEMA_2K) return w <= 2048 && h <= 1080;
    return w <= 4096 && h <= 2160;
}

// J2KProfile::set_cinema_parameters (j2kprofile.cpp:941-1081)
static void set_cinema_parameters(grkgpu_cparams *p, const grkgpu_image_desc *img) {
    p->tile_size_on = 0;
    p->cp_tdx = p->cp_tdy = 1;
    p->tp_flag = 'C';
    p->tp_on = 1;
    p->cp_tx0 = p->cp_ty0 = 0;
    p->cblockw_init = p->cblockh_init = 32;
    p->irreversible = 1;
    if (p->tcp_numlayers > 1) {
        p->tcp_rates[0] = p->tcp_rates[p->tcp_numlayers - 1];
        p->tcp_numlayers = 1;
    }
    if (p->rsiz == GRKGPU_PROFILE_CINEMA_2K) {
        if (p->numresolution > 6) p->numresolution = 6;
    } else {
        if (p->numresolution < 2) p->numresolution = 1;
        else if (p->numresolution > 7) p->numresolution = 7;
    }
    p->csty |= GRKGPU_CSTY_PRT;
    p->res_spec = p->numresolution - 1;
    for (uint32_t i = 0; i < p->res_spec; i++) p->prcw_init[i] = p->prch_init[i] = 256;
    p->prog_order = GRKGPU_CPRL;
    if (p->rsiz == GRKGPU_PROFILE_CINEMA_4K) {  // initialise_4K_poc (j2kprofile.cpp:922-939)
        const uint32_t nr = p->numresolution;
        p->POC[0] = {1, 0, 0, 1, nr - 1, 3, GRKGPU_CPRL};
        p->POC[1] = {1, nr - 1, 0, 1, nr, 3, GRKGPU_CPRL};
        p->numpocs = 2;
    } else {
        p->numpocs = 0;
    }
    p->cp_disto_alloc = 1;
    const uint64_t kCs = 1302083u, kComp = 1041666u;  // GRK_CINEMA_24_CS / _COMP (grok.h:316-318)
    if (p->max_cs_size == 0 || p->max_cs_size > kCs) p->max_cs_size = kCs;
    if (p->max_comp_size == 0 || p->max_comp_size > kComp) p->max_comp_size = kComp;
    const double w = img->x1 - img->x0, h = img->y1 - img->y0;
    p->tcp_rates[0] = ((double)img->numcomps * w * h * img->prec[0]) / ((double)p->max_cs_size * 8 * 1 * 1);
}

// j2k_setup_encoder (j2k.cpp:1609-2050) with the grk_compress post-parse
// defaults (grk_compress.cpp:1579-1583 one lossless layer, :1997-1998 MCT)
// and the cinema profiles, for the options grkgpu_cparams carries.  Layer
// rates stay compression ratios here; update_rates converts them to bytes.
static int setup_params(const grkgpu_image_desc *img, const grkgpu_cparams *pin, CodingParams &cp) {
    if (!img || !pin) return set_err(GRKGPU_EINVAL, "null image/params");
    grkgpu_cparams P = *pin;  // the profiles rewrite the parameters, as the reference does
    grkgpu_cparams *p = &P;
    if (img->numcomps < 1 || img->numcomps > 16) return set_err(GRKGPU_EINVAL, "numcomps must be 1..16");
    if (img->x1 <= img->x0 || img->y1 <= img->y0) return set_err(GRKGPU_EINVAL, "empty image");
    for (uint32_t k = 0; k < img->numcomps; ++k)
        if (img->prec[k] < 1 || img->prec[k] > 16) return set_err(GRKGPU_EUNSUPPORTED, "precision must be 1..16");
    if (p->tcp_numlayers > 100) return set_err(GRKGPU_EINVAL, "at most 100 quality layers");
    // code-block mode switches (COD SPcod style, j2k.cpp j2k_setup_encoder):
    // BYPASS, RESET, TERMALL, VSC, PTERM, SEGSYM; not HT (0x40)
    if (p->cblk_sty & ~0x3Fu) return set_err(GRKGPU_EUNSUPPORTED, "HT code-block style not supported");
    cp.cblksty = p->cblk_sty;
    if (p->roi_shift) {  // j2k_setup_encoder (j2k.cpp:1997-2001)
        if (p->roi_compno < 0 || (uint32_t)p->roi_compno >= img->numcomps)
            return set_err(GRKGPU_EINVAL, "ROI component out of range");
        if (p->roi_shift > 255) return set_err(GRKGPU_EINVAL, "ROI shift must fit a byte");
        cp.roishift[p->roi_compno] = (uint8_t)p->roi_shift;
    }
    if (p->tcp_numlayers == 0) {
        p->tcp_rates[0] = 0;
        p->tcp_numlayers = 1;
        p->cp_disto_alloc = 1;
    }
    if (p->cp_disto_alloc && p->cp_fixed_quality) return set_err(GRKGPU_EINVAL, "-r and -q cannot be used together");
    {  // max codestream size vs layer rates (j2k.cpp:1663-1689)
        // component 0's plane size, divided by its subsampling once more (sic)
        const uint32_t dx0 = img->dx[0] ? img->dx[0] : 1, dy0 = img->dy[0] ? img->dy[0] : 1;
        const Rect c0 = comp_rect({img->x0, img->y0, img->x1, img->y1}, dx0, dy0);
        const double image_bytes =
            ((double)img->numcomps * c0.w() * c0.h() * img->prec[0]) / (8.0 * dx0 * dy0);
        const uint32_t L = p->tcp_numlayers;
        if (p->max_cs_size == 0) {
            if (p->tcp_rates[L - 1] > 0) p->max_cs_size = (uint64_t)floor(image_bytes / p->tcp_rates[L - 1]);
        } else {
            const double min_rate = image_bytes / (double)p->max_cs_size;
            for (uint32_t i = 0; i < L; i++)
                if (p->tcp_rates[i] < min_rate) p->tcp_rates[i] = min_rate;
        }
    }
    if (p->rsiz == GRKGPU_PROFILE_CINEMA_2K || p->rsiz == GRKGPU_PROFILE_CINEMA_4K) {
        if (cinema_compliant(img, p->rsiz)) set_cinema_parameters(p, img);
        else p->rsiz = 0;  // "Non-profile-3/4 codestream will be generated"
    } else if (p->rsiz & RSIZ_PART2) {  // j2k.cpp:1720-1731: Part 2 with the MCT extension only
        if (p->rsiz != (RSIZ_PART2 | RSIZ_EXT_MCT)) p->rsiz = 0;
    } else if (p->rsiz != 0) {
        return set_err(GRKGPU_EUNSUPPORTED, "only the 2K / 4K digital cinema profiles and Part-2 MCT are supported");
    }
    if (p->numresolution < 1 || p->numresolution > 33) return set_err(GRKGPU_EINVAL, "numresolution must be 1..33");
    auto pow2 = [](uint32_t v) { return v >= 4 && v <= 64 && (v & (v - 1)) == 0; };
    if (!pow2(p->cblockw_init) || !pow2(p->cblockh_init))
        return set_err(GRKGPU_EINVAL, "code-block dimensions must be powers of two in [4, 64]");
    cp.numcomps = img->numcomps;
    cp.image = {img->x0, img->y0, img->x1, img->y1};
    for (uint32_t k = 0; k < img->numcomps; ++k) {
        cp.prec[k] = img->prec[k];
        cp.sgnd[k] = img->sgnd[k] ? 1 : 0;
        cp.shift[k] = cp.sgnd[k] ? 0 : (1 << (cp.prec[k] - 1));
        cp.dx[k] = img->dx[k] ? img->dx[k] : 1;
        cp.dy[k] = img->dy[k] ? img->dy[k] : 1;
        if (cp.dx[k] > 255 || cp.dy[k] > 255) return set_err(GRKGPU_EINVAL, "component subsampling must be 1..255");
    }
    cp.numres = p->numresolution;
    cp.cblkw = (uint32_t)floorlog2((int32_t)p->cblockw_init);
    cp.cblkh = (uint32_t)floorlog2((int32_t)p->cblockh_init);
    cp.irrev = p->irreversible ? 1 : 0;
    cp.mct = p->tcp_mct < 0 ? (img->numcomps >= 3 ? 1 : 0) : (p->tcp_mct == 2 ? 2 : p->tcp_mct ? 1 : 0);
    if (cp.mct == 1 && img->numcomps < 3) cp.mct = 0;
    if (p->mct_ncomp) {  // grk_set_MCT's mct_data (j2k.cpp:1899-1961)
        const uint32_t n = img->numcomps;
        if (p->mct_ncomp != n) return set_err(GRKGPU_EINVAL, "custom MCT matrix size differs from the component count");
        if (!p->irreversible) return set_err(GRKGPU_EUNSUPPORTED, "a custom MCT needs the 9/7 wavelet (grk_set_MCT sets it)");
        cp.mct = 2;
        for (uint32_t i = 0; i < n * n; ++i)  // (int32)(m * 2^13), mct.cpp:452-454
            cp.mct_coding[i] = (int32_t)(p->mct_matrix[i] * (float)(1 << 13));
        float m[16 * 16];
        memcpy(m, p->mct_matrix, sizeof(float) * n * n);
        if (!mct_invert(m, cp.mct_decoding, n))
            return set_err(GRKGPU_EINVAL, "Failed to inverse encoder MCT decoding matrix");
        for (uint32_t i = 0; i < n; ++i) {  // mct::calculate_norms (mct.cpp:409-427): column norms of the inverse
            double s = 0;
            for (uint32_t j = 0; j < n; ++j) {
                const float v = cp.mct_decoding[(size_t)j * n + i];
                s += (double)(v * v);
            }
            cp.mct_norms[i] = sqrt(s);
        }
    } else if (cp.mct == 2) {
        return set_err(GRKGPU_EINVAL, "tcp_mct 2 without a custom matrix (grkgpu_set_mct)");
    }
    // "Cannot perform MCT on components with different sizes. Disabling MCT." (j2k.cpp:1963-1971)
    if (cp.mct == 1 && (cp.dx[1] != cp.dx[0] || cp.dx[2] != cp.dx[0] || cp.dy[1] != cp.dy[0] || cp.dy[2] != cp.dy[0]))
        cp.mct = 0;
    if (cp.mct == 2) {
        for (uint32_t k = 1; k < img->numcomps; ++k)
            if (cp.dx[k] != cp.dx[0] || cp.dy[k] != cp.dy[0])
                return set_err(GRKGPU_EUNSUPPORTED, "a custom MCT over components of different sizes");
        for (uint32_t k = 0; k < img->numcomps; ++k) cp.shift[k] = p->mct_dc_shift[k];  // j2k.cpp:1952-1955
    }
    if (p->tile_size_on) {
        if (!p->cp_tdx || !p->cp_tdy) return set_err(GRKGPU_EINVAL, "zero tile size");
        if (p->cp_tx0 > img->x0 || p->cp_ty0 > img->y0 || (uint64_t)p->cp_tx0 + p->cp_tdx <= img->x0 ||
            (uint64_t)p->cp_ty0 + p->cp_tdy <= img->y0)
            return set_err(GRKGPU_EINVAL, "tile origin must satisfy tx0 <= x0 < tx0 + tdx");
        cp.tdx = p->cp_tdx; cp.tdy = p->cp_tdy; cp.tx0 = p->cp_tx0; cp.ty0 = p->cp_ty0;
        cp.tw = ceildiv(img->x1 - cp.tx0, cp.tdx);
        cp.th = ceildiv(img->y1 - cp.ty0, cp.tdy);
    } else {
        cp.tx0 = p->cp_tx0; cp.ty0 = p->cp_ty0;
        if (cp.tx0 > img->x0 || cp.ty0 > img->y0) return set_err(GRKGPU_EINVAL, "tile origin after the image origin");
        cp.tdx = img->x1 - cp.tx0; cp.tdy = img->y1 - cp.ty0;
        cp.tw = cp.th = 1;
    }
    if ((uint64_t)cp.tw * cp.th > 65535) return set_err(GRKGPU_EINVAL, "too many tiles");
    // layers and rate control (j2k.cpp:1841-1857)
    cp.numlayers = p->tcp_numlayers;
    cp.disto_alloc = p->cp_disto_alloc ? 1 : 0;
    cp.fixed_quality = p->cp_fixed_quality ? 1 : 0;
    cp.rate_algo = p->rate_control_algorithm == 1 ? 1 : 0;
    for (uint32_t j = 0; j < cp.numlayers; ++j) {
        const bool prof = p->rsiz != 0;
        if (cp.fixed_quality) cp.distoratio[j] = p->tcp_distoratio[j];
        if (prof || !cp.fixed_quality) cp.rates[j] = p->tcp_rates[j];
    }
    cp.rsiz = (uint16_t)p->rsiz;
    cp.max_cs_size = p->max_cs_size;
    cp.max_comp_size = p->max_comp_size;
    // coding style, precincts (j2k.cpp:1989-2041), progression, tile-parts
    if (p->csty & ~7u) return set_err(GRKGPU_EINVAL, "unknown csty bits");
    cp.csty = p->csty;
    if (p->prog_order < 0 || p->prog_order > 4) return set_err(GRKGPU_EINVAL, "unknown progression order");
    cp.prog = (uint32_t)p->prog_order;
    if ((cp.csty & CSTY_PRT) && p->res_spec) {
        uint32_t q = 0;
        for (int32_t r = (int32_t)cp.numres - 1; r >= 0; --r, ++q) {
            uint32_t w, h;
            if (q < p->res_spec) {
                w = p->prcw_init[q];
                h = p->prch_init[q];
            } else {
                const uint32_t rs = p->res_spec;
                w = p->prcw_init[rs - 1] >> (q - (rs - 1));
                h = p->prch_init[rs - 1] >> (q - (rs - 1));
            }
            cp.prcw[r] = (uint8_t)(w < 1 ? 1 : floorlog2((int32_t)w));
            cp.prch[r] = (uint8_t)(h < 1 ? 1 : floorlog2((int32_t)h));
        }
    } else {
        cp.csty &= ~CSTY_PRT;
        for (uint32_t r = 0; r < cp.numres; ++r) cp.prcw[r] = cp.prch[r] = 15;
    }
    if (p->numpocs) {
        // POC entries of tile 1 (the reference copies tile-matching entries,
        // j2k.cpp:1866-1890); more than one tile with POCs is not supported
        if (p->numpocs > 32) return set_err(GRKGPU_EINVAL, "at most 32 progression order changes");
        if (cp.tw * cp.th != 1) return set_err(GRKGPU_EUNSUPPORTED, "progression order changes need a single tile");
        uint32_t n = 0;
        for (uint32_t i = 0; i < p->numpocs; ++i) {
            if (p->POC[i].tile != 1) continue;
            const grkgpu_poc &src = p->POC[n];  // sic: indexed by the entry count (j2k.cpp:1872-1878)
            if (src.prog < 0 || src.prog > 4) return set_err(GRKGPU_EINVAL, "unknown POC progression");
            cp.pocs[n] = {src.resno0, src.compno0, src.layno1, src.resno1, src.compno1, (uint32_t)src.prog};
            ++n;
        }
        if (!n) return set_err(GRKGPU_EINVAL, "Problem with specified progression order changes");
        cp.numpocs = n;
    }
    cp.tp_on = p->tp_on != 0;
    cp.tp_flag = (char)p->tp_flag;
    generate_qcd(cp);
    return GRKGPU_OK;
}

// ---------------------------------------------------------------------------
// DWT job tables (dwt.hip).  Every tile-component owns two LL ping-pong
// buffers (A: the largest LL, R_{numres-2}; B: the next one), with rows padded
// to 16 elements.  Forward level l writes its LL into buffer l % 2 (the last
// level straight into the Mallat buffer); inverse level r writes into
// (numres - 2 - r) % 2 (the last into the output buffer).
// ---------------------------------------------------------------------------
static uint32_t pad16(uint32_t v) { return (v + 15) & ~15u; }

struct LLGeom { uint32_t strideA = 0, rowsA = 0, strideB = 0, rowsB = 0; uint64_t elems = 0; };

static LLGeom ll_geom(const TileComp &tc) {
    LLGeom g;
    if (tc.numres >= 2) { g.strideA = pad16(tc.res[tc.numres - 2].r.w()); g.rowsA = tc.res[tc.numres - 2].r.h(); }
    if (tc.numres >= 3) { g.strideB = pad16(tc.res[tc.numres - 3].r.w()); g.rowsB = tc.res[tc.numres - 3].r.h(); }
    g.elems = ((uint64_t)g.strideA * g.rowsA + 63) / 64 * 64 + ((uint64_t)g.strideB * g.rowsB + 63) / 64 * 64;
    return g;
}

struct DwtPlan {
    std::vector<std::vector<DwtJob>> levels;  // [level][job]
    std::vector<int> th;                      // window rows per level (dwt_finalize)
    // numres == 1: dst <- src, each tile-component's own sample count (edge
    // tiles and subsampled components are smaller than the others)
    struct Copy1D { int32_t *dst; const int32_t *src; uint64_t elems; };
    std::vector<Copy1D> copies;
    struct Copy2D { int32_t *dst; const int32_t *src; uint32_t dpitch, spitch, w, h; };  // elements
    std::vector<Copy2D> copies2d;  // reduced decode at resolution 0: LL band -> compact output
    bool fused0 = false;  // forward level 0 reads the image planes (DC shift + MCT fused, dwt.hip)
    bool mct3 = false;    // ... and its jobs are MCT component triples (tile-major, component-minor)
    int32_t fmt = SMP_I32;  // ... reading image samples of this format
    bool pixels = false;    // ... from interleaved pixels (MCT triples)
    bool inverse = false;
    std::vector<uint32_t> f01;  // per level: workgroups per job if levels l, l+1 run fused (k_dwt_fwd01), else 0
    std::vector<uint8_t> f01ny; // ... and its level-0 row windows per workgroup (k_dwt_fwd01)
    std::vector<uint8_t> pnw;   // ... or, run by k_dwt_fwd_pair: its level-l waves per workgroup (0: k_dwt_fwd01)
    std::vector<int32_t> ps1;   // ... and its level-(l+1) rows per segment
    uint32_t i01 = 0;           // inverse: workgroups per job if the last two levels run fused (k_dwt_inv01)
    bool restricted = false;    // inverse jobs limited to output regions (window decode)
};

// inverse with numres_dec < tc.numres (reduced-resolution decode): only the
// levels up to resolution numres_dec - 1; the last writes that resolution
// compactly (stride = its width) into `work`.
// resneed (window decode, inverse): per resolution the region (absolute
// resolution coordinates) whose samples the window needs (window_need); each
// inverse level then runs only the windows over its region.
static void dwt_plan_tc(DwtPlan &P, const TileComp &tc, int32_t *work, int32_t *coef, int32_t *llbase, int irrev,
                        bool inverse, uint32_t numres_dec = 0, const std::vector<Rect> *resneed = nullptr) {
    const uint32_t stride = tc.r.w(), rows = tc.r.h();
    P.inverse = inverse;
    if (!inverse || numres_dec == 0 || numres_dec > tc.numres) numres_dec = tc.numres;
    if (inverse && numres_dec == 1 && tc.numres > 1) {
        const Rect &r0 = tc.res[0].r;
        if (r0.w() && r0.h()) P.copies2d.push_back({work, coef, r0.w(), stride, r0.w(), r0.h()});
        return;
    }
    if (tc.numres == 1) {
        if (inverse) P.copies.push_back({work, coef, (uint64_t)stride * rows});
        else P.copies.push_back({coef, work, (uint64_t)stride * rows});
        return;
    }
    const LLGeom g = ll_geom(tc);
    int32_t *buf[2] = {llbase, llbase + ((uint64_t)g.strideA * g.rowsA + 63) / 64 * 64};
    const uint32_t bstride[2] = {g.strideA, g.strideB}, brows[2] = {g.rowsA, g.rowsB};
    const uint32_t full_bytes = (uint32_t)std::min<uint64_t>((uint64_t)stride * rows * 4, 0xffffffffu);
    const uint32_t nlev = inverse ? numres_dec : tc.numres;
    if (P.levels.size() < nlev - 1) P.levels.resize(nlev - 1);
    for (uint32_t lvl = 0; lvl + 1 < nlev; ++lvl) {
        DwtJob j{};
        const bool last = lvl + 2 == nlev;
        Rect cur, lo;
        uint32_t slot;
        if (!inverse) {
            cur = tc.res[tc.numres - 1 - lvl].r;
            lo = tc.res[tc.numres - 2 - lvl].r;
            slot = lvl & 1;
            const uint32_t pslot = (lvl - 1) & 1;
            j.in = lvl == 0 ? work : buf[pslot];
            j.in_stride = lvl == 0 ? stride : bstride[pslot];
            j.in_bytes = lvl == 0 ? full_bytes : bstride[pslot] * brows[pslot] * 4;
            j.out = last ? coef : buf[slot];
            j.out_stride = last ? stride : bstride[slot];
            j.out_bytes = last ? full_bytes : bstride[slot] * brows[slot] * 4;
            j.bands = coef;
            j.bands_stride = stride;
            j.bands_bytes = full_bytes;
        } else {
            const uint32_t r = lvl + 1;
            cur = tc.res[r].r;
            lo = tc.res[r - 1].r;
            slot = (tc.numres - 2 - r) & 1;
            const uint32_t pslot = slot ^ 1;
            j.in = r == 1 ? coef : buf[pslot];
            j.in_stride = r == 1 ? stride : bstride[pslot];
            j.in_bytes = r == 1 ? full_bytes : bstride[pslot] * brows[pslot] * 4;
            j.coef = coef;
            j.coef_stride = stride;
            j.coef_bytes = full_bytes;
            const bool compact = numres_dec < tc.numres;  // reduced: the last level's output is compact
            j.out = last ? work : buf[slot];
            j.out_stride = last ? (compact ? cur.w() : stride) : bstride[slot];
            j.out_bytes = last ? full_bytes : bstride[slot] * brows[slot] * 4;
        }
        if (!cur.w() || !cur.h()) continue;
        j.rw = (int32_t)cur.w(); j.rh = (int32_t)cur.h();
        j.casx = (int32_t)(cur.x0 & 1); j.casy = (int32_t)(cur.y0 & 1);
        j.snx = (int32_t)lo.w(); j.sny = (int32_t)lo.h();
        if (inverse && resneed && lvl + 1 < resneed->size()) {
            const Rect &n = (*resneed)[lvl + 1];  // region of the resolution this level reconstructs
            j.reg_x0 = (int32_t)n.x0 - (int32_t)cur.x0; j.reg_x1 = (int32_t)n.x1 - (int32_t)cur.x0;
            j.reg_y0 = (int32_t)n.y0 - (int32_t)cur.y0; j.reg_y1 = (int32_t)n.y1 - (int32_t)cur.y0;
            if (j.reg_x1 <= j.reg_x0 || j.reg_y1 <= j.reg_y0) j.reg_x0 = j.reg_y0 = 0, j.reg_x1 = j.reg_y1 = 1;
            P.restricted = true;
        }
        P.levels[lvl].push_back(j);
    }
}

// Forward 9/7 levels l and l + 1 fused into one launch (dwt.hip
// k_dwt_fwd01: level l + 1 lifted from level l's LL band kept in LDS) when
// every tile-component has both levels, level l is not the fused DC shift +
// MCT one, and the resolutions are big enough (>= 16 samples each way) for
// the fused windows; f01_rows = 0 keeps one launch per level.  Returns
// the workgroups per job, 0 = not fused.
static uint32_t dwt_f01_tiles(const DwtPlan &P, size_t li, int irrev, int *ny, int *nw0, int *s1) {
    const DwtOptions &o = dwt_options();
    *nw0 = 0;
    if (P.inverse || (li == 0 && P.fused0) || li + 1 >= P.levels.size() || !o.f01_rows) return 0;
    // k_dwt_fwd_pair for 5/3 (pair_kernel 1, the default) or for both (2);
    // 9/7 keeps k_dwt_fwd01's windows by default: the streamed pair moves
    // less (435 vs 593 MB read per 8K frame) but its barrier-coupled
    // strips leave the 64-bit fixed-point lifting latency-bound -- 198 us
    // against 185 (profiles/r05/dwt_pair_ab.txt)
    const bool stream = o.pair_kernel == 2 || (o.pair_kernel == 1 && !irrev);
    if (!irrev && !stream) return 0;
    const auto &l0 = P.levels[li], &l1 = P.levels[li + 1];
    if (l0.empty() || l0.size() != l1.size()) return 0;
    uint64_t samples = 0;
    for (auto &j : l0) samples += (uint64_t)j.rw * j.rh;
    for (size_t i = 0; i < l0.size(); ++i) {
        const DwtJob &a = l0[i], &b = l1[i];
        if (a.snx != b.rw || a.sny != b.rh || a.rw < 16 || a.rh < 16 || b.rw < 16 || b.rh < 16) return 0;
        if (a.out != b.in) return 0;  // level l + 1 must read level l's LL
        if (a.reg_x1 > 0 || b.reg_x1 > 0) return 0;
    }
    if (stream) {
        // k_dwt_fwd_pair: strips of CW1 level-(l+1) columns (3 or 4 level-l
        // waves, whichever wastes fewer columns at the jobs' widths), segments
        // of S1 rows sized so that the launch is about one resident wave of
        // workgroups (3 per CU: 30 KB of LDS and 6 wavefronts each)
        if (samples < o.pair_min_samples) return 0;
        uint64_t cols[2] = {0, 0};
        int maxh = 0;
        for (auto &b : l1) {
            for (int k = 0; k < 2; ++k) {
                const int cw1 = dwt_pair_cw1(irrev, 3 + k);
                cols[k] += (uint64_t)((b.rw + b.casx + cw1 - 1) / cw1) * (3 + k);
            }
            maxh = std::max(maxh, b.rh + b.casy);
        }
        *nw0 = o.pair_waves ? o.pair_waves : cols[0] < cols[1] ? 3 : 4;
        uint64_t strips = 0;
        for (auto &b : l1) {
            const int cw1 = dwt_pair_cw1(irrev, *nw0);
            strips += (uint64_t)((b.rw + b.casx + cw1 - 1) / cw1);
        }
        int rows = o.pair_rows;
        if (!rows) {
            const uint64_t target = 768;
            const uint64_t nseg = std::max<uint64_t>(1, (target + strips / 2) / std::max<uint64_t>(strips, 1));
            rows = (int)(((uint64_t)maxh + nseg - 1) / nseg);
            // whole level-(l+1) chunks of 8 rows: 9/7 streams start 2 rows
            // above the segment (8k - 2 rows), 5/3 at it (8k)
            rows = irrev ? std::max(14, (rows + 2 + 7) / 8 * 8 - 2) : std::max(8, (rows + 7) / 8 * 8);
        }
        *s1 = rows;
        uint32_t maxt = 0;
        for (auto &b : l1)
            maxt = std::max<uint32_t>(maxt, (uint32_t)dwt_pair_wgs(irrev, *nw0, rows, b.rw, b.rh, b.casx, b.casy));
        return maxt;
    }
    // k_dwt_fwd01: only where the pair still fills the chip (f01_min_samples,
    // default 2^23): the 8K frame's levels 2 + 3 fused with 4 row windows took
    // 26 us against 14 + 7 apart (378 workgroups), and with 2 row windows
    // (twice the workgroups; f01_small_min_samples, off by default) 26.4 us
    // of kernel time, the frame's DWT span 220 us against 217 apart
    if (samples >= o.f01_min_samples) *ny = o.f01_rows;
    else if (samples >= o.f01_small_min_samples) *ny = 2;
    else return 0;
    uint32_t maxt = 0;
    for (size_t i = 0; i < l0.size(); ++i) {
        const DwtJob &b = l1[i];
        int tx;
        const int n = dwt01_tiles(irrev, *ny, b.rw, b.rh, b.casx, b.casy, &tx);
        if (n <= 0) return 0;
        maxt = std::max<uint32_t>(maxt, (uint32_t)n);
    }
    return maxt;
}

// The two largest inverse levels (the last two of an inverse plan) in one
// launch (dwt.hip k_dwt_inv01: the smaller one's output kept in LDS) when
// every tile-component has both, the second reads the first's output, both
// resolutions are >= 16 samples each way and the larger level has at least
// inv01_min_samples samples.  Returns the workgroups per job, 0 = apart.
static uint32_t dwt_inv01_plan(const DwtPlan &P, int irrev) {
    const DwtOptions &o = dwt_options();
    const size_t n = P.levels.size();
    if (!P.inverse || !o.inv01 || n < 2 || P.restricted) return 0;
    const auto &la = P.levels[n - 2], &lb = P.levels[n - 1];
    if (la.empty() || la.size() != lb.size()) return 0;
    uint64_t samples = 0;
    for (auto &j : lb) samples += (uint64_t)j.rw * j.rh;
    if (samples < o.inv01_min_samples) return 0;
    uint32_t maxt = 0;
    for (size_t i = 0; i < la.size(); ++i) {
        const DwtJob &a = la[i], &b = lb[i];
        if (b.in != a.out || b.snx != a.rw || b.sny != a.rh || a.rw < 16 || a.rh < 16 || b.rw < 16 || b.rh < 16)
            return 0;
        maxt = std::max<uint32_t>(maxt, (uint32_t)dwt_inv01_tiles(irrev, b.rw, b.rh, b.casx, b.casy));
    }
    return maxt;
}

// Pick each level's window height from the level's total size; tile counts.
static void dwt_finalize(DwtPlan &P, int irrev) {
    P.i01 = dwt_inv01_plan(P, irrev);
    P.th.assign(P.levels.size(), 8);
    for (size_t l = 0; l < P.levels.size(); ++l) {
        uint64_t samples = 0;
        int minw = INT32_MAX, minh = INT32_MAX;
        for (auto &j : P.levels[l]) {
            samples += (uint64_t)j.rw * j.rh;
            minw = std::min(minw, (int)j.rw);
            minh = std::min(minh, (int)j.rh);
        }
        P.th[l] = dwt_pick_th(irrev, samples, minw, minh);
        // the fused DC shift + MCT level 0 holds the windows of three
        // components: 8-row windows (measured on the 8K frame: 5/3 162 us at
        // TH 8, 168 at 16, 194 at 32; 9/7 229 / 319 / 330)
        if (l == 0 && P.mct3) P.th[l] = 8;
        for (auto &j : P.levels[l]) dwt_job_tiles(irrev, P.th[l], j);
    }
    // Fused level pairs (k_dwt_fwd01).  A fused pair never writes its first
    // level's LL band, so the LL ping-pong is re-dealt: every level reads the
    // last LL band written and keeps its own output slot unless its launch
    // reads that slot (for a fused pair: the pair's input), in which case it
    // takes the other one -- no launch reads and writes one buffer.
    P.f01.assign(P.levels.size(), 0);
    P.f01ny.assign(P.levels.size(), 0);
    P.pnw.assign(P.levels.size(), 0);
    P.ps1.assign(P.levels.size(), 0);
    bool any = false;
    for (size_t l = 0; l + 1 < P.levels.size(); ++l) {
        int ny = 4, nw0 = 0, s1 = 0;
        if ((P.f01[l] = dwt_f01_tiles(P, l, irrev, &ny, &nw0, &s1))) {
            P.f01ny[l] = (uint8_t)ny;
            P.pnw[l] = (uint8_t)nw0;
            P.ps1[l] = s1;
            any = true;
            ++l;
        }
    }
    // the re-deal below pairs job i of every level (one tile-component)
    for (auto &l : P.levels) any = any && l.size() == P.levels[0].size();
    if (!any) {
        P.f01.assign(P.levels.size(), 0);
        return;
    }
    struct Slot { int32_t *p; uint32_t stride, bytes; };
    for (size_t i = 0; i < P.levels[0].size(); ++i) {
        Slot slot[2] = {{P.levels[0][i].out, P.levels[0][i].out_stride, P.levels[0][i].out_bytes}, {nullptr, 0, 0}};
        if (P.levels.size() > 2) slot[1] = {P.levels[1][i].out, P.levels[1][i].out_stride, P.levels[1][i].out_bytes};
        Slot prev{const_cast<int32_t *>(P.levels[0][i].in), P.levels[0][i].in_stride, P.levels[0][i].in_bytes};
        for (size_t l = 0; l < P.levels.size(); ++l) {
            DwtJob &j = P.levels[l][i];
            const bool second = l > 0 && P.f01[l - 1];
            if (!second) { j.in = prev.p; j.in_stride = prev.stride; j.in_bytes = prev.bytes; }
            if (j.out != j.bands) {  // not the last level (that one writes its LL into the Mallat buffer)
                // the plan's own slot unless the launch reads it
                const int32_t *rd = second ? P.levels[l - 1][i].in : j.in;
                if (j.out == rd) {
                    const Slot &o = slot[0].p != rd ? slot[0] : slot[1];
                    j.out = o.p; j.out_stride = o.stride; j.out_bytes = o.bytes;
                }
            }
            prev = {j.out, j.out_stride, j.out_bytes};
        }
    }
}

// Upload the job table (one H2D from pinned memory).
static hipError_t dwt_upload(DwtPlan &P, DevBuf &djobs, HostBuf &hjobs, int irrev, hipStream_t s) {
    dwt_finalize(P, irrev);
    size_t n = 0;
    for (auto &l : P.levels) n += l.size();
    if (!n) return hipSuccess;
    hipError_t e = djobs.ensure(n * sizeof(DwtJob) + 256);
    if (e == hipSuccess) e = hjobs.ensure(n * sizeof(DwtJob) + 256);
    if (e != hipSuccess) return e;
    DwtJob *h = hjobs.as<DwtJob>();
    size_t k = 0;
    for (auto &l : P.levels)
        for (auto &j : l) h[k++] = j;
    return hipMemcpyAsync(djobs.p, hjobs.p, n * sizeof(DwtJob), hipMemcpyHostToDevice, s);
}

// Run the levels (job table already uploaded by dwt_upload on the same stream).
// All levels of an uploaded plan (job table at djobs, levels back to back);
// fused 9/7 level pairs (P.f01) as one launch (8K frame: 0+1, then 2, 3, 4).
// Launch log (grkgpu_set_launch_timing): events around every level launch
// and each launch's kernel and algorithmic bytes (B_DWT's 8 B per sample of
// every level it computes).
// Per-launch device times: one event between consecutive launches of a
// level sequence (a launch's end is the next one's start), so what a launch
// is charged is the stream's time from the previous launch's end to its own
// -- an event pair around every launch added ~1.5 us of event handling to
// each (8K 9/7: 224.7 us summed vs 213.4 by rocprof, 218.6 span).
struct LaunchLog {
    std::vector<hipEvent_t> *ev;
    std::vector<grkgpu_launch_time> *rec;
    std::vector<std::pair<uint32_t, uint32_t>> *idx;
    uint32_t used = 0;  // events recorded in this call
};

static uint64_t level_bytes(const std::vector<DwtJob> &l) {
    uint64_t n = 0;
    for (auto &j : l) n += 8ull * (uint64_t)j.rw * (uint64_t)j.rh;
    return n;
}

static hipError_t log_event(LaunchLog *log, hipStream_t s, uint32_t *at) {
    while (log->ev->size() <= log->used) {
        hipEvent_t e;
        hipError_t r = hipEventCreate(&e);
        if (r != hipSuccess) return r;
        log->ev->push_back(e);
    }
    *at = log->used++;
    return hipEventRecord((*log->ev)[*at], s);
}

// chained: the previous logged launch ended right before this one (same
// level sequence, nothing else enqueued in between): its end event is this
// launch's start
static hipError_t log_begin(LaunchLog *log, hipStream_t s, const char *name, uint32_t lev0, uint32_t nlev, uint64_t bytes,
                            bool chained = false) {
    if (!log) return hipSuccess;
    grkgpu_launch_time t{};
    snprintf(t.kernel, sizeof(t.kernel), "%s", name);
    t.level0 = lev0;
    t.levels = nlev;
    t.bytes = bytes;
    uint32_t at;
    if (chained && !log->idx->empty()) {
        at = log->idx->back().second;
    } else {
        hipError_t r = log_event(log, s, &at);
        if (r != hipSuccess) return r;
    }
    log->rec->push_back(t);
    log->idx->push_back({at, at});
    return hipSuccess;
}

static hipError_t log_end(LaunchLog *log, hipStream_t s) {
    if (!log) return hipSuccess;
    return log_event(log, s, &log->idx->back().second);
}

static hipError_t dwt_run_levels(const DwtPlan &P, DwtJob *djobs, int irrev, bool inverse, hipStream_t s,
                                 LaunchLog *log = nullptr) {
    hipError_t e = hipSuccess;
    size_t k = 0;
    const char *wl = irrev ? "9/7" : "5/3";
    char name[48];
    for (size_t li = 0; li < P.levels.size(); ++li) {
        const auto &l = P.levels[li];
        if (li < P.f01.size() && P.f01[li]) {
            snprintf(name, sizeof(name), P.pnw[li] ? "k_dwt_fwd_pair<%s>" : "k_dwt_fwd01<%s>", wl);
            if ((e = log_begin(log, s, name, (uint32_t)li, 2, level_bytes(l) + level_bytes(P.levels[li + 1]), li > 0)))
                return e;
            if (P.pnw[li])
                e = launch_dwt_fwd_pair(djobs + k, djobs + k + l.size(), (uint32_t)l.size(), P.f01[li], irrev, P.pnw[li],
                                        P.ps1[li], s);
            else
                e = launch_dwt_fwd01(djobs + k, djobs + k + l.size(), (uint32_t)l.size(), P.f01[li], irrev, P.f01ny[li],
                                     s);
            if (e != hipSuccess || (e = log_end(log, s))) return e;
            k += l.size() + P.levels[li + 1].size();
            ++li;
            continue;
        }
        if (inverse && P.i01 && li + 2 == P.levels.size()) {
            snprintf(name, sizeof(name), "k_dwt_inv01<%s>", wl);
            if ((e = log_begin(log, s, name, (uint32_t)li, 2, level_bytes(l) + level_bytes(P.levels[li + 1]), li > 0)))
                return e;
            e = launch_dwt_inv01(djobs + k, djobs + k + l.size(), (uint32_t)l.size(), P.i01, irrev,
                                 dwt_options().inv01, s);
            if (e != hipSuccess || (e = log_end(log, s))) return e;
            k += l.size() + P.levels[li + 1].size();
            ++li;
            continue;
        }
        uint32_t maxt = 0;
        for (auto &j : l) maxt = std::max<uint32_t>(maxt, (uint32_t)j.ntiles);
        const bool f0 = li == 0 && P.fused0 && !inverse;
        const int code = P.th[li] | (f0 ? (P.mct3 ? DWT_FUSED_MCT3 : DWT_FUSED) | (P.fmt << DWT_FMT_SHIFT) |
                                       (P.mct3 && P.pixels ? DWT_FUSED_PIXELS : 0)
                                 : 0);
        snprintf(name, sizeof(name), "%s<%s,%d>", inverse ? "k_dwt_inv" : f0 && P.mct3 ? "k_dwt_fwd_mct3" : "k_dwt_fwd", wl,
                 P.th[li] & 0xff);
        if ((e = log_begin(log, s, name, (uint32_t)li, 1, level_bytes(l), li > 0))) return e;
        e = launch_dwt_jobs(djobs + k, (uint32_t)l.size(), maxt, code, irrev, inverse ? 1 : 0, s);
        if (e != hipSuccess || (e = log_end(log, s))) return e;
        k += l.size();
    }
    return hipSuccess;
}

// fill in the launch times once the stream has passed the logged launches
static void log_collect(grkgpu_ctx *c) {
    for (size_t i = 0; i < c->ltimes.size() && i < c->lidx.size(); ++i)
        if (hipEventElapsedTime(&c->ltimes[i].ms, c->lev[c->lidx[i].first], c->lev[c->lidx[i].second]) != hipSuccess)
            c->ltimes[i].ms = -1;
}

static hipError_t dwt_launch(DwtPlan &P, DevBuf &djobs, int irrev, bool inverse, hipStream_t s,
                             LaunchLog *log = nullptr) {
    for (auto &cp : P.copies) {
        if (!cp.elems) continue;
        hipError_t e = hipMemcpyAsync(cp.dst, cp.src, cp.elems * 4, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return e;
    }
    for (auto &cp : P.copies2d) {
        hipError_t e = hipMemcpy2DAsync(cp.dst, (size_t)cp.dpitch * 4, cp.src, (size_t)cp.spitch * 4, (size_t)cp.w * 4,
                                        cp.h, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return e;
    }
    return dwt_run_levels(P, djobs.as<DwtJob>(), irrev, inverse, s, log);
}

// the launches and copies dwt_launch issues for a plan
static uint32_t dwt_launch_count(const DwtPlan &P, bool inverse) {
    uint32_t nl = (uint32_t)P.copies2d.size();
    for (auto &cp : P.copies) nl += cp.elems != 0;
    for (size_t li = 0; li < P.levels.size(); ++li) {
        ++nl;
        if ((li < P.f01.size() && P.f01[li]) || (inverse && P.i01 && li + 2 == P.levels.size())) ++li;  // a level pair
    }
    return nl;
}

// The plan pair of a call whose tile-components may mix the wavelets (COC /
// tile COD, or the items of a batch): P[1] the 9/7 plan through dwtjobs, P[0]
// the 5/3 plan through dwtjobs53.  Their uploads, and their launches under the
// call's launch log; *nl grows by the launches and copies issued.
static hipError_t dwt_upload_plans(grkgpu_ctx *c, DwtPlan (&P)[2]) {
    const hipError_t e = dwt_upload(P[1], c->dwtjobs, c->h_dwtjobs, 1, c->stream);
    return e != hipSuccess ? e : dwt_upload(P[0], c->dwtjobs53, c->h_dwtjobs53, 0, c->stream);
}
static hipError_t dwt_launch_plans(grkgpu_ctx *c, DwtPlan (&P)[2], bool inverse, uint32_t *nl) {
    c->ltimes.clear();
    c->lidx.clear();
    LaunchLog llog{&c->lev, &c->ltimes, &c->lidx};
    LaunchLog *log = c->launch_timing ? &llog : nullptr;
    hipError_t e = dwt_launch(P[1], c->dwtjobs, 1, inverse, c->stream, log);
    if (e == hipSuccess) e = dwt_launch(P[0], c->dwtjobs53, 0, inverse, c->stream, log);
    *nl += dwt_launch_count(P[1], inverse) + dwt_launch_count(P[0], inverse);
    return e;
}

static bool overlap(const Rect &a, const Rect &b) { return a.x0 < b.x1 && b.x0 < a.x1 && a.y0 < b.y1 && b.y0 < a.y1; }
static Rect intersect(const Rect &a, const Rect &b) {
    Rect r{std::max(a.x0, b.x0), std::max(a.y0, b.y0), std::min(a.x1, b.x1), std::min(a.y1, b.y1)};
    if (r.x1 < r.x0) r.x1 = r.x0;
    if (r.y1 < r.y0) r.y1 = r.y0;
    return r;
}

using BandNeed = std::vector<std::array<Rect, 3>>;  // [resno][band] region a window needs

// need: (window decode) only code-blocks overlapping need[resno][band].
template <typename F>
static void for_each_cblk(TileComp &tc, F f, uint32_t maxres = 0xffffffffu, const BandNeed *need = nullptr) {
    for (uint32_t resno = 0; resno < tc.numres && resno < maxres; ++resno) {
        Resolution &res = tc.res[resno];
        for (uint32_t b = 0; b < res.numbands; ++b) {
            Band &band = res.bands[b];
            for (auto &pr : band.precs)
                for (auto &c : pr.cblks)
                    if (!need || overlap(c.r, (*need)[resno][b])) f(band, c);
        }
    }
}

// Window decode: the sub-band regions whose coefficients reach the samples
// of `win` (tile-component coordinates).  Going down from the full
// resolution, a region of resolution r needs, in each of its bands and in the
// resolution r-1 below, the half-size region widened by M samples on every
// side -- more than the synthesis supports (5/3: 2 taps, 9/7: 4 taps at the
// full scale, i.e. <= 2 at the band scale), so every coefficient that
// influences the window is decoded and the window's samples come out exactly
// as in a full decode (dwt.cpp decode_tile_53 / _97 compute each output from
// its support only).
// resneed (optional): per resolution the region of its samples the window
// needs (the inverse DWT levels run only over these).
static BandNeed window_need(const TileComp &tc, const Rect &win, std::vector<Rect> *resneed = nullptr,
                            uint32_t reduce = 0) {
    constexpr uint32_t M = 4;
    BandNeed need(tc.numres);
    // win: on the component's grid at resolution numres - 1 - reduce
    Rect n = intersect(win, tc.res[tc.numres - 1 - reduce].r);
    if (resneed) resneed->assign(tc.numres, Rect{});
    for (int32_t r = (int32_t)tc.numres - 1 - (int32_t)reduce; r >= 0; --r) {
        const Resolution &res = tc.res[r];
        if (resneed) (*resneed)[r] = n;
        if (r == 0) {
            need[0][0] = intersect(n, res.bands[0].r);
            break;
        }
        const Rect half{n.x0 / 2 > M ? n.x0 / 2 - M : 0, n.y0 / 2 > M ? n.y0 / 2 - M : 0, (n.x1 + 1) / 2 + M,
                        (n.y1 + 1) / 2 + M};
        for (uint32_t b = 0; b < res.numbands; ++b) need[r][b] = intersect(half, res.bands[b].r);
        n = intersect(half, tc.res[r - 1].r);
    }
    return need;
}

// ---------------------------------------------------------------------------
// encode
// ---------------------------------------------------------------------------
// The host half of an encode is EncHost: begin() (parameter and format checks,
// tile geometry, the code-block tables with their slab offsets, the tile-part
// counts -- everything that can refuse an image before a device is touched),
// records() (the coders' results as EncCblkState and pass records, from the
// device-formed records or from EncResult), finish() (rate allocation and
// packets per tile on the host pool, the header blob and the PlanItem list).
// compress_impl runs the three around its device work for one image; the
// batch encode runs them per item and merges the tables in between.  Offsets
// in eb (coef_off, out_off), symoff and the tiles' arena_off / lloff start at
// zero here; the batch rebases them (EncHost::rebase).
namespace {
struct EncHost {
    // ---- in ----
    const grkgpu_image_desc *img = nullptr;
    const grkgpu_cparams *p = nullptr;
    int32_t fmt_in = 0;  // sample_fmt with its flags
    uint32_t tb = 0, te = 0xffffffffu, parts = GRKGPU_PART_ALL;
    uint32_t row0 = 0, nrows = 0, col0 = 0, ncols = 0;
    bool export_blocks = false, batch = false;
    int force_dist = 0;

    // ---- begin() ----
    CodingParams cp;
    int32_t fmt = 0, lfmt = 0;  // the width; the width with the flags the loader kernels take
    bool il = false, big = false, mixed = false;
    uint32_t sb = 4, nc = 0, iw = 0, ih = 0, pw = 0;
    uint64_t plane = 0;
    Rect prect[GRKGPU_MAX_COMPS];
    uint64_t poff[GRKGPU_MAX_COMPS + 1];
    uint32_t ntiles = 0;
    std::vector<Tile> tiles;
    uint64_t arena = 0, llarena = 0;
    std::vector<uint64_t> lloff;
    std::vector<EncBlock> eb;
    struct BlkInfo {  // position + distortion weights (t1_getwmsedec)
        uint32_t compno, level, orient;
        float stepsize;
        uint32_t tileno, resno, precno, cblkno;
        Rect r;
    };
    std::vector<BlkInfo> binfo;
    std::vector<uint64_t> symoff;  // per-block symbol-stream slots, sized by the band's numbps bound (nblk + 1)
    std::vector<uint32_t> pcap;    // per-block pass-record slots (3 numbps - 2 of that bound)
    uint64_t sym_total = 0, out_total = 0, ptotal = 0;
    uint32_t maxdepth = 1, nblk = 0;
    bool need_rc = false;
    const double *mct_norms = nullptr;
    uint32_t mct_numcomps = 0;
    std::vector<std::vector<uint32_t>> tp_counts;  // [tile][poc entry]
    uint32_t total_tile_parts = 0;
    // the image's place in the merged tables of a batch (zero in a single
    // call): its first block, first rate-controlled block, first pass-record slot
    uint64_t mb0 = 0, rcb0 = 0, slot0 = 0;

    // ---- records ----
    std::vector<EncCblkState> cst;
    EncPass *precs = nullptr;  // the records Tier-2 reads (cst[i].pass0 counts from here)
    uint64_t npass = 0, nsym = 0;
    std::vector<EncLayer> layers;
    std::vector<double> blk_disto;
    std::vector<uint32_t> blen;  // each block's MQ bytes

    // ---- finish ----
    struct TileOut {
        ByteBuf hdr;
        std::vector<PlanItem> plan;
        std::vector<uint8_t> tlm;
        double rate_ms = 0, packet_ms = 0;
        RateStats rs;
        bool ok = true;
    };
    std::vector<TileOut> touts;
    ByteBuf hdr, mainhdr;
    std::vector<PlanItem> plan;
    size_t tlm_at = 0;
    uint64_t tile_bound = 0;
    double t_rate = 0, t_packets = 0;  // summed over tiles (host CPU time)
    RateStats rsum;

    int begin();
    // element offset of tile-component tc's first sample in plane k
    uint64_t plane_org(uint32_t k, const TileComp &tc) const {
        return (uint64_t)(tc.r.y0 - prect[k].y0) * prect[k].w() + (tc.r.x0 - prect[k].x0);
    }
    double wfac(uint32_t i) const {
        const BlkInfo &bi = binfo[i];
        return t1_wmsedec_factor(bi.compno, bi.level, bi.orient, cp.irrev ? 0 : 1, (double)bi.stepsize, mct_norms,
                                 mct_numcomps);
    }
    void rebase(uint64_t abase, uint64_t llbase, uint64_t obase, uint64_t sbase);
    void records_alloc();
    int records_dev(const PassSum *sm, const uint64_t *p0, EncPass *recs);
    int records_host_count(const EncResult *res);
    void records_host_fill(const EncResult *res, EncPass *out);
    int finish_begin();
    void finish_tile(size_t ti);
    int finish_end();
    void tile_rates(const Rect &tr, uint32_t ntp, double *rates) const;
};

int EncHost::begin() {
    int rc = setup_params(img, p, cp);
    if (rc) return rc;
    // sample_fmt = width | flags (GRKGPU_SAMPLE_INTERLEAVED / _BIG_ENDIAN), all
    // checked before the context or a device is touched
    const int32_t fflags = fmt_in & ~0xff;
    fmt = fmt_in & 0xff;
    if (fflags & ~(SMP_INTERLEAVED | SMP_BIG_ENDIAN)) return set_err(GRKGPU_EINVAL, "unknown sample format flags");
    if (fmt < SMP_I32 || fmt > SMP_I16) return set_err(GRKGPU_EINVAL, "unknown sample format");
    if ((fflags & SMP_BIG_ENDIAN) && fmt != SMP_U16 && fmt != SMP_I16)
        return set_err(GRKGPU_EINVAL, "big-endian samples are 16-bit (U16 / I16)");
    for (uint32_t k = 0; fmt != SMP_I32 && k < img->numcomps; ++k) {
        const bool sg = fmt == SMP_I8 || fmt == SMP_I16;
        if ((img->sgnd[k] != 0) != sg || img->prec[k] > 8 * sample_bytes(fmt))
            return set_err(GRKGPU_EINVAL, "sample format does not hold the component's precision / signedness");
    }
    sb = sample_bytes(fmt);  // bytes per input sample
    for (uint32_t k = 1; (fflags & SMP_INTERLEAVED) && k < cp.numcomps; ++k)
        if (cp.dx[k] != cp.dx[0] || cp.dy[k] != cp.dy[0])
            return set_err(GRKGPU_EUNSUPPORTED, "interleaved samples need every component on one grid");
    // pixels in planes[0] (one component's pixels are its plane), and the
    // format as the loader kernels take it
    il = (fflags & SMP_INTERLEAVED) && cp.numcomps > 1;
    big = (fflags & SMP_BIG_ENDIAN) != 0;
    lfmt = fmt | (il ? SMP_INTERLEAVED : 0) | (big ? SMP_BIG_ENDIAN : 0);
    {
        const uint32_t nt = cp.tw * cp.th;
        if (te > nt) te = nt;
        if (tb > te) return set_err(GRKGPU_EINVAL, "bad tile range");
    }
    nc = cp.numcomps;
    iw = cp.image.w();
    ih = cp.image.h();
    if (nrows == 0) {
        if (row0) return set_err(GRKGPU_EINVAL, "row0 without nrows");
        nrows = ih;
    }
    if ((uint64_t)row0 + nrows > ih) return set_err(GRKGPU_EINVAL, "row range outside the image");
    if (ncols == 0) {
        if (col0) return set_err(GRKGPU_EINVAL, "col0 without ncols");
        ncols = iw;
    }
    if ((uint64_t)col0 + ncols > iw) return set_err(GRKGPU_EINVAL, "column range outside the image");
    pw = ncols;                    // row stride of the caller's planes (samples)
    plane = (uint64_t)pw * nrows;  // samples per plane held by the caller
    // subsampled components (SIZ XRsiz / YRsiz): each plane on its own grid
    bool subs = false;
    mixed = false;  // components on different grids
    for (uint32_t k = 0; k < nc; ++k) {
        subs = subs || cp.dx[k] != 1 || cp.dy[k] != 1;
        mixed = mixed || cp.dx[k] != cp.dx[0] || cp.dy[k] != cp.dy[0];
    }
    if (batch && subs) return set_err(GRKGPU_EUNSUPPORTED, "a subsampled component is not supported in a batch");
    if (batch && cp.mct == 2) return set_err(GRKGPU_EUNSUPPORTED, "a custom MCT is not supported in a batch");
    // the rectangle each caller plane covers (the rows / columns held, on the
    // component's grid: ceil(x / dx), TileComponent.cpp:150-196 -- a tile's
    // plane holds its tile-component, as grk_write_tile's data does,
    // TileProcessor.cpp:1923-1972), its stride, and its offset in the staging
    // buffer (samples)
    poff[0] = 0;
    const Rect held{cp.image.x0 + col0, cp.image.y0 + row0, cp.image.x0 + col0 + ncols, cp.image.y0 + row0 + nrows};
    for (uint32_t k = 0; k < nc; ++k) {
        prect[k] = comp_rect(held, cp.dx[k], cp.dy[k]);
        poff[k + 1] = poff[k] + (uint64_t)prect[k].w() * prect[k].h();
    }

    // geometry for every tile of the shard, arena offsets, block table
    ntiles = te - tb;
    tiles.resize(ntiles);
    lloff.resize((size_t)ntiles * nc);
    // tile geometry (independent per tile) on the host pool, then the block
    // table in tile order
    for (uint32_t t = 0; t < ntiles; ++t) {
        const Rect r = tile_rect(cp, tb + t);
        if (r.y0 - cp.image.y0 < row0 || r.y1 - cp.image.y0 > row0 + nrows || r.x0 - cp.image.x0 < col0 ||
            r.x1 - cp.image.x0 > col0 + ncols)
            return set_err(GRKGPU_EINVAL, "a tile of the range lies outside the rows / columns given");
    }
    host_parallel_for(ntiles, 1, [&](size_t t0, size_t t1) {
        for (size_t t = t0; t < t1; ++t) {
            Tile &tile = tiles[t];
            tile.index = tb + (uint32_t)t;
            tile.r = tile_rect(cp, tile.index);
            tile.comps.resize(nc);
            for (uint32_t k = 0; k < nc; ++k) build_tilecomp(tile.comps[k], tile.r, cp, k, true);
        }
    });
    for (uint32_t t = 0; t < ntiles; ++t) {
        Tile &tile = tiles[t];
        for (uint32_t k = 0; k < nc; ++k) {
            TileComp &tc = tile.comps[k];
            tc.arena_off = arena;
            uint64_t area = (uint64_t)tc.r.w() * tc.r.h();
            arena += (area + 63) & ~63ull;
            lloff[t * nc + k] = llarena;
            llarena += ll_geom(tc).elems;
            for_each_cblk(tc, [&](Band &band, Cblk &cb) {
                cb.gidx = (uint32_t)eb.size();
                EncBlock b;
                b.coef_off = tc.arena_off + (uint64_t)cb.by * tc.r.w() + cb.bx;
                b.out_off = 0;
                b.stride = tc.r.w();
                b.w = cb.r.w();
                b.h = cb.r.h();
                b.orient = band.bandno;
                b.qmfbid = cp.irrev ? 0 : 1;
                b.inv_step = (int32_t)band.inv_step;
                eb.push_back(b);
                uint32_t resno = 0;
                while (&tc.res[resno].bands[0] > &band || &tc.res[resno].bands[2] < &band) ++resno;
                uint32_t precno = 0, cblkno = 0;
                for (size_t q = 0; q < band.precs.size(); ++q) {
                    const auto &cv = band.precs[q].cblks;
                    if (!cv.empty() && &cb >= &cv.front() && &cb <= &cv.back()) {
                        precno = (uint32_t)q;
                        cblkno = (uint32_t)(&cb - &cv.front());
                        break;
                    }
                }
                binfo.push_back({k, tc.numres - 1 - resno, band.bandno, band.stepsize, tile.index, resno, precno,
                                 cblkno, cb.r});
                const uint32_t bound = std::min<uint32_t>(band.numbps, 32);
                pcap.push_back(bound ? 3 * bound - 2 : 0);
                symoff.push_back(sym_total);
                sym_total += (uint64_t)bound * sym_slot_bytes(b.w, b.h);
                maxdepth = std::max(maxdepth, bound);
            });
        }
    }
    nblk = (uint32_t)eb.size();
    out_total = 0;
    ptotal = 0;
    for (uint32_t i = 0; i < nblk; ++i) {  // MQ output slab: t1_enc_slab_bytes at the band's bound (+ the zero pad byte before)
        EncBlock &b = eb[i];
        out_total += 16;
        b.out_off = out_total;
        out_total += ((uint64_t)t1_enc_slab_bytes(b.w, b.h, cp.cblksty, (pcap[i] + 2) / 3) + 15) & ~15ull;
        ptotal += pcap[i];
    }
    symoff.push_back(sym_total);
    // per-pass distortion only when some layer is rate-controlled
    // (TileProcessor::needs_rate_control, TileProcessor.cpp:260-266)
    need_rc = force_dist != 0;
    for (uint32_t l = 0; l < cp.numlayers; ++l)
        need_rc = need_rc || (cp.disto_alloc && cp.rates[l] > 0.0) || (cp.fixed_quality && cp.distoratio[l] > 0.0f);
    if (cp.mct == 1) {  // TileProcessor::t1_encode (TileProcessor.cpp:1535-1551), mct.cpp:65-79
        static const double kRev[3] = {1.732, .8292, .8292}, kIrrev[3] = {1.732, 1.805, 1.573};
        mct_norms = cp.irrev ? kIrrev : kRev;
        mct_numcomps = 3;
    } else {  // custom MCT: the inverse's column norms (TileProcessor.cpp:1548-1551); else none
        mct_numcomps = nc;
        if (cp.mct == 2) mct_norms = cp.mct_norms;  // (cp is a member: an EncHost is never copied after begin())
    }
    if (export_blocks) return GRKGPU_OK;
    // tile-parts of every tile (j2k_calculate_tp, j2k.cpp:2990-3048): needed
    // for the TLM marker and the rate bookkeeping even outside the shard
    const uint32_t ntot = cp.tw * cp.th;
    tp_counts.resize(ntot);
    total_tile_parts = 0;
    for (uint32_t t = 0; t < ntot; ++t) {
        Tile tmp;
        const Tile *tp = nullptr;
        if (t >= tb && t < te) tp = &tiles[t - tb];
        else if (cp.tp_on) {
            tmp.index = t;
            tmp.r = tile_rect(cp, t);
            tmp.comps.resize(nc);
            for (uint32_t k = 0; k < nc; ++k) build_tilecomp(tmp.comps[k], tmp.r, cp, k, true);
            tp = &tmp;
        }
        if (tp) tp_counts[t] = tile_part_counts(cp, *tp);
        else tp_counts[t].assign(num_poc_entries(cp), 1);
        uint32_t n = 0;
        for (uint32_t v : tp_counts[t]) n += v;
        if (n > 255) return set_err(GRKGPU_EUNSUPPORTED, "more than 255 tile-parts in a tile");
        total_tile_parts += n;
    }
    return GRKGPU_OK;
}

// the item's place in the merged tables of a batch: coefficient arena, LL
// arena, MQ slab and symbol arena bases
void EncHost::rebase(uint64_t abase, uint64_t llbase, uint64_t obase, uint64_t sbase) {
    for (EncBlock &b : eb) {
        b.coef_off += abase;
        b.out_off += obase;
    }
    for (uint64_t &o : symoff) o += sbase;
    for (Tile &tile : tiles)
        for (TileComp &tc : tile.comps) tc.arena_off += abase;
    for (uint64_t &o : lloff) o += llbase;
}

void EncHost::records_alloc() {
    cst.assign(nblk, EncCblkState{});
    layers.assign((size_t)nblk * cp.numlayers, EncLayer{0, 0, 0, 0.0});
    blk_disto.assign(nblk, 0.0);
    blen.assign(nblk, 0);
    npass = 0;
    nsym = 0;
}

// the device-formed records (launch_pass_records): sm = this image's block
// summaries, p0 = its blocks' record slots (nblk + 1), recs = the record at
// slot p0[0]
int EncHost::records_dev(const PassSum *sm, const uint64_t *p0, EncPass *recs) {
    records_alloc();
    for (uint32_t i = 0; i < nblk; ++i) {
        const PassSum &q = sm[i];
        if (q.bad & 1u) return set_err(GRKGPU_EUNSUPPORTED, "code-block numbps exceeds its band's bound");
        if (q.bad & 2u) return set_err(GRKGPU_EUNSUPPORTED, "too many coding passes");
        if (q.bad & 4u) return set_err(GRKGPU_EUNSUPPORTED, "MQ slab overflow");
        nsym += q.nsym;
        EncCblkState &st = cst[i];
        st.numbps = q.numbps;
        st.numpasses = q.numpasses;
        st.pass0 = (uint32_t)(p0[i] - p0[0]);
        st.dev_off = eb[i].out_off;
        st.smin = q.smin;
        st.smax = q.smax;
        st.s0max = q.s0max;
        st.z0 = q.z0 != 0;
        blk_disto[i] = q.disto;
        blen[i] = q.len;
    }
    if (ptotal > 0xffffffffu) return set_err(GRKGPU_EUNSUPPORTED, "too many coding passes");
    npass = ptotal;
    precs = recs;
    return GRKGPU_OK;
}

// the host-formed records: validate and lay the blocks' passes out (prefix
// sum; npass records), then -- records_host_fill -- fill them on the host
// pool (blocks are independent)
int EncHost::records_host_count(const EncResult *res) {
    records_alloc();
    for (uint32_t i = 0; i < nblk; ++i) {
        const EncResult &r = res[i];
        if (r.pad) return set_err(GRKGPU_EUNSUPPORTED, "code-block numbps exceeds its band's bound");
        if (r.numpasses > GRK_MAX_PASSES) return set_err(GRKGPU_EUNSUPPORTED, "too many coding passes");
        const uint32_t np = r.numpasses;
        if (np && r.rate[np - 1] > t1_enc_slab_bytes(eb[i].w, eb[i].h, cp.cblksty, r.numbps)) return set_err(GRKGPU_EUNSUPPORTED, "MQ slab overflow");
        nsym += r.nsym;
        EncCblkState &st = cst[i];
        st.numbps = r.numbps;
        st.numpasses = np;
        st.pass0 = (uint32_t)npass;
        st.dev_off = eb[i].out_off;
        npass += np;
    }
    return GRKGPU_OK;
}

void EncHost::records_host_fill(const EncResult *res, EncPass *out0) {
    host_parallel_for(nblk, 1024, [&](size_t b0, size_t b1) {
        for (size_t i = b0; i < b1; ++i) {
            const EncResult &r = res[i];
            const uint32_t np = r.numpasses;
            EncPass *out = out0 + cst[i].pass0;
            double cum = 0.0;
            const double wf = need_rc ? wfac((uint32_t)i) : 0.0;
            for (uint32_t k = 0; k < np; ++k) {
                EncPass ps;
                ps.rate = r.rate[k];
                ps.len = r.rate[k] - (k ? r.rate[k - 1] : 0);
                // t1_enc_is_term_pass (t1.cpp:1131-1151)
                {
                    const int32_t bp = k == 0 ? (int32_t)r.numbps - 1 : (int32_t)r.numbps - 2 - (int32_t)((k - 1) / 3);
                    const int pt = k == 0 ? 2 : (int)((k - 1) % 3);
                    ps.term = t1_pass_term(cp.cblksty, bp, pt, r.numbps);
                }
                ps.slope = 0;
                if (need_rc) {  // t1_encode_cblk's cumulative distortion (t1.cpp:1249-1254)
                    const int32_t bpno = k == 0 ? (int32_t)r.numbps - 1 : (int32_t)r.numbps - 2 - (int32_t)((k - 1) / 3);
                    cum += t1_wmsedec_at(wf, r.nmsedec[k], bpno);
                }
                ps.dd = cum;
                out[k] = ps;
            }
            // the simple PCRD's slope range over this block's passes, from
            // the records just written (pcrd_simple's own loop, TileEnc::slopes)
            block_slopes(cst[i], out);
            blk_disto[i] = cum;
        }
    });
    precs = out0;
    for (uint32_t i = 0; i < nblk; ++i) blen[i] = res[i].len;
}

// j2k_update_rates (j2k.cpp:2806-2926): layer ratios -> byte budgets per tile
void EncHost::tile_rates(const Rect &tr, uint32_t ntp, double *rates) const {
    const uint32_t L = cp.numlayers;
    const double header_size = (double)mainhdr.size();
    const double bits_empty = 8.0 * cp.dx[0] * cp.dy[0], size_pixel = (double)nc * cp.prec[0];
    const uint32_t width = iw, height = ih;
    const double offset = (double)(cp.tp_on ? (float)((ntp - 1) * 14) : 0.0f) / L;
    const uint64_t npix = (uint64_t)tr.w() * tr.h();
    for (uint32_t k = 0; k < L; ++k) {
        rates[k] = cp.rates[k];
        if (rates[k] > 0.0f) rates[k] = (size_pixel * (double)npix) / (rates[k] * bits_empty) - offset;
    }
    rates[L] = 0;
    const double sot_adjust = ((double)npix * header_size) / ((double)width * height);
    double *r = rates;
    if (*r > 0.0) {
        *r -= sot_adjust;
        if (*r < 30.0f) *r = 30.0f;
    }
    ++r;
    const uint32_t last_res = L - 1;
    for (uint32_t k = 1; k < last_res; ++k) {
        if (*r > 0.0) {
            *r -= sot_adjust;
            if (*r < *(r - 1) + 10.0) *r = (*(r - 1)) + 20.0;
        }
        ++r;
    }
    if (*r > 0.0) {
        *r -= (sot_adjust + 2.0);
        if (*r < *(r - 1) + 10.0) *r = (*(r - 1)) + 20.0;
    }
}

// Tier-2 + headers on the host (j2k_encode :2059, j2k_post_write_tile
// :2196, T2::encode_packets): only header BITS are produced here; the
// code-block bytes never visit the host -- a gather kernel assembles the
// codestream in HBM and one D2H copies it into the pinned output buffer.
// finish_begin(): the main header and the rate allocator's tile bound;
// finish_tile(ti): one tile's tile-parts into its own header blob and plan;
// finish_end(): those appended in tile order, TLM and EOC.
int EncHost::finish_begin() {
    hdr.v.reserve(batch ? 4096 : 1 << 20);
    plan.reserve(nblk + 64);
    write_main_header(mainhdr, cp, &tlm_at, total_tile_parts);
    if (parts & GRKGPU_PART_HEADER) {
        hdr.putn(mainhdr.v.data(), mainhdr.size());
        plan.push_back({0, (uint32_t)hdr.size(), 0});
    }
    // tile buffer bound for the rate allocator (j2k_post_write_tile :2196-2222,
    // j2k_get_specific_header_sizes :4346-4366, then SOT / POC / SOD / EOC room)
    const bool cinema = cp.rsiz == RSIZ_CINEMA_2K || cp.rsiz == RSIZ_CINEMA_4K;
    {
        uint64_t ts = 0;
        for (uint32_t k = 0; k < nc; ++k) ts += (uint64_t)cp.tdx * cp.tdy * cp.prec[k];
        ts = (uint64_t)((double)ts * 0.1625);
        uint32_t max_tp = 0;
        for (auto &v : tp_counts) {
            uint32_t n = 0;
            for (uint32_t x : v) n += x;
            max_tp = std::max(max_tp, n);
        }
        uint64_t spec = 12ull * max_tp;
        if (!cinema) {
            const uint64_t coc = 6 + ((cp.csty & CSTY_PRT) ? 5 + cp.numres : 5);
            spec += (uint64_t)(nc - 1) * coc * 2;
        }
        spec += 4 + 9ull * num_poc_entries(cp);
        ts += spec;
        if (ts < 256ull * nc) ts = 256ull * nc;
        const uint64_t pocsz = (!cinema && cp.numpocs) ? 4 + (5 + 2 * (nc <= 256 ? 1 : 2)) * cp.numpocs : 0;
        tile_bound = ts - 12 - pocsz - 4;
    }
    // Tiles are independent in rate control and Tier-2 (their blocks, layer
    // records and packet state are disjoint): each tile's tile-parts are
    // formed on the host pool into its own header blob and plan, then
    // appended in tile order (header runs rebased onto the shared blob).
    touts.clear();
    touts.resize(tiles.size());
    return GRKGPU_OK;
}

void EncHost::finish_tile(size_t ti) {
    const uint32_t L = cp.numlayers;
    const bool cinema = cp.rsiz == RSIZ_CINEMA_2K || cp.rsiz == RSIZ_CINEMA_4K;
    Tile &tile = tiles[ti];
    TileOut &to = touts[ti];
    TileEnc tenc;
    tenc.tile = &tile;
    tenc.cblk = &cst;
    tenc.passes = precs;
    tenc.layers = &layers;
    tenc.slopes = true;  // the pass-record fill above computed every block's slope range
    init_enc_pocs(cp, tenc);
    CodingParams cpt = cp;
    uint32_t ntp = 0;
    for (uint32_t v : tp_counts[tile.index]) ntp += v;
    tile_rates(tile.r, ntp, cpt.rates);
    tenc.distotile = 0;
    for (auto &tc : tile.comps) for_each_cblk(tc, [&](Band &, Cblk &cb) { tenc.distotile += blk_disto[cb.gidx]; });
    const double tr0 = now_ms();
    if (!rate_allocate(cpt, tenc, tile_bound, &to.rs)) { to.ok = false; return; }
    const double tp0 = now_ms();
    to.rate_ms = tp0 - tr0;
    // The tile-parts' packets (T2::encode_packets per tile-part,
    // T2.cpp:64-125).  Tile-parts whose packets touch disjoint
    // precincts (tile-parts split by component or resolution, no POC
    // revisiting a precinct: the cinema profiles) are independent --
    // a packet header's state is its precinct's tag trees and its
    // code-blocks' inclusion records -- and are written in parallel,
    // each from its own SOP packet number; the bytes are the same.
    struct TpOut {
        uint32_t pino, tpn, packno0 = 0;
        std::vector<PacketId> order;
        ByteBuf hdr;
        std::vector<PlanItem> plan;
    };
    std::vector<TpOut> tps;
    for (uint32_t pino = 0; pino < tenc.pocs.size(); ++pino)
        for (uint32_t tpn = 0; tpn < tp_counts[tile.index][pino]; ++tpn) {
            tps.push_back(TpOut{pino, tpn});
            encode_packet_order(cpt, tenc, pino, tpn, tps.back().order);
        }
    bool disjoint = tps.size() > 1;
    {
        std::vector<int32_t> owner;  // precinct -> tile-part
        std::vector<std::vector<uint32_t>> pb(nc);  // first precinct index of (component, resolution)
        uint32_t np = 0;
        for (uint32_t k = 0; k < nc; ++k) {
            pb[k].resize(tile.comps[k].numres);
            for (uint32_t r = 0; r < tile.comps[k].numres; ++r) {
                pb[k][r] = np;
                np += tile.comps[k].res[r].pw * tile.comps[k].res[r].ph;
            }
        }
        owner.assign(np, -1);
        uint32_t packno = 0;
        for (size_t j = 0; j < tps.size() && disjoint; ++j) {
            tps[j].packno0 = packno;
            for (auto &pk : tps[j].order) {
                if (pk.layno >= L) continue;
                ++packno;
                int32_t &o = owner[pb[pk.compno][pk.resno] + pk.precno];
                if (o >= 0 && o != (int32_t)j) { disjoint = false; break; }
                o = (int32_t)j;
            }
        }
    }
    auto write_tp = [&](TpOut &t, TileEnc &te) {
        for (auto &pk : t.order)
            if (pk.layno < L) write_packet(cpt, te, pk, t.hdr, t.plan);
    };
    if (disjoint) {
        host_parallel_for(tps.size(), 1, [&](size_t j0, size_t j1) {
            for (size_t j = j0; j < j1; ++j) {
                TileEnc te = tenc;  // shares the tile's state; its own packet counter
                te.packno = tps[j].packno0;
                write_tp(tps[j], te);
            }
        });
    } else {
        for (auto &t : tps) write_tp(t, tenc);
    }
    uint32_t tpno = 0;
    ByteBuf &th = to.hdr;
    for (auto &t : tps) {
        const size_t sot = th.size();
        th.put16(0xFF90); th.put16(10); th.put16(tile.index); th.put32(0); th.put8(tpno); th.put8(ntp);
        if (tpno == 0 && !cinema && cp.numpocs) write_poc(th, cpt);
        th.put16(0xFF93);
        to.plan.push_back({sot, (uint32_t)(th.size() - sot), 0});
        const size_t first = to.plan.size() - 1;
        const uint64_t base = th.size();
        th.putn(t.hdr.v.data(), t.hdr.size());
        for (PlanItem it : t.plan) {
            if (it.kind == 0) it.src += base;
            to.plan.push_back(it);
        }
        uint64_t psot = 0;
        for (size_t i = first; i < to.plan.size(); ++i) psot += to.plan[i].len;
        th.set32(sot + 6, (uint32_t)psot);  // Psot (j2k.cpp:2418-2426)
        if (cinema) {
            to.tlm.push_back((uint8_t)tile.index);
            for (int b = 3; b >= 0; --b) to.tlm.push_back((uint8_t)(psot >> (8 * b)));
        }
        ++tpno;
    }
    to.packet_ms = now_ms() - tp0;
}

int EncHost::finish_end() {
    std::vector<uint8_t> tlm;  // TLM records (j2k_update_tlm, j2k.cpp:6649-6660)
    for (auto &to : touts) {
        if (!to.ok) return set_err(GRKGPU_EINVAL, "rate allocation failed");
        t_rate += to.rate_ms;
        t_packets += to.packet_ms;
        rsum.probes += to.rs.probes;
        rsum.skipped += to.rs.skipped;
        rsum.evals += to.rs.evals;
        rsum.sims += to.rs.sims;
        rsum.form_ms += to.rs.form_ms;
        rsum.sim_ms += to.rs.sim_ms;
        const uint64_t base = hdr.size();
        hdr.putn(to.hdr.v.data(), to.hdr.size());
        for (PlanItem it : to.plan) {
            if (it.kind == 0) it.src += base;
            plan.push_back(it);
        }
        tlm.insert(tlm.end(), to.tlm.begin(), to.tlm.end());
    }
    if ((parts & GRKGPU_PART_HEADER) && tlm_at && tlm.size() == 5ull * total_tile_parts)
        memcpy(hdr.v.data() + tlm_at, tlm.data(), tlm.size());  // j2k_write_updated_tlm (:2555-2577)
    if (parts & GRKGPU_PART_EOC) {
        size_t eoc = hdr.size();
        hdr.put16(0xFFD9);
        plan.push_back({eoc, 2, 0});
    }
    return GRKGPU_OK;
}
}  // namespace

// The device stages of an encode: compress_impl runs them over its one
// image's tables, the batch encode over its merged ones.
//
// A run of the block table coded in one style (a Tier-1 launch set each): its
// images (indices into the caller's EncHost array) in table order, the
// rate-controlled ones first -- the run's first nrc blocks.  scr0 / ord0: its
// place in ctx->scratch (bytes) and ctx->t1order (words); rc0: its first
// block among the rate-controlled ones of all runs.
struct StyGroup {
    uint32_t sty = 0, b0 = 0, n = 0, nrc = 0, maxdepth = 1, rc0 = 0;
    uint64_t scr0 = 0, ord0 = 0;
    std::vector<uint32_t> items;
};

// the kernel launches and fills launch_t1_encode issues for n blocks
static uint32_t t1_encode_launch_count(uint32_t n) {
    if (!n) return 0;
    return 3 + (dwt_options().t1_enc_sort && n > 64 ? 4 : 0);
}

// the buffers of an encode of nblk blocks that both paths size alike
static int enc_ensure(grkgpu_ctx *c, uint64_t arena, uint64_t llarena, uint64_t scr_bytes, uint64_t ord_words,
                      uint64_t out_total, uint64_t sym_total, uint32_t nblk) {
    HIPCHK(c->work.ensure(arena * 4 + 256));
    HIPCHK(c->coef.ensure(arena * 4 + 256));
    HIPCHK(c->ll.ensure(llarena * 4 + 256));
    HIPCHK(c->scratch.ensure((size_t)scr_bytes + 256));
    HIPCHK(c->t1order.ensure((size_t)ord_words * 4 + 256));
    HIPCHK(c->mqout.ensure(out_total + 256));
    HIPCHK(c->blocks.ensure((size_t)nblk * sizeof(EncBlock) + 256));
    HIPCHK(c->results.ensure((size_t)nblk * sizeof(EncResult) + 256));
    HIPCHK(c->h_results.ensure((size_t)nblk * sizeof(EncResult) + 256));
    HIPCHK(c->h_blocks.ensure((size_t)nblk * sizeof(EncBlock) + 256));
    HIPCHK(c->sym.ensure(sym_total + 256));
    HIPCHK(c->symoff.ensure(((size_t)nblk + 1) * 8 + 256));
    HIPCHK(c->h_symoff.ensure(((size_t)nblk + 1) * 8 + 256));
    return GRKGPU_OK;
}

// The Tier-1 stage of an encode, from the table uploads to the results on the
// host (event 4 after the last coder launch).  In: nblk EncBlocks and nblk + 1
// symbol-stream offsets staged in h_blocks / h_symoff, the runs `sg` over
// them, H = the images the runs' items index; nrc / slots = the
// rate-controlled blocks and their pass-record slots over all runs.  *nl
// grows by the launches and fills issued.
// With rate control the pass records are formed on the device
// (launch_pass_records): the host fills each block's distortion factor and
// record slots while the GPU codes (h_pinfo: nrc factors, then the slots, nrc
// + one end per run, run g's from rc0 + g), and only the records (h_precs) and
// per-block summaries (h_psum) come back.  Without it the host forms them
// from the coders' results (h_results, rates only: no distortion to weigh).
static int enc_t1_stage(grkgpu_ctx *c, const std::vector<StyGroup> &sg, const EncHost *H, uint32_t nblk, uint32_t nrc,
                        uint64_t slots, uint32_t *nl) {
    hipStream_t s = c->stream;
    const bool lone = lone_call();
    HIPCHK(hipMemcpyAsync(c->blocks.p, c->h_blocks.p, (size_t)nblk * sizeof(EncBlock), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->symoff.p, c->h_symoff.p, ((size_t)nblk + 1) * 8, hipMemcpyHostToDevice, s));
    for (const StyGroup &g : sg) {
        HIPCHK(launch_t1_encode(c->blocks.as<EncBlock>() + g.b0, g.n, c->coef.as<int32_t>(),
                                c->scratch.as<uint8_t>() + g.scr0, c->sym.as<uint8_t>(), c->symoff.as<uint64_t>() + g.b0,
                                g.maxdepth, c->mqout.as<uint8_t>(), c->results.as<EncResult>() + g.b0, s, g.sty,
                                lone ? lone_bpw(g.n) : 0, c->t1order.as<uint32_t>() + g.ord0));
        *nl += t1_encode_launch_count(g.n);
    }
    const size_t p0_words = (size_t)nrc + sg.size();
    if (nrc) {
        HIPCHK(c->h_pinfo.ensure(((size_t)nrc + p0_words) * 8 + 256));
        HIPCHK(c->pinfo.ensure(((size_t)nrc + p0_words) * 8 + 256));
        double *wf = c->h_pinfo.as<double>();
        uint64_t *p0 = (uint64_t *)(wf + nrc);
        for (size_t gi = 0; gi < sg.size(); ++gi) {
            const StyGroup &g = sg[gi];
            uint64_t sl = 0;
            for (uint32_t i : g.items) {
                const EncHost &h = H[i];
                if (!h.need_rc) continue;
                sl = h.slot0;
                for (uint32_t q = 0; q < h.nblk; ++q) {
                    wf[h.rcb0 + q] = h.wfac(q);
                    p0[h.rcb0 + gi + q] = sl;
                    sl += h.pcap[q];
                }
            }
            p0[(size_t)g.rc0 + gi + g.nrc] = g.nrc ? sl : 0;
        }
        HIPCHK(hipMemcpyAsync(c->pinfo.p, c->h_pinfo.p, ((size_t)nrc + p0_words) * 8, hipMemcpyHostToDevice, s));
    }
    for (const StyGroup &g : sg) {
        if (!g.nrc) continue;
        HIPCHK(launch_t1_dist(c->blocks.as<EncBlock>() + g.b0, g.n, g.maxdepth, c->coef.as<int32_t>(),
                              c->scratch.as<uint8_t>() + g.scr0, c->results.as<EncResult>() + g.b0, s));
        ++*nl;
    }
    HIPCHK(hipEventRecord(c->ev[4], s));
    if (nrc) {
        const size_t sum_bytes = ((size_t)nrc * sizeof(PassSum) + 255) & ~(size_t)255;
        HIPCHK(c->precs.ensure(sum_bytes + slots * sizeof(DevPass) + 256));
        HIPCHK(c->h_psum.ensure(sum_bytes + 256));
        HIPCHK(c->h_precs.ensure(slots * sizeof(DevPass) + 256));
        PassSum *dsum = c->precs.as<PassSum>();
        DevPass *dpass = (DevPass *)(c->precs.as<uint8_t>() + sum_bytes);
        const double *dwf = c->pinfo.as<double>();
        const uint64_t *dp0 = (const uint64_t *)(dwf + nrc);
        for (size_t gi = 0; gi < sg.size(); ++gi) {
            const StyGroup &g = sg[gi];
            if (!g.nrc) continue;
            HIPCHK(launch_pass_records(c->blocks.as<EncBlock>() + g.b0, c->results.as<EncResult>() + g.b0, dwf + g.rc0,
                                       dp0 + g.rc0 + gi, g.nrc, g.sty, dpass, dsum + g.rc0, s));
            ++*nl;
        }
        HIPCHK(hipMemcpyAsync(c->h_psum.p, dsum, (size_t)nrc * sizeof(PassSum), hipMemcpyDeviceToHost, s));
        if (slots) HIPCHK(hipMemcpyAsync(c->h_precs.p, dpass, slots * sizeof(DevPass), hipMemcpyDeviceToHost, s));
    }
    for (const StyGroup &g : sg) {  // the other blocks' results, rates only
        if (g.n == g.nrc) continue;
        const size_t o = ((size_t)g.b0 + g.nrc) * sizeof(EncResult);
        HIPCHK(hipMemcpy2DAsync(c->h_results.as<uint8_t>() + o, sizeof(EncResult), c->results.as<uint8_t>() + o,
                                sizeof(EncResult), ENC_RESULT_RATE_BYTES, g.n - g.nrc, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    return GRKGPU_OK;
}

// One image's PlanItems appended to a gather list, its bytes from `total` on
// (advanced), its header runs `hbase` into the blob the list is gathered from.
static void gather_append(std::vector<GatherItem> &gi, const std::vector<PlanItem> &plan, uint64_t hbase, uint64_t &total) {
    for (const PlanItem &pi : plan) {
        if (pi.len) gi.push_back({pi.kind == 0 ? pi.src + hbase : pi.src, total, pi.len, pi.kind});
        total += pi.len;
    }
}

// The output stage of an encode: the gather list and the header blob to the
// device, the gather kernel (header runs from the blob, code-block bytes from
// the MQ slab, assembled in HBM) and one D2H of the `total` bytes into the
// pinned output buffer, events 5..7 around them.  out_lk (not yet locked) is
// the caller's lock on ctx->out_mu: taken here before h_out is chosen, for
// the caller to hold while it hands h_out's bytes out.
static int enc_output_stage(grkgpu_ctx *c, const std::vector<GatherItem> &gi, const ByteBuf &hdr, uint64_t total,
                            std::unique_lock<std::mutex> &out_lk, uint32_t *nl) {
    hipStream_t s = c->stream;
    HIPCHK(c->gather.ensure(gi.size() * sizeof(GatherItem) + hdr.size() + 512));
    HIPCHK(c->h_gather.ensure(gi.size() * sizeof(GatherItem) + hdr.size() + 512));
    HIPCHK(c->packed.ensure(total + 256));
    out_lk.lock();
    if (!c->h_out.p && !c->out_spare.empty()) {  // taken by a view: reuse a given-back buffer
        auto big = std::max_element(c->out_spare.begin(), c->out_spare.end(),
                                    [](const auto &a, const auto &b) { return a.second < b.second; });
        c->h_out.p = big->first;
        c->h_out.cap = big->second;
        c->out_spare.erase(big);
    }
    HIPCHK(c->h_out.ensure(total + 256));
    const size_t gbytes = gi.size() * sizeof(GatherItem);
    const size_t hoff = (gbytes + 255) & ~(size_t)255;
    memcpy(c->h_gather.p, gi.data(), gbytes);
    memcpy(c->h_gather.as<uint8_t>() + hoff, hdr.v.data(), hdr.size());
    HIPCHK(hipEventRecord(c->ev[5], s));
    HIPCHK(hipMemcpyAsync(c->gather.p, c->h_gather.p, hoff + hdr.size(), hipMemcpyHostToDevice, s));
    if (!gi.empty()) {  // (launch_gather issues nothing for an empty list)
        HIPCHK(launch_gather(c->gather.as<uint8_t>() + hoff, c->mqout.as<uint8_t>(), c->gather.as<GatherItem>(),
                             (uint32_t)gi.size(), c->packed.as<uint8_t>(), s));
        ++*nl;
    }
    HIPCHK(hipEventRecord(c->ev[6], s));
    // (a batch's pad bytes before a stream's 16-byte boundary are copied as they are: no item's cs / len covers them)
    if (total) HIPCHK(hipMemcpyAsync(c->h_out.p, c->packed.p, total, hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(c->ev[7], s));
    HIPCHK(hipStreamSynchronize(s));
    return GRKGPU_OK;
}

// The statistics of an encode (grkgpu_get_stats) from the stage events and the
// host's clock.  tail: what the calls that write a codestream add (null:
// grkgpu_encode_blocks, which stops after Tier-1 -- those fields stay zero).
struct EncStatsTail {
    double t_t2, t_t2_end, t_passrec, t_rate, t_packets;
    uint64_t cs_bytes;
    const RateStats &rs;
};
static void fill_enc_stats(grkgpu_ctx *c, double t_start, double t_end, uint32_t nblk, uint64_t nsym,
                           const EncStatsTail *tail) {
    grkgpu_stats &st = c->stats;
    memset(&st, 0, sizeof(st));
    hipEventElapsedTime(&st.h2d_ms, c->ev[0], c->ev[1]);
    hipEventElapsedTime(&st.dcshift_mct_ms, c->ev[1], c->ev[2]);
    hipEventElapsedTime(&st.dwt_ms, c->ev[2], c->ev[3]);
    hipEventElapsedTime(&st.t1_ms, c->ev[3], c->ev[4]);
    if (tail) {
        hipEventElapsedTime(&st.gather_ms, c->ev[5], c->ev[6]);
        hipEventElapsedTime(&st.d2h_ms, c->ev[6], c->ev[7]);
    }
    log_collect(c);
    st.total_ms = (float)(t_end - t_start);
    st.num_cblks = nblk;
    st.mq_symbols = nsym;
    if (!tail) return;
    st.host_t2_ms = (float)(tail->t_t2_end - tail->t_t2);
    st.cs_bytes = tail->cs_bytes;
    st.rate_ms = (float)tail->t_rate;
    st.packet_ms = (float)tail->t_packets;
    st.rate_probes = tail->rs.probes;
    st.rate_probes_skipped = tail->rs.skipped;
    st.rate_block_evals = tail->rs.evals;
    st.rate_precinct_sims = tail->rs.sims;
    st.rate_form_ms = (float)tail->rs.form_ms;
    st.rate_sim_ms = (float)tail->rs.sim_ms;
    st.passrec_ms = (float)tail->t_passrec;
}

// Encode tiles [tb, te) (a tile shard: j2k_encode's per-tile loop,
// j2k.cpp:2088-2111) and emit [main header][their tile-parts][EOC] per `parts`.
// export_blocks: stop after Tier-1 and hand the per-code-block results to the
// caller instead of writing a codestream (grkgpu_encode_blocks).
//
// row0 / nrows: the planes hold only image rows [row0, row0 + nrows) (a tile-
// row shard: a rank loads just the rows of its tiles); nrows = 0: all rows.
static int compress_impl(grkgpu_ctx *c, const grkgpu_image_desc *img, const grkgpu_cparams *p,
                         const void *const *planes, int planes_on_device, int32_t fmt_in, const uint8_t **view,
                         size_t *outlen,
                         uint32_t tb = 0, uint32_t te = 0xffffffffu, uint32_t parts = GRKGPU_PART_ALL,
                         bool export_blocks = false, int force_dist = 0, uint32_t row0 = 0, uint32_t nrows = 0,
                         uint32_t col0 = 0, uint32_t ncols = 0, const std::vector<uint8_t> *jp2_boxes = nullptr) {
    if (!c || !planes) return set_err(GRKGPU_EINVAL, "null argument");
    ActiveCall active;
    // the host half (EncHost): every check that needs no device, the tile
    // geometry and the block tables
    EncHost H;
    H.img = img; H.p = p; H.fmt_in = fmt_in;
    H.tb = tb; H.te = te; H.parts = parts;
    H.row0 = row0; H.nrows = nrows; H.col0 = col0; H.ncols = ncols;
    H.export_blocks = export_blocks; H.force_dist = force_dist;
    double t_start = now_ms();
    int rc = H.begin();
    if (rc) return rc;
    const CodingParams &cp = H.cp;
    tb = H.tb; te = H.te;
    const int32_t fmt = H.fmt, lfmt = H.lfmt;
    const bool il = H.il, big = H.big, mixed = H.mixed, need_rc = H.need_rc;
    const uint32_t sb = H.sb, nc = H.nc, pw = H.pw, nblk = H.nblk, maxdepth = H.maxdepth;
    const uint64_t plane = H.plane, arena = H.arena, llarena = H.llarena, sym_total = H.sym_total,
                   out_total = H.out_total;
    const Rect *prect = H.prect;
    const uint64_t *poff = H.poff;
    std::vector<Tile> &tiles = H.tiles;
    const std::vector<uint64_t> &lloff = H.lloff, &symoff = H.symoff;
    const std::vector<EncBlock> &eb = H.eb;
    const std::vector<EncHost::BlkInfo> &binfo = H.binfo;
    auto plane_org = [&](uint32_t k, const TileComp &tc) { return H.plane_org(k, tc); };
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    rc = enc_ensure(c, arena, llarena, t1e_scratch_bytes(nblk, maxdepth), t1_order_words(nblk), out_total, sym_total, nblk);
    if (rc) return rc;

    HIPCHK(hipEventRecord(c->ev[0], s));
    // input planes on the device, as the caller's samples (widened to int32
    // by the first kernel that reads them)
    SrcPlanes src{};
    if (planes_on_device) {
        for (uint32_t k = 0; k < (il ? 1u : nc); ++k) src.p[k] = planes[k];
    } else if (il) {  // one copy of the pixels held: rows * columns * components samples
        HIPCHK(c->img.ensure(poff[nc] * sb + 256));
        src.p[0] = c->img.as<uint8_t>();
        HIPCHK(hipMemcpyAsync((void *)src.p[0], planes[0], poff[nc] * sb, hipMemcpyHostToDevice, s));
    } else {
        HIPCHK(c->img.ensure(poff[nc] * sb + 256));
        for (uint32_t k = 0; k < nc; ++k) {
            src.p[k] = c->img.as<uint8_t>() + poff[k] * sb;
            HIPCHK(hipMemcpyAsync((void *)src.p[k], planes[k], (poff[k + 1] - poff[k]) * sb, hipMemcpyHostToDevice,
                                  s));
        }
    }
    // sample `off` (an element offset in the component's plane: a pixel offset) of component k
    auto src_at = [&](uint32_t k, uint64_t off) {
        return il ? (const void *)((const uint8_t *)src.p[0] + (off * nc + k) * sb)
                  : (const void *)((const uint8_t *)src.p[k] + off * sb);
    };
    HIPCHK(hipEventRecord(c->ev[1], s));
    ShiftArr sh{};
    for (uint32_t k = 0; k < nc; ++k) sh.v[k] = cp.shift[k];
    // The DC shift + RCT of a 3-component 5/3 tile is fused into its first
    // DWT level (k_dwt_fwd_mct3: one wavefront reads the three image planes
    // once and lifts the three components of its window): 162 us instead of
    // 132 (MCT pass) + 133 (level 0) on the 8K frame.  The 9/7 (ICT) triple
    // is left separate: fused 229 us vs 132 + 145, but the separate level-0
    // launch is the DWT whose roofline the bench reports.
    // grkgpu_dwt_options.fuse_level0 = 0 / 1 forces it off / on (1: also 9/7
    // and single components, DC shift in the loads).  Requires every
    // tile-component to be decomposed at least once and to span its tile.
    const int fo = dwt_options().fuse_level0;
    bool fuse = fo >= 0 ? fo != 0 : (!cp.irrev && cp.mct == 1 && nc == 3);
    for (auto &tile : tiles)
        for (uint32_t k = 0; k < nc; ++k) {
            const TileComp &tc = tile.comps[k];
            fuse = fuse && tc.numres >= 2 && tc.r.w() == tile.r.w() && tc.r.h() == tile.r.h();
        }
    if ((cp.mct && nc != 3) || cp.mct == 2) fuse = false;  // MCT over more than 3 components, custom MCT: separate pass
    if (fmt == SMP_I8 || fmt == SMP_I16) fuse = false;  // the fused loads read int32, u16 or u8 samples
    if (big) fuse = false;                               // ... in host byte order
    // ... and interleaved pixels only as an MCT triple (k_dwt_fwd_mct3); the
    // single-component fused loads stay planar: other pixels take the separate pass
    if (il && !(cp.mct == 1 && nc == 3 && (uintptr_t)src.p[0] % sb == 0)) fuse = false;
    DwtPlan dplan;
    dplan.fused0 = fuse;
    dplan.mct3 = fuse && cp.mct == 1 && nc == 3;
    for (auto &tile : tiles)
        for (uint32_t k = 0; k < nc; ++k) {
            const TileComp &tc = tile.comps[k];
            const size_t before = dplan.levels.empty() ? 0 : dplan.levels[0].size();
            dwt_plan_tc(dplan, tc, c->work.as<int32_t>() + tc.arena_off, c->coef.as<int32_t>() + tc.arena_off,
                        c->ll.as<int32_t>() + lloff[(tile.index - tb) * nc + k], cp.irrev, false);
            if (!fuse || dplan.levels.empty() || dplan.levels[0].size() == before) continue;
            DwtJob &j = dplan.levels[0].back();
            const uint64_t org = plane_org(k, tc);  // fused: no subsampling, every plane alike
            const bool mct3 = cp.mct == 1 && nc >= 3 && k < 3;
            for (uint32_t i = 0; i < 3; ++i) {
                const uint32_t pk = mct3 ? i : k;
                j.src[i] = src_at(pk, org);
                j.shift[i] = cp.shift[pk];
            }
            j.src_stride = il ? pw * nc : pw;
            j.src_pitch = il ? (int32_t)nc : 1;
            j.src_bytes = (uint32_t)std::min<uint64_t>((plane - org) * (il ? nc : 1) * sb, 0xffffffffu);
            j.src_fmt = fmt;
            j.mct_mode = mct3 ? (cp.irrev ? 3 : 2) : 1;
            j.comp = (int32_t)k;
            bool al = (j.src_stride & 1) == 0;
            for (uint32_t i = 0; i < (il ? 1u : 3u); ++i) al = al && ((uintptr_t)j.src[i] & (2 * sb - 1)) == 0;
            j.src_vec = al ? 1 : 0;
        }
    dplan.fmt = fmt;
    dplan.pixels = il && fuse;
    HIPCHK(dwt_upload(dplan, c->dwtjobs, c->h_dwtjobs, cp.irrev, s));
    for (auto &tile : tiles) {
        if (fuse) break;
        if (mixed) {  // one launch per tile-component, each on its own grid (no MCT, j2k.cpp:1963-1971)
            for (uint32_t k = 0; k < nc; ++k) {
                const TileComp &tc = tile.comps[k];
                SrcPlanes tsrc{};
                PlanePtrs tdst{};
                ShiftArr sk{};
                tsrc.p[0] = src_at(k, plane_org(k, tc));
                tdst.p[0] = c->work.as<int32_t>() + tc.arena_off;
                sk.v[0] = sh.v[k];
                HIPCHK(launch_dcshift_mct_fwd(tsrc, fmt | (big ? SMP_BIG_ENDIAN : 0), prect[k].w(), tdst, tc.r.w(),
                                              tc.r.h(), 1, sk, 0, cp.irrev, s));
            }
            continue;
        }
        // every component on one grid (no subsampling, or the same dx / dy
        // for all): one launch over the tile, MCT included
        SrcPlanes tsrc{};
        PlanePtrs tdst{};
        for (uint32_t k = 0; k < nc; ++k) {
            tsrc.p[k] = src_at(k, plane_org(k, tile.comps[k]));
            tdst.p[k] = c->work.as<int32_t>() + tile.comps[k].arena_off;
        }
        const Rect &tcr = tile.comps[0].r;
        const uint32_t spw = prect[0].w() * (il ? nc : 1);  // interleaved: tsrc.p[0] = the tile's first pixel
        if (cp.mct == 2) {
            MctMatrix mm{};
            memcpy(mm.c, cp.mct_coding, sizeof(int32_t) * nc * nc);
            HIPCHK(launch_dcshift_mct_custom(tsrc, lfmt, spw, tdst, tcr.w(), tcr.h(), nc, sh, mm, s));
        } else {
            HIPCHK(launch_dcshift_mct_fwd(tsrc, lfmt, spw, tdst, tcr.w(), tcr.h(), nc, sh, cp.mct, cp.irrev, s));
        }
    }
    HIPCHK(hipEventRecord(c->ev[2], s));
    c->ltimes.clear();
    c->lidx.clear();
    LaunchLog llog{&c->lev, &c->ltimes, &c->lidx};
    HIPCHK(dwt_launch(dplan, c->dwtjobs, cp.irrev, false, s, c->launch_timing ? &llog : nullptr));
    HIPCHK(hipEventRecord(c->ev[3], s));
    memcpy(c->h_blocks.p, eb.data(), (size_t)nblk * sizeof(EncBlock));
    memcpy(c->h_symoff.p, symoff.data(), symoff.size() * 8);
    // one run of the image's style: all of its blocks rate-controlled, or none
    // (then, or with no block at all, the host forms the pass records)
    const bool dev_rec = need_rc && nblk;
    std::vector<StyGroup> sg(1);
    sg[0].sty = cp.cblksty; sg[0].n = nblk; sg[0].nrc = need_rc ? nblk : 0; sg[0].maxdepth = maxdepth;
    sg[0].items.push_back(0);
    uint32_t nl = 0;  // (the batch's launch count: not reported by this call)
    rc = enc_t1_stage(c, sg, &H, nblk, sg[0].nrc, H.ptotal, &nl);
    if (rc) return rc;
    const EncResult *res = c->h_results.as<EncResult>();

    // Tier-2 + headers on the host (j2k_encode :2059, j2k_post_write_tile
    // :2196, T2::encode_packets): only header BITS are produced here; the
    // code-block bytes never visit the host -- a gather kernel assembles the
    // codestream in HBM and one D2H copies it into the pinned output buffer.
    double t_t2 = now_ms();
    if (dev_rec) {
        rc = H.records_dev(c->h_psum.as<PassSum>(), (const uint64_t *)(c->h_pinfo.as<double>() + nblk),
                           c->h_precs.as<EncPass>());
        if (rc) return rc;
    } else {
        rc = H.records_host_count(res);
        if (rc) return rc;
        std::vector<EncPass> &passes = c->enc_passes;  // host-formed records: [0, npass) filled below
        if (passes.size() < H.npass) passes.resize(H.npass);
        H.records_host_fill(res, passes.data());
    }
    const std::vector<EncCblkState> &cst = H.cst;
    const std::vector<uint32_t> &blen = H.blen;
    const EncPass *precs = H.precs;  // the records Tier-2 reads: the host-formed ones, or the device's
    const uint64_t npass = H.npass, nsym = H.nsym;
    const double t_passrec = now_ms() - t_t2;
    if (export_blocks) {
        // the MQ slab to pinned host memory, then one record per block
        HIPCHK(c->h_slab.ensure(out_total + 256));
        if (out_total) HIPCHK(hipMemcpyAsync(c->h_slab.p, c->mqout.p, out_total, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        c->bexp.assign(nblk, grkgpu_block_info{});
        c->bexp_rate.resize((size_t)npass + 1);
        c->bexp_dist.resize((size_t)npass + 1);
        for (size_t k = 0; k < npass; ++k) {
            c->bexp_rate[k] = precs[k].rate;
            c->bexp_dist[k] = precs[k].dd;
        }
        for (uint32_t i = 0; i < nblk; ++i) {
            grkgpu_block_info &o = c->bexp[i];
            const EncHost::BlkInfo &bi = binfo[i];
            o.tileno = bi.tileno; o.compno = bi.compno; o.resno = bi.resno; o.bandno = bi.orient;
            o.precno = bi.precno; o.cblkno = bi.cblkno;
            o.x0 = bi.r.x0; o.y0 = bi.r.y0; o.x1 = bi.r.x1; o.y1 = bi.r.y1;
            o.numbps = cst[i].numbps;
            o.numpasses = cst[i].numpasses;
            o.len = blen[i];
            o.stepsize = bi.stepsize;
            o.data = c->h_slab.as<uint8_t>() + eb[i].out_off;
            o.rate = c->bexp_rate.data() + cst[i].pass0;
            o.distortion = c->bexp_dist.data() + cst[i].pass0;
        }
        c->bexp_coef.clear();
        for (auto &tile : tiles)
            for (uint32_t k = 0; k < nc; ++k)
                c->bexp_coef.push_back({tile.index, k, tile.comps[k].r.w(), tile.comps[k].r.h(), tile.comps[k].arena_off});
        fill_enc_stats(c, t_start, now_ms(), nblk, nsym, nullptr);
        return GRKGPU_OK;
    }
    rc = H.finish_begin();
    if (rc) return rc;
    host_parallel_for(tiles.size(), 1, [&](size_t t0, size_t t1) {
        for (size_t ti = t0; ti < t1; ++ti) H.finish_tile(ti);
    });
    rc = H.finish_end();
    if (rc) return rc;
    ByteBuf &hdr = H.hdr;
    std::vector<PlanItem> &plan = H.plan;
    if (jp2_boxes) {
        // grkgpu_jp2_compress: the file's boxes (ending in the jp2c box header)
        // are one more run of the header blob, gathered ahead of everything
        // else; the plan's total is the codestream's length, so jp2c's LBox
        // (jp2_write_jp2c, jp2.cpp:2075-2116) is known before the launch
        uint64_t cslen = 0;
        for (auto &pi : plan) cslen += pi.len;
        if (cslen + 8 >= (1ull << 32)) return set_err(GRKGPU_EUNSUPPORTED, "JP2: codestream too long for a 32-bit LBox");
        const size_t at = hdr.size();
        hdr.putn(jp2_boxes->data(), jp2_boxes->size());
        hdr.set32(at + jp2_boxes->size() - 8, (uint32_t)(cslen + 8));
        plan.insert(plan.begin(), PlanItem{at, (uint32_t)jp2_boxes->size(), 0});
    }
    // gather list: dst offsets = prefix sum of run lengths
    std::vector<GatherItem> gi;
    gi.reserve(plan.size());
    uint64_t total = 0;
    gather_append(gi, plan, 0, total);
    double t_t2_end = now_ms();
    std::unique_lock<std::mutex> out_lk(c->out_mu, std::defer_lock);
    rc = enc_output_stage(c, gi, hdr, total, out_lk, &nl);
    if (rc) return rc;
    double t_end = now_ms();
    *view = c->h_out.as<uint8_t>();
    *outlen = total;
    const EncStatsTail tail{t_t2, t_t2_end, t_passrec, H.t_rate, H.t_packets, total, H.rsum};
    fill_enc_stats(c, t_start, t_end, nblk, nsym, &tail);
    return GRKGPU_OK;
}

extern "C" int grkgpu_compress_view(grkgpu_ctx *c, const grkgpu_image_desc *img, const grkgpu_cparams *p,
                                    const int32_t *const *planes, int planes_on_device, const uint8_t **out,
                                    size_t *outlen) {
    if (!out || !outlen) return set_err(GRKGPU_EINVAL, "null argument");
    return compress_impl(c, img, p, (const void *const *)planes, planes_on_device, SMP_I32, out, outlen);
}

extern "C" int grkgpu_compress(grkgpu_ctx *c, const grkgpu_image_desc *img, const grkgpu_cparams *p,
                               const int32_t *const *planes, int planes_on_device, uint8_t **out, size_t *outlen) {
    if (!out || !outlen) return set_err(GRKGPU_EINVAL, "null argument");
    const uint8_t *v = nullptr;
    size_t n = 0;
    int rc = compress_impl(c, img, p, (const void *const *)planes, planes_on_device, SMP_I32, &v, &n);
    if (rc) return rc;
    uint8_t *o = (uint8_t *)malloc(n ? n : 1);
    if (!o) return set_err(GRKGPU_EINVAL, "out of host memory");
    memcpy(o, v, n);
    *out = o;
    *outlen = n;
    return GRKGPU_OK;
}

extern "C" int grkgpu_compress_ex(grkgpu_ctx *c, const grkgpu_image_desc *img, const grkgpu_cparams *p,
                                  const grkgpu_planes *in, uint32_t tile_begin, uint32_t tile_end, uint32_t parts,
                                  const uint8_t **out, size_t *outlen) {
    if (!in || !out || !outlen) return set_err(GRKGPU_EINVAL, "null argument");
    if (in->nrows == 0 && in->row0) return set_err(GRKGPU_EINVAL, "row0 without nrows");
    if (in->ncols == 0 && in->col0) return set_err(GRKGPU_EINVAL, "col0 without ncols");
    return compress_impl(c, img, p, in->planes, in->on_device, (int32_t)in->sample_fmt, out, outlen, tile_begin,
                         tile_end, parts, false, 0, in->row0, in->nrows, in->col0, in->ncols);
}

extern "C" int grkgpu_encode_blocks(grkgpu_ctx *c, const grkgpu_image_desc *img, const grkgpu_cparams *p,
                                    const int32_t *const *planes, int planes_on_device, int with_distortion,
                                    const grkgpu_block_info **blocks, uint32_t *nblocks) {
    if (!planes || !img) return set_err(GRKGPU_EINVAL, "null argument");
    grkgpu_planes pl;
    memset(&pl, 0, sizeof(pl));
    for (uint32_t k = 0; k < img->numcomps && k < GRKGPU_MAX_COMPS; ++k) pl.planes[k] = planes[k];
    pl.sample_fmt = GRKGPU_SAMPLE_I32;
    pl.on_device = planes_on_device;
    return grkgpu_encode_blocks_ex(c, img, p, &pl, with_distortion, blocks, nblocks);
}

extern "C" int grkgpu_encode_blocks_ex(grkgpu_ctx *c, const grkgpu_image_desc *img, const grkgpu_cparams *p,
                                       const grkgpu_planes *in, int with_distortion,
                                       const grkgpu_block_info **blocks, uint32_t *nblocks) {
    if (!in || !blocks || !nblocks) return set_err(GRKGPU_EINVAL, "null argument");
    if (in->nrows == 0 && in->row0) return set_err(GRKGPU_EINVAL, "row0 without nrows");
    if (in->ncols == 0 && in->col0) return set_err(GRKGPU_EINVAL, "col0 without ncols");
    int rc = compress_impl(c, img, p, in->planes, in->on_device, (int32_t)in->sample_fmt, nullptr, nullptr, 0,
                           0xffffffffu, GRKGPU_PART_ALL, true, with_distortion, in->row0, in->nrows, in->col0,
                           in->ncols);
    if (rc) return rc;
    *blocks = c->bexp.data();
    *nblocks = (uint32_t)c->bexp.size();
    return GRKGPU_OK;
}

extern "C" int grkgpu_encode_blocks_coefficients(grkgpu_ctx *c, uint32_t tileno, uint32_t compno, int32_t *dst,
                                                  uint32_t dst_stride) {
    if (!c || !dst) return set_err(GRKGPU_EINVAL, "null argument");
    for (const auto &r : c->bexp_coef) {
        if (r.tileno != tileno || r.compno != compno) continue;
        if (dst_stride < r.w) return set_err(GRKGPU_EINVAL, "dst_stride below the tile-component width");
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipMemcpy2DAsync(dst, (size_t)dst_stride * 4, c->coef.as<int32_t>() + r.off, (size_t)r.w * 4,
                                (size_t)r.w * 4, r.h, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return GRKGPU_OK;
    }
    return set_err(GRKGPU_EINVAL, "no such tile-component in the last grkgpu_encode_blocks call");
}

extern "C" int grkgpu_num_tiles(const grkgpu_image_desc *img, const grkgpu_cparams *p, uint32_t *ntiles) {
    if (!ntiles) return set_err(GRKGPU_EINVAL, "null argument");
    CodingParams cp;
    int rc = setup_params(img, p, cp);
    if (rc) return rc;
    *ntiles = cp.tw * cp.th;
    return GRKGPU_OK;
}

extern "C" int grkgpu_compress_tiles(grkgpu_ctx *c, const grkgpu_image_desc *img, const grkgpu_cparams *p,
                                     const int32_t *const *planes, int planes_on_device, uint32_t tile_begin,
                                     uint32_t tile_end, uint32_t parts, uint8_t **out, size_t *outlen) {
    if (!out || !outlen) return set_err(GRKGPU_EINVAL, "null argument");
    const uint8_t *v = nullptr;
    size_t n = 0;
    int rc = compress_impl(c, img, p, (const void *const *)planes, planes_on_device, SMP_I32, &v, &n, tile_begin,
                           tile_end, parts);
    if (rc) return rc;
    uint8_t *o = (uint8_t *)malloc(n ? n : 1);
    if (!o) return set_err(GRKGPU_EINVAL, "out of host memory");
    memcpy(o, v, n);
    *out = o;
    *outlen = n;
    return GRKGPU_OK;
}

extern "C" int grkgpu_compress_tile_rows(grkgpu_ctx *c, const grkgpu_image_desc *img, const grkgpu_cparams *p,
                                         const int32_t *const *planes, int planes_on_device, uint32_t row0,
                                         uint32_t nrows, uint32_t tile_begin, uint32_t tile_end, uint32_t parts,
                                         uint8_t **out, size_t *outlen) {
    if (!out || !outlen) return set_err(GRKGPU_EINVAL, "null argument");
    if (nrows == 0) return set_err(GRKGPU_EINVAL, "nrows must be > 0");
    const uint8_t *v = nullptr;
    size_t n = 0;
    int rc = compress_impl(c, img, p, (const void *const *)planes, planes_on_device, SMP_I32, &v, &n, tile_begin,
                           tile_end, parts, false, 0, row0, nrows);
    if (rc) return rc;
    uint8_t *o = (uint8_t *)malloc(n ? n : 1);
    if (!o) return set_err(GRKGPU_EINVAL, "out of host memory");
    memcpy(o, v, n);
    *out = o;
    *outlen = n;
    return GRKGPU_OK;
}

// ---------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------
static void image_desc_of(const CodingParams &cp, grkgpu_image_desc *img);

extern "C" int grkgpu_read_header(const uint8_t *cs, size_t len, grkgpu_image_desc *img) {
    if (!cs || !img) return set_err(GRKGPU_EINVAL, "null argument");
    CodingParams cp;
    size_t sot = 0;
    std::string err;
    if (!parse_main_header(cs, len, cp, sot, err)) return set_err(GRKGPU_EUNSUPPORTED, err);
    image_desc_of(cp, img);
    return GRKGPU_OK;
}

// the image a parsed main header describes (grkgpu_read_header's result)
static void image_desc_of(const CodingParams &cp, grkgpu_image_desc *img) {
    memset(img, 0, sizeof(*img));
    img->x0 = cp.image.x0; img->y0 = cp.image.y0; img->x1 = cp.image.x1; img->y1 = cp.image.y1;
    img->numcomps = cp.numcomps;
    for (uint32_t k = 0; k < cp.numcomps; ++k) {
        img->prec[k] = cp.prec[k];
        img->sgnd[k] = cp.sgnd[k];
        img->dx[k] = cp.dx[k];
        img->dy[k] = cp.dy[k];
    }
}

// The custom (Part 2 array-based) MCT of a stream, host only.  A failure of
// the main header is GRKGPU_ECORRUPT where the MCT segments are malformed.
extern "C" int grkgpu_read_mct(const uint8_t *cs, size_t len, grkgpu_image_desc *img, float *matrix,
                               int32_t *offsets, uint32_t *n) {
    if (!cs || !n) return set_err(GRKGPU_EINVAL, "null argument");
    CodingParams cp;
    size_t sot = 0;
    std::string err;
    bool corrupt = false;
    if (!parse_main_header(cs, len, cp, sot, err, true, &corrupt))
        return set_err(corrupt ? GRKGPU_ECORRUPT : GRKGPU_EUNSUPPORTED, err);
    if (img) image_desc_of(cp, img);
    *n = cp.mct == 2 ? cp.numcomps : 0;
    for (uint32_t i = 0; matrix && i < *n * *n; ++i) matrix[i] = cp.mct_decoding[i];
    for (uint32_t k = 0; offsets && k < *n; ++k) offsets[k] = cp.mct_offsets[k];
    return GRKGPU_OK;
}

extern "C" int grkgpu_read_header_info(const uint8_t *cs, size_t len, grkgpu_header_info *hi) {
    if (!cs || !hi) return set_err(GRKGPU_EINVAL, "null argument");
    CodingParams cp;
    size_t sot = 0;
    std::string err;
    if (!parse_main_header(cs, len, cp, sot, err)) return set_err(GRKGPU_EUNSUPPORTED, err);
    memset(hi, 0, sizeof(*hi));
    // the code-block / wavelet / precinct fields are component 0's (j2k.cpp:
    // 445-467 reads tcp->tccps[0]: a main COC for component 0 shows here)
    const CompParams &c0 = cp.comp[0];
    hi->cblockw_init = 1u << c0.cblkw;
    hi->cblockh_init = 1u << c0.cblkh;
    hi->irreversible = (uint32_t)c0.irrev;
    hi->mct = (uint32_t)cp.mct;
    hi->rsiz = cp.rsiz;
    hi->numresolutions = c0.numres;
    hi->csty = cp.csty;
    hi->cblk_sty = c0.cblksty;
    for (uint32_t r = 0; r < 33; ++r) {
        hi->prcw_init[r] = 1u << c0.prcw[r];
        hi->prch_init[r] = 1u << c0.prch[r];
    }
    hi->tx0 = cp.tx0; hi->ty0 = cp.ty0; hi->tdx = cp.tdx; hi->tdy = cp.tdy; hi->tw = cp.tw; hi->th = cp.th;
    hi->numlayers = cp.numlayers;
    hi->prog = cp.prog;
    hi->numcomps = cp.numcomps;
    hi->numgbits = cp.numgbits;
    hi->qntsty = cp.qntsty;
    hi->nsteps = std::min<uint32_t>(cp.nsteps, 97);
    for (uint32_t b = 0; b < hi->nsteps; ++b) { hi->step_expn[b] = cp.ss[b].expn; hi->step_mant[b] = cp.ss[b].mant; }
    for (uint32_t k = 0; k < cp.numcomps && k < 16; ++k) hi->roishift[k] = cp.roishift[k];
    return GRKGPU_OK;
}

extern "C" int grkgpu_read_comp_info(const uint8_t *cs, size_t len, uint32_t compno, grkgpu_comp_info *ci) {
    if (!cs || !ci) return set_err(GRKGPU_EINVAL, "null argument");
    CodingParams cp;
    size_t sot = 0;
    std::string err;
    if (!parse_main_header(cs, len, cp, sot, err)) return set_err(GRKGPU_EUNSUPPORTED, err);
    if (compno >= cp.numcomps) return set_err(GRKGPU_EINVAL, "component index out of range");
    const CompParams &c = cp.comp[compno];
    memset(ci, 0, sizeof(*ci));
    ci->csty = c.csty;
    ci->numresolutions = c.numres;
    ci->cblkw = c.cblkw;
    ci->cblkh = c.cblkh;
    ci->cblk_sty = c.cblksty;
    ci->qmfbid = c.irrev ? 0 : 1;
    for (uint32_t r = 0; r < 33; ++r) { ci->prcw[r] = c.prcw[r]; ci->prch[r] = c.prch[r]; }
    ci->qntsty = c.qntsty;
    ci->numgbits = c.numgbits;
    ci->nsteps = std::min<uint32_t>(c.nsteps, 100);
    for (uint32_t b = 0; b < ci->nsteps; ++b) { ci->step_expn[b] = c.ss[b].expn; ci->step_mant[b] = c.ss[b].mant; }
    ci->roishift = cp.roishift[compno];
    return GRKGPU_OK;
}

static uint32_t rd16(const uint8_t *p) { return ((uint32_t)p[0] << 8) | p[1]; }
static uint32_t rd32(const uint8_t *p) { return (rd16(p) << 16) | rd16(p + 2); }

static uint32_t ceil_pow2(uint32_t v, uint32_t r) { return (uint32_t)(((uint64_t)v + ((1ull << r) - 1)) >> r); }


// ---------------------------------------------------------------------------
// The reference decoder's walk over the tile-parts, restated over a memory
// stream (j2k_decode_tiles, j2k.cpp:1136-1224; j2k_read_tile_header :627-978
// with j2k_read_sot :5138-5260 and j2k_read_sod :5399-5480; the marker read
// after a decoded tile in j2k_decode_tile :979-1120; the look-ahead of
// j2k_need_nb_tile_parts_correction :534-625; BufferedStream / mem_stream
// reads and seeks, util/BufferedStream.cpp, util/mem_stream.cpp).  It decides
// which tiles a decode produces, from which of their tile-parts, and which
// short or damaged streams fail:
//   * tiles are decoded as their last tile-part (TNsot) is read; a stream
//     that ends -- or reaches EOC -- before a tile is complete still decodes
//     a tile whose data has begun, from the tile-parts read;
//   * a tile the walk never reaches is not decoded: its samples stay zero
//     (the multi-tile output image is cleared first, j2k.cpp:1148-1156);
//   * a stream ending inside a tile-part header, between a tile-part and the
//     next one of the same tile, or right after an SOD (a tile with no data)
//     fails, as do headers the reference refuses (tile-part index order,
//     Psot, markers outside their place, an unknown marker);
//   * the once-per-decode look-ahead over the following SOT headers fails on
//     an SOT cut inside its 10 header bytes, wherever the walk itself stops.
// A tile-part's data length is Psot less its header, clamped to the stream
// (Psot = 0: up to the last 2 bytes); skipped tiles (outside a decode
// window) step over their tile-parts, which a memory stream does past its
// end without failing -- the next read fails instead.
// ---------------------------------------------------------------------------
struct TpMarker { uint32_t m; size_t off; uint32_t len; };
struct TileWalk {
    std::vector<std::vector<std::pair<size_t, size_t>>> parts;  // per tile: data of the tile-parts read
    std::vector<std::vector<TpMarker>> marks;                  // per tile: its tile-part header markers
    std::vector<std::vector<uint32_t>> seq;                    // per tile: codestream index of each tile-part
    std::vector<uint8_t> decoded;                              // per tile: decoded by the walk
    std::vector<uint32_t> order;                               // the decoded tiles, in the order the walk decodes them
    uint32_t ntp = 0;
};

static bool tph_marker(uint32_t m) {  // allowed in a tile-part header (j2k.cpp:87-106, J2K_DEC_STATE_TPH)
    switch (m) {
        case 0xFF52: case 0xFF53: case 0xFF5E: case 0xFF5C: case 0xFF5D: case 0xFF5F: case 0xFF58: case 0xFF61:
        case 0xFF64: case 0xFF74: case 0xFF75: case 0xFF77: return true;
        default: return false;
    }
}

// j2k_need_nb_tile_parts_correction from position q (after tile `tile`'s
// last tile-part): false = the decode fails; *fix = a later SOT of the same
// tile has TPsot == TNsot (the non-conformant streams the reference patches:
// walk_tile_parts then raises every tile-part count by one, as j2k.cpp:809-835)
static bool tp_lookahead(const uint8_t *cs, size_t len, uint64_t q, uint32_t tile, bool *fix, std::string &err) {
    *fix = false;
    for (;;) {
        if (q > len || len - q < 2) return true;  // no further marker: assumed fine
        const uint32_t m = rd16(cs + q);
        q += 2;
        if (m != 0xFF90) return true;
        if (len - q < 2) { err = "Stream too short"; return false; }
        if (rd16(cs + q) != 10) { err = "Inconsistent marker size"; return false; }
        q += 2;
        if (len - q < 8) { err = "Stream too short"; return false; }
        const uint32_t t = rd16(cs + q), tot = rd32(cs + q + 2), part = cs[q + 6], nparts = cs[q + 7];
        q += 8;
        if (t == tile) { *fix = part == nparts; return true; }
        if (tot < 14) return true;  // 0: the last tile-part; < 14: invalid -- assumed fine
        q += tot - 12;              // a seek past the end succeeds; the next read fails
    }
}

// skip[t]: tile t lies outside the decode window (m_skip_data, j2k.cpp:5262-5274)
static bool walk_tile_parts(const uint8_t *cs, size_t len, size_t sot0, uint32_t ntiles, const std::vector<uint8_t> &skip,
                            TileWalk &w, std::string &err) {
    enum : uint32_t { TPHSOT = 0x08, TPH = 0x10, NEOC = 0x40, EOC = 0x100 };
    w.parts.assign(ntiles, {});
    w.marks.assign(ntiles, {});
    w.seq.assign(ntiles, {});
    w.decoded.assign(ntiles, 0);
    w.order.clear();
    w.ntp = 0;
    std::vector<int32_t> cur_tp(ntiles, -1);
    std::vector<uint32_t> nb_tp(ntiles, 0);
    std::vector<uint8_t> has_data(ntiles, 0);
    uint64_t p = sot0 + 2;  // the first SOT's code was read with the main header
    // bytes left; past the end (after a seek) the stream's unsigned count is huge
    auto left = [&]() -> uint64_t { return p <= len ? len - p : ~0ull; };
    auto read = [&](uint64_t n, uint64_t *at) -> bool {  // a short read takes what is left
        *at = p;
        if (p <= len && n <= len - p) { p += n; return true; }
        if (p < len) p = len;
        return false;
    };
    uint32_t state = TPHSOT, tcur = 0, tpl = 0, ndec = 0;
    uint32_t corr = 0;  // m_nb_tile_parts_correction: 1 once a TPsot == TNsot stream was detected
    bool ready = false, last_tp = false, checked = false, skipping = false;
    uint64_t at;
    for (uint32_t nr = 0; nr < ntiles; ++nr) {
        uint32_t marker = 0xFF90;
        if (state == EOC) marker = 0xFFD9;
        else if (state != TPHSOT) { err = "Stream too short"; return false; }
        while (!ready && marker != 0xFFD9) {
            while (marker != 0xFF93) {
                if (left() == 0) { state = NEOC; break; }
                if (!read(2, &at)) { err = "Stream too short"; return false; }
                uint32_t ms = rd16(cs + at);
                if (ms < 2) { err = "Inconsistent marker size"; return false; }
                if (state & TPH) tpl -= ms + 2;
                ms -= 2;
                const bool sot = marker == 0xFF90;
                if (sot ? !(state & TPHSOT) : (!(state & TPH) || !tph_marker(marker))) {
                    err = "Marker is not compliant with its position";
                    return false;
                }
                if (!read(ms, &at)) { err = "Stream too short"; return false; }
                if (sot) {  // j2k_read_sot
                    if (ms != 8) { err = "Error reading SOT marker"; return false; }
                    const uint32_t t = rd16(cs + at), psot = rd32(cs + at + 2), part = cs[at + 6], nparts = cs[at + 7];
                    if (t >= ntiles) { err = "Invalid tile number"; return false; }
                    tcur = t;
                    if (cur_tp[t] + 1 != (int32_t)part) { err = "Invalid tile part index"; return false; }
                    ++cur_tp[t];
                    if (psot && psot < 14 && psot != 12) { err = "Psot value is not correct"; return false; }
                    if (!psot) last_tp = true;
                    if (nb_tp[t] && part >= nb_tp[t]) { err = "Current tile part number greater than the tile-parts"; return false; }
                    if (nparts) {  // j2k.cpp:5210-5236: TNsot + the correction, as a byte
                        const uint32_t np = (nparts + corr) & 0xFF;
                        if (part >= np) { err = "In SOT marker, TPSot is not valid"; return false; }
                        nb_tp[t] = np;
                    }
                    if (nb_tp[t] && nb_tp[t] == part + 1) ready = true;
                    tpl = last_tp ? 0u : psot - 12;
                    state = TPH;
                    skipping = skip[t] != 0;
                    w.seq[t].push_back(w.ntp++);
                } else if (marker == 0xFF52 || marker == 0xFF5C || marker == 0xFF53 || marker == 0xFF5D ||
                           marker == 0xFF5E || marker == 0xFF5F || marker == 0xFF61 ||
                           marker == 0xFF74 || marker == 0xFF75 || marker == 0xFF77) {
                    // (MCT / MCC / MCO: only a custom-MCT decode looks at them, to refuse)
                    w.marks[tcur].push_back({marker, (size_t)at, ms});
                }
                if (skipping) {  // the rest of the tile-part stepped over
                    p += tpl;
                    marker = 0xFF93;
                } else {
                    if (!read(2, &at)) { err = "Stream too short"; return false; }
                    marker = rd16(cs + at);
                }
            }
            if (left() == 0 && state == NEOC) break;
            if (!skipping) {  // j2k_read_sod
                if (last_tp) tpl = (uint32_t)(left() - 2);
                else if (tpl >= 2) tpl -= 2;
                if (tpl && tpl > left()) tpl = (uint32_t)left();
                if (tpl) {
                    w.parts[tcur].push_back({(size_t)p, tpl});
                    has_data[tcur] = 1;
                    p += tpl;
                }
                state = TPHSOT;
                if (ready && !checked) {
                    checked = true;
                    bool fix = false;
                    if (!tp_lookahead(cs, len, p, tcur, &fix, err)) return false;
                    if (fix) {  // Issue 254 (j2k.cpp:809-835): every known tile-part count + 1, later TNsot + 1
                        ready = false;
                        corr = 1;
                        for (auto &n : nb_tp)
                            if (n) n = (n + 1) & 0xFF;
                    }
                }
                if (!ready) {
                    if (!read(2, &at)) { err = "Stream too short"; return false; }
                    marker = rd16(cs + at);
                }
            } else {
                skipping = false;
                ready = false;
                state = TPHSOT;
                if (!read(2, &at)) { err = "Stream too short"; return false; }
                marker = rd16(cs + at);
            }
        }
        if (marker == 0xFFD9 && state != EOC) { state = EOC; tcur = 0; }
        if (!ready) {  // the stream ended or reached EOC: the next tile holding data, if any
            while (tcur < ntiles && !has_data[tcur]) ++tcur;
            if (tcur == ntiles) break;
        }
        // j2k_decode_tile
        if (!has_data[tcur]) { err = "Failed to decode tile (no tile data)"; return false; }
        w.decoded[tcur] = 1;
        w.order.push_back(tcur);
        has_data[tcur] = 0;
        ready = false;
        ++ndec;
        if (left() == 0 && state == NEOC) break;
        if (state != EOC && read(2, &at)) {  // the marker after the tile: EOC, SOT, or the end
            const uint32_t m = rd16(cs + at);
            if (m == 0xFFD9) { tcur = 0; state = EOC; }
            else if (m != 0xFF90) {
                if (left() == 0) state = NEOC;
                else if (nr + 1 < ntiles) { err = "Stream too short, expected SOT"; return false; }
            }
        }
        if (left() == 0 && state == NEOC) break;
    }
    if (!ndec) { err = "No tiles were decoded"; return false; }
    return true;
}

// Where a decode stores its samples: the caller's planes, their sample format
// (SampleFmt) and layout.
struct DecodeOut {
    void *const *planes;  // planar: one per component; interleaved: planes[0]
    int32_t fmt;          // SampleFmt
    int32_t interleaved;
    int on_device;
    int upsample;  // GRKGPU_LAYOUT_UPSAMPLE: subsampled components replicated to the image grid
    const grkgpu_out_ops *ops;  // grkgpu_decompress_convert: colour / precision in the last store (null: none)
    int custom_mct;  // grkgpu_decompress_mct: a COD with MCT = 2 (Part 2 array-based) is decoded, not refused
    const struct ChanMap *chan;  // grkgpu_jp2_decompress: the output channels where they are not the components in order
    int is_rgb;  // grkgpu_jp2_decompress: the file says sRGB (GRKGPU_COLOUR_FORCE_RGB leaves 3+ channels alone)
    // grkgpu_decompress_float: fmt is SMP_F32 / _F16 / _BF16 (refused everywhere else), the samples leave as
    // v * scale + bias per output channel (null: 1, 0).  Such a decode always converts: ops is never null.
    int fl;
    const grkgpu_out_norm *norm;
};
// the formats a decode stores: the integer ones, or (the float entry points) the float ones
static bool out_fmt_ok(const DecodeOut &od) {
    return od.fl ? float_fmt(od.fmt) : (od.fmt >= SMP_I32 && od.fmt <= SMP_I16);
}
// The output channels of a JP2 file with a palette or a channel swap
// (jp2_resolve_channels): channel c takes component comp[c]'s sample, or entry
// [sample][pcol[c]] of the ne x npc table (host memory), and leaves with prec[c]
// bits.  Planes, sample format, layout and ops of the call describe channels.
struct ChanMap {
    uint32_t nch;
    uint32_t comp[GRKGPU_MAX_COMPS];
    int32_t pcol[GRKGPU_MAX_COMPS];
    uint32_t prec[GRKGPU_MAX_COMPS];
    int32_t sgnd[GRKGPU_MAX_COMPS];
    uint32_t ne, npc;
    const uint16_t *table;
};
static DecodeOut i32_planes(int32_t *const *planes, int on_device) {
    return {(void *const *)planes, SMP_I32, 0, on_device};
}

// grkgpu_out_ops' own rules, checked before anything touches a device; fmt = the
// output's sample format
static uint32_t colour_of(const grkgpu_out_ops *o) { return o->colour & ~GRKGPU_COLOUR_FORCE_RGB; }
static int check_out_ops(const grkgpu_out_ops *o, uint32_t fmt) {
    if (!o) return GRKGPU_OK;
    const uint32_t col = colour_of(o);  // (2 and 5 are GRKGPU_COLOUR_AUTO / _AUTO_RGB, resolved by the JP2 entry point)
    if (col != GRKGPU_COLOUR_NONE && col != GRKGPU_COLOUR_SYCC && col != GRKGPU_COLOUR_EYCC && col != GRKGPU_COLOUR_CMYK)
        return set_err(GRKGPU_EINVAL, "unknown colour conversion");
    if (o->prec > 16) return set_err(GRKGPU_EINVAL, "output precision must be 1 .. 16 (0: the component's own)");
    if (o->prec && o->prec_mode > GRKGPU_PREC_SCALE) return set_err(GRKGPU_EINVAL, "unknown precision mode");
    if (o->reserved) return set_err(GRKGPU_EINVAL, "reserved field of the output ops must be 0");
    if (o->prec && fmt != SMP_I32 && !float_fmt((int32_t)fmt) && o->prec > 8 * sample_bytes((int32_t)fmt))
        return set_err(GRKGPU_EINVAL, "sample format does not hold the output precision");
    return GRKGPU_OK;
}
static bool out_ops_active(const grkgpu_out_ops *o) { return o && (o->colour || o->prec); }

// The device form of checked ops for components of (prec, sgnd, dx, dy): the
// shape rules of the colour step (color_sycc_to_rgb, color.cpp:384-418;
// color_esycc_to_rgb / color_cmyk_to_rgb, :881-995, and grk_decompress's own
// checks around them) and each output channel's precision op (clip_component
// / scale_component, convert.cpp:82-161).  no = the output channels (the
// components, one fewer after CMYK), oprec[c] / osgnd[c] = what channel c
// leaves with.
static int resolve_out_ops(const grkgpu_out_ops *o, uint32_t nc, const uint32_t *prec_in, const int32_t *sgnd_in,
                           const uint32_t *dx, const uint32_t *dy, OutOps &dev, uint32_t &no, uint32_t *oprec,
                           int32_t *osgnd) {
    dev = OutOps{};
    no = nc;
    // the channels the precision step sees
    uint32_t prec[GRKGPU_MAX_COMPS];
    int32_t sgnd[GRKGPU_MAX_COMPS];
    for (uint32_t k = 0; k < nc; ++k) { prec[k] = prec_in[k]; sgnd[k] = sgnd_in[k]; }
    const uint32_t col = colour_of(o);
    if (col == GRKGPU_COLOUR_EYCC || col == GRKGPU_COLOUR_CMYK) {
        const bool cmyk = col == GRKGPU_COLOUR_CMYK;
        if (cmyk ? nc < 4 : nc != 3)
            return set_err(GRKGPU_EINVAL, cmyk ? "CMYK conversion needs at least 4 components"
                                               : "eYCC conversion needs exactly 3 components");
        for (uint32_t k = 1; k < nc; ++k)
            if (dx[k] != dx[0] || dy[k] != dy[0])
                return set_err(GRKGPU_EINVAL, cmyk ? "CMYK conversion needs every component on one grid"
                                                   : "eYCC conversion needs every component on one grid");
        if (cmyk) {
            for (uint32_t k = 0; k < 4; ++k) {
                if (sgnd[k] || prec[k] < 1 || prec[k] > 16)
                    return set_err(GRKGPU_EINVAL, "CMYK conversion needs unsigned inks of precision 1 .. 16");
                dev.sc[k] = 1.0f / (float)((1 << prec[k]) - 1);
            }
            dev.col = COL_CMYK;
            no = nc - 1;
            for (uint32_t c = 0; c < no; ++c) {
                prec[c] = c < 3 ? 8 : prec_in[c + 1];
                sgnd[c] = c < 3 ? 0 : sgnd_in[c + 1];
            }
        } else {
            if (sgnd[0] || prec[0] < 1 || prec[0] > 16 || prec[1] != prec[0] || prec[2] != prec[0])
                return set_err(GRKGPU_EINVAL, "eYCC conversion needs an unsigned component 0 and one precision (1 .. 16)");
            dev.col = COL_EYCC;
            dev.coff[0] = sgnd[1] ? 0 : 1 << (prec[0] - 1);
            dev.coff[1] = sgnd[2] ? 0 : 1 << (prec[0] - 1);
            dev.upb = (int32_t)((1u << prec[0]) - 1);
            sgnd[0] = sgnd[1] = sgnd[2] = 0;  // R, G, B in [0, upb]: reported, and scaled or clipped, as unsigned
        }
    }
    if (col == GRKGPU_COLOUR_SYCC) {
        if (nc != 3) return set_err(GRKGPU_EINVAL, "sYCC conversion needs exactly 3 components");
        for (uint32_t k = 0; k < 3; ++k)
            if (sgnd[k] || prec[k] != prec[0] || prec[k] < 1 || prec[k] > 16)
                return set_err(GRKGPU_EINVAL, "sYCC conversion needs unsigned components of one precision (1 .. 16)");
        const bool shape = dx[0] == 1 && dy[0] == 1 && dx[1] == dx[2] && dy[1] == dy[2] &&
                           ((dx[1] == 1 && dy[1] == 1) || (dx[1] == 2 && (dy[1] == 1 || dy[1] == 2)));
        if (!shape) return set_err(GRKGPU_EINVAL, "sYCC conversion needs 4:4:4, 4:2:2 or 4:2:0 subsampling");
        dev.sycc = 1;
        dev.off = 1 << (prec[0] - 1);
        dev.upb = (int32_t)((1u << prec[0]) - 1);
    }
    for (uint32_t k = 0; k < no; ++k) {
        const uint32_t q = prec[k], p = o->prec;
        PrecOp &op = dev.pc[k];
        oprec[k] = p ? p : q;
        osgnd[k] = sgnd[k];
        if (!p || p == q) continue;
        if (o->prec_mode == GRKGPU_PREC_CLIP) {
            if (p > q) continue;  // every value is inside the wider range
            op.mode = POP_CLIP;
            op.a = sgnd[k] ? -(1 << (p - 1)) : 0;
            op.b = sgnd[k] ? (1 << (p - 1)) - 1 : (int32_t)((1u << p) - 1);
        } else if (p < q) {
            op.mode = POP_SHR;
            op.a = (int32_t)(q - p);
        } else if (sgnd[k]) {
            op.mode = POP_MUL;
            op.a = 1 << (p - q);
        } else {
            op.mode = POP_MULDIV;
            op.a = (int32_t)((1u << p) - 1);
            op.b = (int32_t)((1u << q) - 1);
        }
    }
    return GRKGPU_OK;
}
// the narrowest sample format holding every component (a staging plane that keeps the stream's precision)
static int32_t holding_fmt(uint32_t nc, const uint32_t *prec, const int32_t *sgnd) {
    uint32_t mp = 0;
    bool any_s = false, any_u = false;
    for (uint32_t k = 0; k < nc; ++k) {
        mp = std::max(mp, prec[k]);
        (sgnd[k] ? any_s : any_u) = true;
    }
    if ((any_s && any_u) || mp > 16) return SMP_I32;
    return mp <= 8 ? (any_s ? SMP_I8 : SMP_U8) : (any_s ? SMP_I16 : SMP_U16);
}
// channel k's part of an image's ops, as the ops of a one-component store (a plane converted on its own grid)
static OutOps plane_ops(const OutOps &o, uint32_t k) {
    OutOps ok{};
    ok.pc[0] = o.pc[k];
    ok.scale[0] = o.scale[k];
    ok.bias[0] = o.bias[k];
    return ok;
}

// reduce > 0 (whole-image decode only): the image at resolution
// numres - 1 - reduce (grk_decompress -r, cp_reduce, grok.h:698-702): every
// packet is still parsed, code-blocks of the dropped resolutions are not
// decoded, the inverse DWT stops `reduce` levels early (TileProcessor.cpp:1165,
// TileComponent.cpp:199-204) and MCT + DC shift run on the reduced tiles; the
// image is ceil(coordinate / 2^reduce) (j2k.cpp:1464-1476).
//
// win (image coordinates; whole-image decode only): the window decode of
// grk_set_decode_area (grok.h:1587, j2k.cpp j2k_set_decode_area): only tiles
// meeting the window are parsed, only code-blocks whose coefficients reach it
// are decoded (window_need), the inverse DWT runs on those tiles and MCT +
// DC shift on the window; the output planes are the window.
//
// max_layers > 0: only the first max_layers quality layers are decoded
// (grk_decompress -l, cp_layer, grok.h:703-709; tcp->num_layers_to_decode,
// j2k.cpp:3861-3865): the packets of later layers are parsed and stepped over
// and their passes still count toward the block's pass total
// (T2::skip_packet_data, T2.cpp:758-819), so T1 runs those passes over the
// 0xFF fill past the decoded bytes, exactly as the reference does.
// host_only: stop after the host Tier-2 (tile-part walk, packet headers, the
// code-block table) -- no device call; *decoded_out (when given) receives the
// tiles decoded (grkgpu_walk_tiles)
//
// od: where the samples go (DecodeOut) -- the caller's planes, their sample
// format and layout.  k_mct_inv_dcshift's clamp leaves every sample inside its
// component's range, and the format must hold that range (compress_impl's
// rule), so a narrow format is exact: the last kernel stores the samples at
// that width, and the staging image, the zero fills and the copies to the host
// are sized by it.  Interleaved: one destination of ncomp-sample pixels, every
// component on one grid.
//
// od.upsample (grk_decompress -u, upsample_image_components,
// grk_decompress.cpp:891-1040) on a stream with subsampled components: every
// component on the image grid.  The launches that today write the planes
// write the subsampled components -- shifted, clamped, narrowed, after their
// MCT when all are subsampled alike -- to staging planes on their image-level
// grids where a tile's first pixels may map to a sample of the neighbouring
// tile (tile-component x0 = ceil(tx0 / dx): `staged` below), and one launch
// per tile (launch_upsample_to) writes the output: the other components
// straight from the tile buffer, the staged ones replicated from their planes.
//
// The host half of a decode is DecHost: begin() (main header, geometry, the
// refusals, the tile-part walk), parse_tiles() (packet headers, tile by tile,
// safe to run for different tiles on different threads) and finish() (arenas
// and the DecBlock / DecSeg tables, offsets counted from the stream's own
// zero).  decompress_impl runs them for its one stream; the batch decode runs
// them for every item and rebases the tables into the merged ones.
struct DecHost {
    // in
    const uint8_t *csb = nullptr;
    size_t len = 0;
    grkgpu_image_desc *img = nullptr;
    DecodeOut od{};
    uint32_t tb = 0, te = 0xffffffffu, reduce = 0, max_layers = 0;
    const Rect *win = nullptr;
    bool host_only = false;
    // an item of grkgpu_decompress_batch / grkgpu_batch_plan, the batch without the converting store: a stream
    // with a subsampled component is refused (grkgpu_decompress_batch_convert takes it)
    bool batch = false;
    // begin()
    void *const *planes = nullptr;
    int planes_on_device = 0;
    uint32_t sb = 4;
    bool il = false;
    CodingParams cp;
    Rect wr{};
    uint32_t ix0 = 0, iy0 = 0, ix1 = 0, iy1 = 0, ox1 = 0, oy1 = 0, nc = 0, ntiles = 0, iw = 0;
    bool whole = true, subs = false, mixed = false, conv = false, sycc = false, colconv = false;
    bool fl = false;  // a float destination: conv holds, dops carries scale / bias, no fill is a memset
    uint32_t colour = 0;
    OutOps dops{};
    uint32_t oprec[GRKGPU_MAX_COMPS];
    int32_t osgnd[GRKGPU_MAX_COMPS];
    const ChanMap *cm = nullptr;
    ChanMap fcm{};  // (cm may point here: a DecHost is never copied after begin())
    uint32_t no = 0;
    bool up = false;
    int32_t sfmt = SMP_I32;
    uint32_t ssb = 4;
    Rect orect[GRKGPU_MAX_COMPS];
    uint64_t ooff[GRKGPU_MAX_COMPS + 1];
    bool opad = false;
    Rect cwin[GRKGPU_MAX_COMPS];
    std::vector<uint8_t> wskip;
    TileWalk walk;
    bool missing = false;
    std::vector<uint8_t> ppm_buf;
    std::vector<std::pair<size_t, size_t>> ppm_chunk;  // (offset in ppm_buf, Nppm)
    uint32_t nsh = 0;
    std::vector<Tile> tiles;
    std::vector<std::vector<uint8_t>> tpacked;  // packed packet headers (PPM / PPT) of each tile
    std::vector<uint8_t> tpacked_on;
    std::vector<size_t> ppm_from;  // PPM: where each tile's packet headers start in ppm_buf
    // PPM: the tiles are parsed one after the other in the walk's order (finish()), ppm_run the reference's
    // one read pointer over the merged headers (cp->ppm_data, T2.cpp:375-378), valid after a parsed tile
    bool ppm_serial = false, ppm_run_valid = false;
    size_t ppm_run = 0;
    std::vector<int> terr, twhy;  // twhy: decode_packet's code behind terr = 2
    std::vector<std::array<uint8_t, 16>> troi;  // per tile: ROI shift of each component
    std::vector<std::array<uint8_t, 16>> tsty;  // per tile: code-block style of each component
    std::vector<int32_t> tmct;                  // per tile: MCT (a tile COD may change it)
    // finish()
    uint64_t arena = 0, llarena = 0;
    std::vector<uint64_t> lloff;
    std::vector<DecBlock> db;
    std::vector<DecSeg> dsegs;        // codeword segments of all blocks
    std::vector<uint8_t> droi;        // per-block ROI shift (empty: no ROI)
    std::vector<uint8_t> dsty;        // per-block code-block style (COD / COC of its tile-component)
    std::vector<uint32_t> seg_first;  // per block: first segment
    std::vector<uint8_t> extra;       // concatenated multi-chunk segments
    bool too_deep = false;

    int begin();
    // bytes of output region k: a plane, or (interleaved) the one image --
    // upsampled, every component has the output rectangle's iw x (oy1 - iy0) samples
    size_t region_bytes(uint32_t k) const {
        if (up) return (size_t)((uint64_t)iw * (oy1 - iy0) * (il ? no : 1)) * sb;
        return (size_t)(il ? ooff[no] : ooff[k + 1] - ooff[k]) * sb;
    }
    void parse_tiles(size_t l0, size_t l1);
    int finish();

    // The last store's decisions as the batch decode's records need them
    // (decompress_impl states the same rules inline, for its per-tile launches).
    // Upsampled: which components go through a staging plane -- all when they
    // share one subsampled grid (their MCT runs first); otherwise those with a
    // tile boundary that is no multiple of dx / dy, where the tile's first
    // pixels map to a sample of the neighbouring tile-component (it starts at
    // ceil(tx0 / dx)).  The others are read from the tile buffers, like the
    // full-resolution components.
    bool staged(uint32_t k) const {
        if (!up || (cp.dx[k] == 1 && cp.dy[k] == 1)) return false;
        const bool xseam = cp.tw > 1 && (cp.tx0 % cp.dx[k] || cp.tdx % cp.dx[k]);
        const bool yseam = cp.th > 1 && (cp.ty0 % cp.dy[k] || cp.tdy % cp.dy[k]);
        return !mixed || xseam || yseam;
    }
    // bytes of component k's staging plane (format sfmt), rounded so that the next one starts on a 16-byte boundary
    size_t stage_bytes(uint32_t k) const {
        return staged(k) ? ((size_t)(ooff[k + 1] - ooff[k]) * ssb + 15) & ~(size_t)15 : 0;
    }
    // the output regions: the planes, or the one interleaved image
    uint32_t nout() const { return il ? 1 : no; }
    // the store on the components' own grids converts (precision or colour on one grid, or precision on each
    // plane's own grid); else the ops, if any, run in the upsampling store
    bool grid_ops() const { return conv && !up; }
    // samples nothing decoded leave as the colour conversion of zeros, by a converting store over null sources
    // (a float destination: always -- the normalised zero is no memset; on each plane's own grid when mixed)
    bool converted_zeros() const { return (colconv || fl) && !up && !cm && (opad || missing); }
    // the clamped, shifted tile at the decoded resolution: where component k's samples of tile lt lie in
    // its tile buffer (tr) and the part of them inside the output (out)
    Rect tile_res(uint32_t lt, uint32_t k) const {
        const TileComp &tc = tiles[lt].comps[k];
        return tc.res[tc.numres - 1 - reduce].r;
    }
    // component k of an upsampled decode's tile as the upsampling store reads it: its staging plane `stg`
    // (staged(k)) or the tile buffer `buf` (null: a tile never reached)
    UpComp up_comp(uint32_t lt, uint32_t k, const void *stg, const int32_t *buf) const {
        UpComp u{};
        u.dx = (uint8_t)cp.dx[k];
        u.dy = (uint8_t)cp.dy[k];
        if (staged(k)) {
            u.src = stg;
            u.stride = orect[k].w();
            u.gx0 = (int32_t)orect[k].x0;
            u.gy0 = (int32_t)orect[k].y0;
        } else {
            const Rect tr = comp_rect(tiles[lt].r, cp.dx[k], cp.dy[k]);
            u.raw = 1;
            u.gx0 = (int32_t)tr.x0;
            u.gy0 = (int32_t)tr.y0;
            u.stride = tr.w();
            if (!tiles[lt].comps.empty()) {
                u.src = buf;
                u.irrev = (uint8_t)tiles[lt].comps[k].irrev;
            }
            u.shift = cp.shift[k];
            u.mn = cp.sgnd[k] ? -(1 << (cp.prec[k] - 1)) : 0;
            u.mx = cp.sgnd[k] ? (1 << (cp.prec[k] - 1)) - 1 : (1 << cp.prec[k]) - 1;
        }
        // the zero lead-in: left of / above the output rectangle's origin on the component's grid
        u.zx0 = std::max((int32_t)orect[k].x0, u.gx0);
        u.zy0 = std::max((int32_t)orect[k].y0, u.gy0);
        return u;
    }
};

int DecHost::begin() {
    planes = od.planes;
    planes_on_device = od.on_device;
    if (!csb || (!planes && !host_only)) return set_err(GRKGPU_EINVAL, "null argument");
    if (!out_fmt_ok(od)) return set_err(GRKGPU_EINVAL, "unknown sample format");
    fl = od.fl != 0;
    sb = sample_bytes(od.fmt);  // bytes per output sample
    il = od.interleaved != 0;
    size_t pos = 0;
    std::string err;
    bool hdr_corrupt = false;
    if (!parse_main_header(csb, len, cp, pos, err, od.custom_mct != 0, &hdr_corrupt))
        return set_err(hdr_corrupt ? GRKGPU_ECORRUPT : GRKGPU_EUNSUPPORTED, err);
    if (img) image_desc_of(cp, img);
    if (reduce >= cp.numres)  // j2k.cpp:6994
        return set_err(GRKGPU_EINVAL, "reduce must be smaller than the number of resolutions");
    // the window, clipped to the image
    if (win) {
        wr = intersect(*win, cp.image);
        if (wr.empty()) return set_err(GRKGPU_EINVAL, "decode window outside the image");
    }
    // output image geometry: the image or the window (reference grid), at the
    // decoded resolution ceil(x / 2^reduce) (j2k_set_decode_area, j2k.cpp:1464-1476)
    const Rect full = win ? wr : cp.image;
    ix0 = ceil_pow2(full.x0, reduce), iy0 = ceil_pow2(full.y0, reduce);
    ix1 = ceil_pow2(full.x1, reduce), iy1 = ceil_pow2(full.y1, reduce);
    if (win && (ix1 <= ix0 || iy1 <= iy0)) return set_err(GRKGPU_EINVAL, "decode window empty at this resolution");
    // Without a window the planes take grk_image_comp_header_update's sizes,
    // ceil(size / 2^reduce) (image.cpp:124-155), while the tiles land from
    // ceil(x0 / 2^reduce) (TileProcessor.cpp:1729-1734): with an odd origin
    // that is one row / column more than the decoded samples, left zero.
    // A window takes update_image_dimensions' (image.cpp:207-246) exact extent.
    ox1 = win ? ix1 : ix0 + ceil_pow2(full.w(), reduce);
    oy1 = win ? iy1 : iy0 + ceil_pow2(full.h(), reduce);
    if (img && (reduce || win)) {
        img->x0 = ix0; img->y0 = iy0;
        img->x1 = ox1; img->y1 = oy1;
    }
    nc = cp.numcomps, ntiles = cp.tw * cp.th;
    iw = ox1 - ix0;
    if (te > ntiles) te = ntiles;
    if (tb > te) return set_err(GRKGPU_EINVAL, "bad tile range");
    whole = tb == 0 && te == ntiles;
    if (reduce && !whole) return set_err(GRKGPU_EINVAL, "reduced decode of a tile range is not supported");
    // subsampled components: component k's output plane is the output
    // rectangle on its grid (ceil(x / dx), the nested ceilings of a reduced
    // decode commute), rows of its own width
    subs = false, mixed = false;  // mixed: components on different grids
    for (uint32_t k = 0; k < nc; ++k) {
        subs = subs || cp.dx[k] != 1 || cp.dy[k] != 1;
        mixed = mixed || cp.dx[k] != cp.dx[0] || cp.dy[k] != cp.dy[0];
    }
    if (subs && !whole) return set_err(GRKGPU_EUNSUPPORTED, "tile-range decode of subsampled images is not supported");
    if (subs && batch) return set_err(GRKGPU_EUNSUPPORTED, "subsampled components are not supported in a batch");
    if (win && !whole) return set_err(GRKGPU_EINVAL, "window decode of a tile range is not supported");
    // od.ops (grkgpu_decompress_convert): the colour and precision steps of
    // grk_decompress in the store of the last kernel -- dops their device
    // form, oprec the precision the samples leave with.  sYCC needs every
    // component of the pixel, so it implies the upsampled output.
    // A float destination (od.fl) converts whatever the ops say: its scale and
    // bias ride in dops, so every store of it is a store with ops.
    conv = out_ops_active(od.ops) || fl;
    colour = conv ? colour_of(od.ops) : GRKGPU_COLOUR_NONE;
    sycc = colour == GRKGPU_COLOUR_SYCC;
    // eYCC / CMYK -> RGB sit where sYCC sits, on components of one grid (they
    // do not imply the upsampled output); CMYK leaves nc - 1 channels
    colconv = colour != GRKGPU_COLOUR_NONE;
    const bool force_rgb = conv && (od.ops->colour & GRKGPU_COLOUR_FORCE_RGB);
    dops = OutOps{};
    for (uint32_t k = 0; k < nc; ++k) { oprec[k] = cp.prec[k]; osgnd[k] = cp.sgnd[k]; }
    // the shape rules, on the codestream's components: ahead of what force-RGB
    // makes of the channel count, and of the refusal behind a channel map
    if (colconv && (!sycc || !od.chan)) {
        uint32_t n_;
        int rc = resolve_out_ops(od.ops, nc, cp.prec, cp.sgnd, cp.dx, cp.dy, dops, n_, oprec, osgnd);
        if (rc) return rc;
    }
    // od.chan (grkgpu_jp2_decompress): `no` output channels instead of the nc
    // components -- what the planes, the format and the ops describe from here on
    cm = od.chan;
    // GRKGPU_COLOUR_FORCE_RGB (convert_gray_to_rgb, grk_decompress.cpp:805-890)
    // on the one or two channels the steps before it leave: channel 0 three
    // times and the second one behind it -- a channel map without a table,
    // stored by the palette kernels
    fcm = ChanMap{};
    {
        const uint32_t nbefore = cm ? cm->nch : (colour == GRKGPU_COLOUR_CMYK ? nc - 1 : nc);
        if (force_rgb && nbefore >= 1 && nbefore <= 2) {
            if (subs) return set_err(GRKGPU_EUNSUPPORTED, "force-RGB over subsampled components");
            if (cp.mct == 2) return set_err(GRKGPU_EUNSUPPORTED, "force-RGB behind a custom MCT");
            fcm.nch = nbefore + 2;
            for (uint32_t ch = 0; ch < fcm.nch; ++ch) {
                const uint32_t from = ch < 3 ? 0 : 1;
                fcm.comp[ch] = cm ? cm->comp[from] : from;
                fcm.pcol[ch] = cm ? cm->pcol[from] : -1;
                fcm.prec[ch] = cm ? cm->prec[from] : cp.prec[from];
                fcm.sgnd[ch] = cm ? cm->sgnd[from] : cp.sgnd[from];
            }
            if (cm) { fcm.ne = cm->ne; fcm.npc = cm->npc; fcm.table = cm->table; }
            cm = &fcm;
        } else if (force_rgb && !colconv && !od.is_rgb) {
            return set_err(GRKGPU_EINVAL, "force-RGB: don't know how to convert these channels to RGB");
        }
    }
    no = cm ? cm->nch : nc;
    if (cm) {
        if (subs) return set_err(GRKGPU_EUNSUPPORTED, "JP2 palette / channel order over subsampled components");
        if (sycc) return set_err(GRKGPU_EUNSUPPORTED, "sYCC conversion behind a JP2 palette or channel swap");
        if (colconv) return set_err(GRKGPU_EUNSUPPORTED, "eYCC / CMYK conversion behind a JP2 palette or channel swap");
        if (no < 1 || no > GRKGPU_MAX_COMPS) return set_err(GRKGPU_EINVAL, "bad channel map");
        for (uint32_t ch = 0; ch < no; ++ch) {
            if (cm->comp[ch] >= nc || (cm->pcol[ch] >= 0 && (!cm->table || !cm->ne || (uint32_t)cm->pcol[ch] >= cm->npc)))
                return set_err(GRKGPU_EINVAL, "bad channel map");
            oprec[ch] = cm->prec[ch];
            osgnd[ch] = cm->sgnd[ch];
        }
        if (img) {
            img->numcomps = no;
            for (uint32_t ch = 0; ch < no; ++ch) {
                img->prec[ch] = cm->prec[ch];
                img->sgnd[ch] = cm->sgnd[ch];
                img->dx[ch] = img->dy[ch] = 1;
            }
        }
        if (conv) {
            uint32_t one[GRKGPU_MAX_COMPS];
            for (uint32_t ch = 0; ch < GRKGPU_MAX_COMPS; ++ch) one[ch] = 1;
            uint32_t n_;
            int rc = resolve_out_ops(od.ops, no, cm->prec, cm->sgnd, one, one, dops, n_, oprec, osgnd);
            if (rc) return rc;
        }
    } else if (conv) {
        int rc = resolve_out_ops(od.ops, nc, cp.prec, cp.sgnd, cp.dx, cp.dy, dops, no, oprec, osgnd);
        if (rc) return rc;
    }
    if (fl) {  // the output channels' scale and bias; entries beyond them are not read
        for (uint32_t k = 0; k < no; ++k) {
            dops.scale[k] = od.norm ? od.norm->scale[k] : 1.0f;
            dops.bias[k] = od.norm ? od.norm->bias[k] : 0.0f;
            if (!std::isfinite(dops.scale[k]) || !std::isfinite(dops.bias[k]))
                return set_err(GRKGPU_EINVAL, "scale and bias of every output channel must be finite");
        }
    }
    up = (od.upsample || sycc) && subs;
    if (up && reduce)  // grk_decompress refuses -u with -r
        return set_err(GRKGPU_EINVAL, "upsampled output of a reduced decode is not supported");
    if (img && up)
        for (uint32_t k = 0; k < nc; ++k) img->dx[k] = img->dy[k] = 1;
    if (img && conv)
        for (uint32_t k = 0; k < no; ++k) img->prec[k] = oprec[k];
    if (img && colconv && !sycc) {  // the output channels: unsigned R, G, B, and CMYK's one fewer
        img->numcomps = no;
        for (uint32_t k = 0; k < no; ++k) {
            img->sgnd[k] = osgnd[k];
            if (no != nc && k >= 3) { img->dx[k] = img->dx[k + 1]; img->dy[k] = img->dy[k + 1]; }
        }
    }
    for (uint32_t k = 0; od.fmt != SMP_I32 && !fl && k < no; ++k) {  // (a float format holds every precision and sign)
        const bool sg = od.fmt == SMP_I8 || od.fmt == SMP_I16;
        if ((osgnd[k] != 0) != sg || oprec[k] > 8 * sb)
            return set_err(GRKGPU_EINVAL, "sample format does not hold the component's precision / signedness");
        // a channel used directly carries its component's samples whatever the palette box says of its size
        if (cm && cm->pcol[k] < 0 && (cm->prec[k] != cp.prec[cm->comp[k]] || (cm->sgnd[k] != 0) != (cp.sgnd[cm->comp[k]] != 0)))
            return set_err(GRKGPU_EINVAL, "a directly mapped channel whose declared size differs from its component's "
                                          "needs int32 samples");
    }
    // the staging planes of an upsampled decode keep the stream's precision:
    // the ops run in the replicating launch, which reads one sample type and
    // writes another (12 bits staged, 8 stored)
    sfmt = conv ? holding_fmt(nc, cp.prec, cp.sgnd) : od.fmt;
    ssb = sample_bytes(sfmt);
    if (il && mixed && !up)
        return set_err(GRKGPU_EUNSUPPORTED, "interleaved output needs every component on one grid");
    if (il && (uint64_t)iw * no > 0xffffffffull)  // the kernel's row stride is 32 bits of samples
        return set_err(GRKGPU_EUNSUPPORTED, "image too wide for interleaved output");
    for (uint32_t k = 0; !host_only && k < (il ? 1u : no); ++k)
        if (!planes[k] || (uintptr_t)planes[k] % sb) return set_err(GRKGPU_EINVAL, "null or misaligned output plane");
    ooff[0] = 0;
    opad = false;  // planes extending past the decoded samples (zero filled)
    for (uint32_t k = 0; k < std::max(nc, no); ++k) {  // (a channel map: every component at (1,1))
        const uint32_t kdx = k < nc ? cp.dx[k] : 1, kdy = k < nc ? cp.dy[k] : 1;
        orect[k] = comp_rect({ix0, iy0, ix1, iy1}, kdx, kdy);
        if (!win) {  // ceil(ceil(size on the component grid) / 2^reduce)
            const Rect cr = comp_rect(cp.image, kdx, kdy);
            const Rect sized{orect[k].x0, orect[k].y0, orect[k].x0 + ceil_pow2(cr.w(), reduce),
                             orect[k].y0 + ceil_pow2(cr.h(), reduce)};
            opad = opad || sized.x1 != orect[k].x1 || sized.y1 != orect[k].y1;
            orect[k] = sized;
        }
        ooff[k + 1] = ooff[k] + (uint64_t)orect[k].w() * orect[k].h();
    }
    // the window on each component's grid at the decoded resolution
    for (uint32_t k = 0; k < nc; ++k) cwin[k] = comp_rect({ix0, iy0, ix1, iy1}, cp.dx[k], cp.dy[k]);

    // tile-parts: the reference's walk (walk_tile_parts) -- which tiles are
    // decoded, from which tile-parts, and where a short stream fails; the
    // coding-parameter markers of the tile-part headers (COD / COC / QCD / QCC
    // / RGN / POC / PPT, j2k.cpp:3829-4990) are applied to the tile's own copy
    // of the parameters below
    wskip.assign(ntiles, 0);
    if (win)
        for (uint32_t t = 0; t < ntiles; ++t)
            wskip[t] = !overlap(comp_rect(tile_rect(cp, t), 1u << reduce, 1u << reduce), {ix0, iy0, ix1, iy1});
    if (!walk_tile_parts(csb, len, pos, ntiles, wskip, walk, err)) return set_err(GRKGPU_ECORRUPT, err);
    missing = false;  // tiles the walk did not decode: zero in the output
    for (uint32_t t = tb; t < te; ++t) missing = missing || (!walk.decoded[t] && !wskip[t]);
    // PPM (j2k_merge_ppm, j2k.cpp:4766-4900): the main header's packed packet
    // headers, Zppm order, as Nppm / Ippm pairs -- the i-th pair holds the
    // headers of the codestream's i-th tile-part
    if (!cp.ppm.empty()) {
        std::vector<uint8_t> raw;
        for (auto &q : cp.ppm) raw.insert(raw.end(), csb + q.off, csb + q.off + q.len);
        size_t o = 0;
        while (o < raw.size()) {
            if (o + 4 > raw.size()) return set_err(GRKGPU_ECORRUPT, "Not enough bytes to read Nppm");
            const uint32_t nppm = rd32(raw.data() + o);
            o += 4;
            if (o + nppm > raw.size()) return set_err(GRKGPU_ECORRUPT, "Corrupted PPM markers");
            ppm_chunk.push_back({ppm_buf.size(), nppm});
            ppm_buf.insert(ppm_buf.end(), raw.begin() + o, raw.begin() + o + nppm);
            o += nppm;
        }
    }

    // host Tier-2 over every tile of the shard; code-block segments -> DecBlock table
    nsh = te - tb;
    tiles.assign(nsh, Tile());
    tpacked.assign(nsh, {});
    tpacked_on.assign(nsh, 0);
    ppm_from.assign(nsh, 0);
    // 1: bad POC marker, 2: corrupt packet header, 3: bad tile-part COD / COC
    // / QCD / QCC / RGN / PPT, 4: tile-component parameters this decoder does
    // not take (code-block style, wavelet or MCT other than the main header's,
    // reduce >= its resolutions), 6: a custom MCT the tile-part headers touch
    // (MCT / MCC / MCO there, a tile COD with another MCT, a 5/3 component)
    terr.assign(nsh, 0);
    twhy.assign(nsh, 0);
    troi.assign(nsh, {});
    tsty.assign(nsh, {});
    tmct.assign(nsh, cp.mct);
    return GRKGPU_OK;
}

// Packet headers of tiles [l0, l1) of the shard (each tile's geometry, tag
// trees and code-block segments are its own, so tiles parse in parallel on
// the host pool); finish() then lays out the arenas and the DecBlock table in
// tile order.
void DecHost::parse_tiles(size_t l0, size_t l1) {
    const auto &tparts = walk.parts;
    const auto &tmarks = walk.marks;
    const auto &tpseq = walk.seq;
    {
        for (size_t lt = l0; lt < l1; ++lt) {
            const uint32_t t = tb + (uint32_t)lt;
            Tile &tile = tiles[lt];
            tile.index = t;
            tile.r = tile_rect(cp, t);
            for (uint32_t k = 0; k < 16; ++k) troi[lt][k] = cp.roishift[k];
            if (win && !overlap(comp_rect(tile.r, 1u << reduce, 1u << reduce), {ix0, iy0, ix1, iy1}))
                continue;  // left without components: skipped below
            if (!walk.decoded[t]) continue;  // never reached: its samples stay zero
            bool run_on = false;  // PPM: the headers go on where the tile decoded before this one left them
            if (!ppm_chunk.empty()) {
                if (!ppm_serial) continue;  // (finish() comes back for it)
                run_on = ppm_run_valid && !win;
                ppm_run_valid = false;
            }
            // the tile's coding parameters: the main header's, then its
            // tile-part headers' markers (precedence tile COC > tile COD >
            // main COC > main COD; QCC / QCD alike); POC entries appended
            CodingParams tcp = cp;
            {
                bool tcod = false, tqcd = false, tcoc[16] = {}, tqcc[16] = {}, ok = true;
                std::string e;
                std::vector<PpxSeg> ppt;
                for (const TpMarker &mk : tmarks[t]) {
                    const uint8_t *mp = csb + mk.off;
                    if (mk.m == 0xFF52) {  // sets every component, a COC before it included
                        ok = parse_cod(mp, mk.len, tcp, e, od.custom_mct != 0);
                        tcod = true;
                        for (uint32_t k = 0; k < 16; ++k) tcoc[k] = false;
                    }
                    else if (mk.m == 0xFF5C) { ok = parse_qcd(mp, mk.len, tcp, e); tqcd = true; }
                    else if (mk.m == 0xFF53) { const int32_t k = parse_coc(mp, mk.len, tcp, e); ok = k >= 0; if (ok) tcoc[k] = true; }
                    else if (mk.m == 0xFF5D) { const int32_t k = parse_qcc(mp, mk.len, tcp, e); ok = k >= 0; if (ok) tqcc[k] = true; }
                    else if (mk.m == 0xFF5E) {  // RGN (j2k_read_rgn, j2k.cpp:5555-5604)
                        const uint32_t room = nc <= 256 ? 1 : 2;
                        const uint32_t k = room == 2 ? rd16(mp) : mp[0];
                        ok = mk.len == 2 + room && k < nc;
                        if (ok) tcp.roishift[k] = mp[room + 1];
                    } else if (mk.m == 0xFF5F) {
                        if (!parse_poc(mp, mk.len, tcp)) { terr[lt] = 1; break; }
                    } else if (mk.m == 0xFF61) {  // PPT (j2k_read_ppt, j2k.cpp:4901-4978): Zppt, Ippt
                        ok = mk.len >= 1;
                        if (ok) ppt.push_back({mp[0], mk.off + 1, (size_t)mk.len - 1});
                    } else if (cp.mct == 2 && (mk.m == 0xFF74 || mk.m == 0xFF75 || mk.m == 0xFF77)) {
                        terr[lt] = 6;
                        break;
                    }
                    if (!ok) break;
                }
                if (terr[lt]) continue;
                if (!ok) { terr[lt] = 3; continue; }
                for (uint32_t k = 0; k < 16; ++k) {
                    if (tcod && !tcoc[k]) comp_style_from_cod(tcp, k);
                    if (tqcd && !tqcc[k]) comp_quant_from_qcd(tcp, k);
                }
                if (!check_qcd_steps(tcp, cp.qcc_set, tqcd, tqcc, e)) { terr[lt] = 5; continue; }
                for (uint32_t k = 0; k < nc; ++k) {
                    // a tile-part COD / COC's code-block style is read as a byte and never checked
                    // (j2k_read_SPCod_SPCoc, j2k.cpp:7019); Tier-2 and Tier-1 look at its six Part-1 bits
                    // only (T2::init_seg, T2.cpp:839-841; HT is the CAP marker's, j2k.cpp:6985), so the
                    // reference decodes style 0x84 as 0x04
                    tcp.comp[k].cblksty &= 0x3Fu;
                    const CompParams &cc = tcp.comp[k];
                    if (reduce >= cc.numres || cc.cblkw > 6 || cc.cblkh > 6) ok = false;
                    troi[lt][k] = tcp.roishift[k];
                    tsty[lt][k] = (uint8_t)cc.cblksty;
                }
                // MCT over components of different wavelets (the reference
                // picks the transform by component 0's alone) or sizes
                if (tcp.mct && nc >= 3 && (tcp.comp[1].irrev != tcp.comp[0].irrev ||
                                           tcp.comp[2].irrev != tcp.comp[0].irrev || cp.dx[1] != cp.dx[0] ||
                                           cp.dx[2] != cp.dx[0] || cp.dy[1] != cp.dy[0] || cp.dy[2] != cp.dy[0]))
                    ok = false;
                tmct[lt] = tcp.mct;
                if (!ok) { terr[lt] = 4; continue; }
                if (cp.mct == 2 || tcp.mct == 2) {  // one transform for the stream, every component 9/7
                    bool same = tcp.mct == cp.mct;
                    for (uint32_t k = 0; k < nc; ++k) same = same && tcp.comp[k].irrev;
                    if (!same) { terr[lt] = 6; continue; }
                }
                // the tile's packed packet headers: its PPT segments in Zppt
                // order (j2k_merge_ppt), or its tile-parts' PPM chunks
                std::sort(ppt.begin(), ppt.end(), [](const PpxSeg &a, const PpxSeg &b) { return a.z < b.z; });
                for (size_t q = 1; q < ppt.size(); ++q)
                    if (ppt[q].z == ppt[q - 1].z) ok = false;  // "Zppt already read" (j2k.cpp:4958)
                std::vector<uint8_t> &ph = tpacked[lt];
                ph.clear();
                if (!ppm_chunk.empty()) {
                    // the reference reads PPM headers through one running
                    // pointer over the merged Nppm chunks (T2.cpp:366-375): a
                    // tile's headers start at its first tile-part's chunk and
                    // run on past its own chunks when the stream ended before
                    // its later tile-parts (the tile is decoded from the
                    // tile-parts read, its later packets' headers still parsed)
                    for (uint32_t q : tpseq[t])
                        if (q >= ppm_chunk.size()) ok = false;
                    // the reference never moves its pointer to a tile's chunk (j2k_merge_ppm sets it once,
                    // j2k.cpp:4883): a tile's headers start where the tile decoded before it stopped
                    // reading, which in a well-formed stream is its first tile-part's chunk -- where a
                    // tile starts when this decode did not parse the tile decoded before it (a shard, a
                    // window)
                    if (ok && !tpseq[t].empty()) ppm_from[lt] = run_on ? ppm_run : ppm_chunk[tpseq[t][0]].first;
                    tpacked_on[lt] = 1;
                } else if (!ppt.empty()) {
                    for (auto &q : ppt) ph.insert(ph.end(), csb + q.off, csb + q.off + q.len);
                    tpacked_on[lt] = 1;
                }
                if (!ok) { terr[lt] = 3; continue; }
            }
            tile.comps.resize(nc);
            for (uint32_t k = 0; k < nc; ++k) build_tilecomp(tile.comps[k], tile.r, tcp, k, false);
            // tile data: the tile-parts in place, walked as the reference's chunk buffer (TileData)
            TileData td;
            td.cs = csb;
            td.cs_len = len;
            for (auto &pp : tparts[t]) td.add(pp.first, pp.second);
            // packets in the tile's progression (T2::decode_packets, T2.cpp:194-258),
            // POC entries of the main header followed by the tile's own
            std::vector<PacketId> order;
            decode_packet_order(tcp, tile, order);
            uint32_t packno = 0;
            PackedHdr packed = ppm_chunk.empty() ? PackedHdr{tpacked[lt].data(), tpacked[lt].size(), 0}
                                                 : PackedHdr{ppm_buf.data() + ppm_from[lt], ppm_buf.size() - ppm_from[lt], 0};
            for (const auto &pk : order) {
                // the data ends before the packets do (a truncated stream):
                // the remaining packets are empty (a zero-length header reads
                // as "no data", T2.cpp:393-400) -- unless the headers are packed
                // (PPM / PPT), which keep coming; their bodies are then empty
                if (!td.left() && !tpacked_on[lt]) break;
                const bool skip = max_layers && pk.layno >= max_layers;
                const int prc = decode_packet(tile.comps[pk.compno], pk.resno, pk.precno, pk.layno, td, tcp.csty, &packno,
                                              skip, tcp.comp[pk.compno].cblksty, tpacked_on[lt] ? &packed : nullptr);
                if (prc < 0) { terr[lt] = 2; twhy[lt] = prc; break; }
            }
            if (!ppm_chunk.empty() && !tpseq[t].empty()) {
                ppm_run = ppm_from[lt] + packed.off;
                ppm_run_valid = true;
            }
        }
    }
}

// The tiles' errors in tile order, then the arenas and the block table.
int DecHost::finish() {
    if (!ppm_chunk.empty()) {
        ppm_serial = true;
        ppm_run_valid = false;
        for (uint32_t t : walk.order)
            if (t >= tb && t < te) parse_tiles(t - tb, t - tb + 1);
            else ppm_run_valid = false;
    }
    arena = llarena = 0;
    lloff.assign((size_t)nsh * nc, 0);
    for (uint32_t lt = 0; lt < nsh; ++lt) {
        if (terr[lt] == 1) return set_err(GRKGPU_ECORRUPT, "Error reading POC marker");
        if (terr[lt] == 2) {
            static const char *const why[] = {"", "SOP marker packet counter does not match", "inclusion bit",
                                              "zero bit-plane tag tree", "impossibly many bit-planes", "number of passes",
                                              "length indicator increment", "too many bits in segment length",
                                              "unable to read packet header"};
            return set_err(GRKGPU_ECORRUPT, std::string("corrupt packet header (") + why[-twhy[lt]] + ")");
        }
        if (terr[lt] == 3) return set_err(GRKGPU_ECORRUPT, "corrupt tile-part header marker (COD/COC/QCD/QCC/RGN/PPT/PPM)");
        if (terr[lt] == 5)
            return set_err(GRKGPU_ECORRUPT, "QCD marker: number of step sizes is less than 3 * (tile decompositions) + 1");
        if (terr[lt] == 6)
            return set_err(GRKGPU_EUNSUPPORTED, "custom MCT: MCT / MCC / MCO in a tile-part header, a tile COD with "
                                                "another MCT or a 5/3 tile-component are not supported");
        if (terr[lt] == 4)
            return set_err(GRKGPU_EUNSUPPORTED, "tile-component coding style not supported ("
                                                "code-blocks above 64 x 64, MCT over components of different "
                                                "wavelets or sizes, or reduce too large)");
    }
    bool any_roi = false;
    for (uint32_t lt = 0; lt < nsh; ++lt)
        for (uint32_t k = 0; k < nc; ++k) any_roi = any_roi || troi[lt][k];
    for (uint32_t lt = 0; lt < nsh; ++lt) {
        Tile &tile = tiles[lt];
        if (tile.comps.empty()) continue;
        for (uint32_t k = 0; k < nc; ++k) {
            tile.comps[k].arena_off = arena;
            uint64_t area = (uint64_t)tile.comps[k].r.w() * tile.comps[k].r.h();
            arena += (area + 63) & ~63ull;
            lloff[lt * nc + k] = llarena;
            llarena += ll_geom(tile.comps[k]).elems;
        }
        for (uint32_t k = 0; k < nc; ++k) {
            TileComp &tc = tile.comps[k];
            const BandNeed need = win ? window_need(tc, cwin[k], nullptr, reduce) : BandNeed();
            for_each_cblk(tc, [&](Band &band, Cblk &cb) {
                DecBlock d{};
                d.dst_off = tc.arena_off + (uint64_t)cb.by * tc.r.w() + cb.bx;
                d.dstride = tc.r.w();
                d.w = cb.r.w();
                d.h = cb.r.h();
                d.orient = band.bandno;
                d.irrev = tc.irrev;
                d.step = band.stepsize;
                dsty.push_back(tsty[lt][k]);
                // passes beyond the last bit-plane are not decoded (t1_decode_cblk
                // stops at bpno < 0, t1.cpp:1086-1090)
                d.numpasses = std::min<uint32_t>(cb.numpasses, cb.numbps ? 3 * cb.numbps - 2 : 0);
                d.numbps = cb.numbps;
                d.len = cb.seglen;
                // codeword segments (one unless TERMALL): each points at its
                // bytes in place when they are one contiguous chunk, else at
                // a copy appended after the codestream
                seg_first.push_back((uint32_t)dsegs.size());
                for (const auto &sg : cb.segs) {
                    DecSeg ds{};
                    ds.len = sg.len;
                    ds.npasses = sg.numpasses;
                    if (sg.chunks.size() == 1) {
                        ds.data_off = sg.chunks[0].first;
                    } else if (!sg.chunks.empty()) {
                        ds.data_off = (uint64_t)len + extra.size();  // placed after the codestream
                        for (auto &ch : sg.chunks) {
                            const uint8_t *srcp = csb + ch.first;
                            extra.insert(extra.end(), srcp, srcp + ch.second);
                        }
                    } else {
                        ds.data_off = 0;
                        ds.len = 0;
                    }
                    dsegs.push_back(ds);
                }
                d.data_off = cb.segs.empty() ? 0 : dsegs[seg_first.back()].data_off;
                if (any_roi) droi.push_back(troi[lt][k]);
                // no bytes: the block stays zero (T1Part1::decode returns before
                // t1_decode_cblk when the block has no data, T1Part1.cpp:139-140)
                if (!d.len) d.numpasses = 0;
                // t1_decode_cblk refuses bpno_plus_one = roishift + numbps >= 31
                // (t1.cpp:1055-1060; our numbps already holds the ROI shift, as
                // T1Part1.cpp:186 subtracts it before the call); the decoder's
                // scratch holds 32 planes
                if (d.numpasses && d.numbps >= 31) too_deep = true;
                db.push_back(d);
            }, tc.numres - reduce, win ? &need : nullptr);
        }
    }
    if (too_deep) return set_err(GRKGPU_ECORRUPT, "unsupported bpno_plus_one >= 31 (code-block bit-planes + ROI shift)");
    return GRKGPU_OK;
}

// The Tier-1 launch plan over a block table (seg_first with its total at the
// end): blocks grouped by code-block style -- a launch range each, returned in
// sranges -- and, by t1_dec_sort, in decreasing order of expected work; the
// T1Scratch records the ranges need are returned.
struct StyRange { uint32_t b0, n, sty; uint64_t scr0; };
static uint64_t order_dec_tables(std::vector<DecBlock> &db, std::vector<DecSeg> &dsegs, std::vector<uint32_t> &seg_first,
                                 std::vector<uint8_t> &droi, std::vector<uint8_t> &dsty, bool lone,
                                 std::vector<StyRange> &sranges) {
    const uint32_t nblk = (uint32_t)db.size();
    bool mixed_sty = false;  // tile-components of different code-block styles: one decode launch per style
    for (uint32_t i = 1; i < nblk; ++i) mixed_sty = mixed_sty || dsty[i] != dsty[0];
    const bool sort_work = (dwt_options().t1_dec_sort == 1 || (dwt_options().t1_dec_sort < 0 && lone)) && nblk > 64;
    if (sort_work || mixed_sty) {
        // blocks grouped by style (a launch each), and -- t1_dec_sort -- since
        // lanes of a wavefront run until its slowest block is done, blocks of
        // similar work (pass count, then coded bytes) together, heaviest first
        // (an LSD radix sort of one 48-bit key per block -- style, then
        // passes and bytes descending -- is the comparison sort's stable
        // order at a fraction of its cost: 26 K blocks, ~0.2 vs ~3 ms)
        std::vector<uint64_t> key(nblk);
        for (uint32_t i = 0; i < nblk; ++i) {
            key[i] = (uint64_t)dsty[i] << 40;
            if (sort_work)
                key[i] |= (uint64_t)(255u - std::min<uint32_t>(db[i].numpasses, 255u)) << 32 | (0xFFFFFFFFu - db[i].len);
        }
        std::vector<uint32_t> ord(nblk), tmp(nblk);
        for (uint32_t i = 0; i < nblk; ++i) ord[i] = i;
        for (int sh = 0; sh < 48; sh += 8) {
            uint32_t cnt[257] = {0};
            for (uint32_t i : ord) ++cnt[((key[i] >> sh) & 255u) + 1];
            if (*std::max_element(cnt + 1, cnt + 257) == nblk) continue;  // one digit value: order unchanged
            for (int b = 0; b < 256; ++b) cnt[b + 1] += cnt[b];
            for (uint32_t i : ord) tmp[cnt[(key[i] >> sh) & 255u]++] = i;
            ord.swap(tmp);
        }
        std::vector<DecBlock> db2(nblk);
        std::vector<DecSeg> segs2;
        segs2.reserve(dsegs.size());
        std::vector<uint32_t> first2(nblk + 1);
        std::vector<uint8_t> roi2(droi.size()), sty2(nblk);
        for (uint32_t j = 0; j < nblk; ++j) {
            const uint32_t i = ord[j];
            db2[j] = db[i];
            sty2[j] = dsty[i];
            first2[j] = (uint32_t)segs2.size();
            segs2.insert(segs2.end(), dsegs.begin() + seg_first[i], dsegs.begin() + seg_first[i + 1]);
            if (!droi.empty()) roi2[j] = droi[i];
        }
        first2[nblk] = (uint32_t)segs2.size();
        db.swap(db2);
        dsegs.swap(segs2);
        seg_first.swap(first2);
        droi.swap(roi2);
        dsty.swap(sty2);
    }
    // launch ranges: one per code-block style, each with its own scratch
    // groups (64 blocks each) so the ranges need no alignment
    uint64_t scr_records = 0;
    for (uint32_t i = 0; i < nblk;) {
        uint32_t j = i;
        while (j < nblk && dsty[j] == dsty[i]) ++j;
        sranges.push_back({i, j - i, dsty[i], scr_records});
        scr_records += t1_scratch_records(j - i);
        i = j;
    }
    return scr_records;
}

// The Tier-1 stage of a decode, over one stream's block table or a batch's
// merged one: prepare() orders the tables (in place: order_dec_tables), gives
// every segment its unstuffed-stream region and stages the tables in h_blocks
// and h_segs (segs | seg_first | roi); upload() copies the two to the device
// (after the codestream bytes they point into, inside the caller's H2D
// interval); launch() runs the decoders over ctx->cs into ctx->coef, a launch
// set per style range.  too_large: the caller's message for a table past the
// 32-bit region offsets.
struct DecT1Stage {
    std::vector<StyRange> sranges;
    size_t segbytes = 0, sfbytes = 0, roibytes = 0;
    uint32_t nblk = 0;
    bool lone = false;
    double t_tables = 0;  // the host's clock once the tables are ordered: the end of the stats' host_t2_ms

    int prepare(grkgpu_ctx *c, std::vector<DecBlock> &db, std::vector<DecSeg> &dsegs, std::vector<uint32_t> &seg_first,
                std::vector<uint8_t> &droi, std::vector<uint8_t> &dsty, const char *too_large) {
        nblk = (uint32_t)db.size();
        lone = lone_call();
        const uint64_t scr_records = order_dec_tables(db, dsegs, seg_first, droi, dsty, lone, sranges);
        t_tables = now_ms();
        // the decoder's lane-interleaved groups span 64 records each (t1_lane.h)
        HIPCHK(c->scratch.ensure((size_t)scr_records * sizeof(T1Scratch) + 256));
        // per-segment unstuffed-stream regions (16-byte units)
        uint64_t uwords = 0;
        for (auto &sg : dsegs) {
            sg.ub_off = (uint32_t)(uwords / 4);
            uwords += t1_unstuff_region_words(sg.len);
        }
        if (uwords / 4 > 0xffffffffull) return set_err(GRKGPU_EUNSUPPORTED, too_large);
        segbytes = dsegs.size() * sizeof(DecSeg);
        sfbytes = seg_first.size() * 4;
        roibytes = droi.size();
        HIPCHK(c->segs.ensure(segbytes + sfbytes + roibytes + 256));
        HIPCHK(c->h_segs.ensure(segbytes + sfbytes + roibytes + 256));
        memcpy(c->h_segs.p, dsegs.data(), segbytes);
        memcpy((uint8_t *)c->h_segs.p + segbytes, seg_first.data(), sfbytes);
        if (roibytes) memcpy((uint8_t *)c->h_segs.p + segbytes + sfbytes, droi.data(), roibytes);
        HIPCHK(c->ubuf.ensure(uwords * 4 + 256));
        HIPCHK(c->blocks.ensure((size_t)nblk * sizeof(DecBlock) + 256));
        HIPCHK(c->h_blocks.ensure((size_t)nblk * sizeof(DecBlock) + 256));
        memcpy(c->h_blocks.p, db.data(), (size_t)nblk * sizeof(DecBlock));
        return GRKGPU_OK;
    }
    int upload(grkgpu_ctx *c) const {
        HIPCHK(hipMemcpyAsync(c->blocks.p, c->h_blocks.p, (size_t)nblk * sizeof(DecBlock), hipMemcpyHostToDevice,
                              c->stream));
        HIPCHK(hipMemcpyAsync(c->segs.p, c->h_segs.p, segbytes + sfbytes + roibytes, hipMemcpyHostToDevice, c->stream));
        return GRKGPU_OK;
    }
    int launch(grkgpu_ctx *c, uint32_t *nl) const {
        for (const StyRange &g : sranges) {
            HIPCHK(launch_t1_decode(c->blocks.as<DecBlock>() + g.b0, g.n, c->cs.as<uint8_t>(),
                                    c->scratch.as<T1Scratch>() + g.scr0, c->coef.as<int32_t>(), c->stream,
                                    c->ubuf.as<uint32_t>(), 0, c->segs.as<DecSeg>(),
                                    (const uint32_t *)(c->segs.as<uint8_t>() + segbytes) + g.b0, g.sty,
                                    roibytes ? c->segs.as<uint8_t>() + segbytes + sfbytes + g.b0 : nullptr,
                                    lone ? lone_bpw(nblk) : 0));
            ++*nl;
        }
        return GRKGPU_OK;
    }
};

// the sample range of a precision (1 .. 31) and sign, and the DC shift into it
struct SampleRange { int32_t shift, mn, mx; };
static SampleRange sample_range(uint32_t prec, int32_t sgnd) {
    const int32_t half = (int32_t)(1u << (prec - 1));
    if (sgnd) return {0, -half, half - 1};
    return {half, 0, (int32_t)((1u << prec) - 1)};
}
// ... as component k of a launch's clamp bounds (and shifts)
static void set_range(uint32_t k, uint32_t prec, int32_t sgnd, ShiftArr &mn, ShiftArr &mx, ShiftArr *sh = nullptr) {
    const SampleRange r = sample_range(prec, sgnd);
    mn.v[k] = r.mn; mx.v[k] = r.mx;
    if (sh) sh->v[k] = r.shift;
}
// the sample range a component's decoded values are clamped to
static void clamp_bounds(const CodingParams &cp, uint32_t k, int32_t &mn, int32_t &mx) {
    const SampleRange r = sample_range(cp.prec[k], cp.sgnd[k]);
    mn = r.mn; mx = r.mx;
}
// a sample format holds every value of a precision and sign
static bool fmt_holds(int32_t fmt, uint32_t prec, int32_t sgnd) {
    if (fmt == SMP_I32) return true;
    return (sgnd != 0) == (fmt == SMP_I8 || fmt == SMP_I16) && prec <= 8 * sample_bytes(fmt);
}
// The n destination planes of a store in format fmt (interleaved: the one
// plane of pixels), bound to d where given; a null or misaligned one refuses.
static int bind_dst(void *const *planes, uint32_t n, int32_t fmt, DstPlanes *d = nullptr) {
    for (uint32_t k = 0; k < n; ++k) {
        if (!planes[k] || (uintptr_t)planes[k] % sample_bytes(fmt))
            return set_err(GRKGPU_EINVAL, "null or misaligned output plane");
        if (d) d->p[k] = planes[k];
    }
    return GRKGPU_OK;
}

// Samples nothing decodes are zero (the plain case: no channel map, no colour
// conversion, no upsampling launch that writes them itself): the margin of a
// reduced decode at an odd origin -- the whole of every output region -- or
// the tiles of [tb, te) a cut stream never reached, their regions only (a
// shard's device planes hold other tiles).  dst[k] = output region k on the
// device; *nl grows by the fills issued.
static hipError_t dec_zero_fills(const DecHost &h, void *const *dst, hipStream_t s, uint32_t *nl) {
    const uint32_t nout = h.il ? 1 : h.no;
    const size_t eb = h.il ? (size_t)h.no * h.sb : h.sb;
    if (h.opad) {
        for (uint32_t k = 0; k < nout; ++k, ++*nl) {
            const hipError_t e = hipMemsetAsync(dst[k], 0, h.region_bytes(k), s);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    if (!h.missing || h.up) return hipSuccess;
    for (uint32_t t = h.tb; t < h.te; ++t) {
        if (h.walk.decoded[t] || h.wskip[t]) continue;
        for (uint32_t k = 0; k < nout; ++k) {
            const Rect cr = comp_rect(tile_rect(h.cp, t), h.cp.dx[k], h.cp.dy[k]);
            const Rect rr{ceil_pow2(cr.x0, h.reduce), ceil_pow2(cr.y0, h.reduce), ceil_pow2(cr.x1, h.reduce),
                          ceil_pow2(cr.y1, h.reduce)};
            const Rect o = intersect(rr, h.orect[k]);
            if (o.empty()) continue;
            const uint32_t ow = h.orect[k].w();
            const uint64_t e0 = (uint64_t)(o.y0 - h.orect[k].y0) * ow + (o.x0 - h.orect[k].x0);
            const hipError_t e = hipMemset2DAsync((uint8_t *)dst[k] + e0 * eb, (size_t)ow * eb, 0, (size_t)o.w() * eb,
                                                  o.h(), s);
            if (e != hipSuccess) return e;
            ++*nl;
        }
    }
    return hipSuccess;
}

// the statistics of a decode (grkgpu_get_stats) from the stage events and the host's clock
static void fill_dec_stats(grkgpu_ctx *c, double t_start, double t_tables, double t_end, uint32_t nblk, uint64_t cs_bytes) {
    grkgpu_stats &st = c->stats;
    memset(&st, 0, sizeof(st));
    hipEventElapsedTime(&st.h2d_ms, c->ev[0], c->ev[1]);
    hipEventElapsedTime(&st.t1_ms, c->ev[1], c->ev[2]);
    hipEventElapsedTime(&st.dwt_ms, c->ev[2], c->ev[3]);
    hipEventElapsedTime(&st.dcshift_mct_ms, c->ev[3], c->ev[4]);
    hipEventElapsedTime(&st.d2h_ms, c->ev[4], c->ev[5]);
    log_collect(c);
    st.host_t2_ms = (float)(t_tables - t_start);
    st.total_ms = (float)(t_end - t_start);
    st.num_cblks = nblk;
    st.cs_bytes = cs_bytes;
}

static int decompress_impl(grkgpu_ctx *c, const uint8_t *csb, size_t len, grkgpu_image_desc *img,
                           const DecodeOut &od, uint32_t tb, uint32_t te,
                           uint32_t reduce = 0, const Rect *win = nullptr, uint32_t max_layers = 0,
                           bool host_only = false, std::vector<uint8_t> *decoded_out = nullptr) {
    if ((!c && !host_only) || !csb || (!od.planes && !host_only)) return set_err(GRKGPU_EINVAL, "null argument");
    if (!out_fmt_ok(od)) return set_err(GRKGPU_EINVAL, "unknown sample format");
    ActiveCall active;
    double t_start = now_ms();
    DecHost H;
    H.csb = csb; H.len = len; H.img = img; H.od = od;
    H.tb = tb; H.te = te; H.reduce = reduce; H.win = win; H.max_layers = max_layers; H.host_only = host_only;
    int hrc = H.begin();
    if (hrc) return hrc;
    host_parallel_for(H.nsh, 1, [&](size_t l0, size_t l1) { H.parse_tiles(l0, l1); });
    hrc = H.finish();
    if (hrc) return hrc;
    if (decoded_out) *decoded_out = H.walk.decoded;
    if (host_only) return GRKGPU_OK;
    // the host half's results, under the names the device half below uses
    void *const *const planes = H.planes;
    const int planes_on_device = H.planes_on_device;
    const uint32_t sb = H.sb, ssb = H.ssb, nc = H.nc, no = H.no, iw = H.iw;
    const uint32_t ix0 = H.ix0, iy0 = H.iy0, ix1 = H.ix1, iy1 = H.iy1;
    const bool il = H.il, whole = H.whole, mixed = H.mixed, conv = H.conv, colconv = H.colconv, up = H.up;
    const bool opad = H.opad, missing = H.missing;
    const int32_t sfmt = H.sfmt;
    const CodingParams &cp = H.cp;
    const OutOps &dops = H.dops;
    const ChanMap *const cm = H.cm;
    const Rect *const orect = H.orect, *const cwin = H.cwin;
    const uint64_t *const ooff = H.ooff;
    const std::vector<uint8_t> &wskip = H.wskip;
    const TileWalk &walk = H.walk;
    std::vector<Tile> &tiles = H.tiles;
    const std::vector<int32_t> &tmct = H.tmct;
    const uint64_t arena = H.arena, llarena = H.llarena;
    const std::vector<uint64_t> &lloff = H.lloff;
    std::vector<DecBlock> &db = H.db;
    std::vector<DecSeg> &dsegs = H.dsegs;
    std::vector<uint8_t> &droi = H.droi, &dsty = H.dsty, &extra = H.extra;
    std::vector<uint32_t> &seg_first = H.seg_first;
    tb = H.tb; te = H.te;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    seg_first.push_back((uint32_t)dsegs.size());
    DecT1Stage t1;
    uint32_t nl = 0;  // (the batch's launch count: not reported by this call)
    hrc = t1.prepare(c, db, dsegs, seg_first, droi, dsty, "codestream too large for one call");
    if (hrc) return hrc;
    HIPCHK(c->cs.ensure(len + extra.size() + 256));
    HIPCHK(c->coef.ensure(arena * 4 + 256));
    HIPCHK(c->work.ensure(arena * 4 + 256));
    HIPCHK(c->ll.ensure(llarena * 4 + 256));

    HIPCHK(hipEventRecord(c->ev[0], s));
    HIPCHK(hipMemcpyAsync(c->cs.p, csb, len, hipMemcpyHostToDevice, s));
    if (!extra.empty()) {
        HIPCHK(c->h_packed.ensure(extra.size() + 256));
        memcpy(c->h_packed.p, extra.data(), extra.size());
        HIPCHK(hipMemcpyAsync(c->cs.as<uint8_t>() + len, c->h_packed.p, extra.size(), hipMemcpyHostToDevice, s));
    }
    hrc = t1.upload(c);
    if (hrc) return hrc;
    // one plan per wavelet (COC / tile COD may mix 5/3 and 9/7 components)
    DwtPlan dplan[2];
    for (auto &tile : tiles)
        for (uint32_t k = 0; k < tile.comps.size(); ++k) {
            const TileComp &tc = tile.comps[k];
            // a window decode reconstructs, per level, only the windows over
            // the region the window's samples depend on
            std::vector<Rect> rn;
            if (win) window_need(tc, cwin[k], &rn, reduce);
            dwt_plan_tc(dplan[tc.irrev], tc, c->work.as<int32_t>() + tc.arena_off, c->coef.as<int32_t>() + tc.arena_off,
                        c->ll.as<int32_t>() + lloff[(tile.index - tb) * nc + k], tc.irrev, true, tc.numres - reduce,
                        win ? &rn : nullptr);
        }
    HIPCHK(dwt_upload_plans(c, dplan));
    // window decode: the coefficients of the code-blocks left undecoded are
    // zero (they lie outside every window sample's support; zero keeps the
    // 9/7 float lifting free of stale NaNs)
    if (win && arena) HIPCHK(hipMemsetAsync(c->coef.p, 0, arena * 4, s));
    // a channel map: the table goes to the device with the codestream, inside
    // the H2D interval (uploaded by every call, so nothing of an earlier one
    // is read) -- the store stage's events then bracket launches only
    PalMap pmap{};
    const uint16_t *ptable = nullptr;
    if (cm) {
        pmap.nch = no;
        pmap.ne = cm->table ? cm->ne : 0;
        pmap.npc = cm->table ? cm->npc : 0;
        for (uint32_t ch = 0; ch < no; ++ch) {
            pmap.comp[ch] = (uint8_t)cm->comp[ch];
            pmap.pcol[ch] = (int8_t)cm->pcol[ch];
        }
        set_pal_used(pmap);
        if (pmap.ne) {
            const size_t tbytes = (size_t)pmap.ne * pmap.npc * sizeof(uint16_t);
            HIPCHK(c->pal.ensure(tbytes));
            HIPCHK(hipMemcpyAsync(c->pal.p, cm->table, tbytes, hipMemcpyHostToDevice, s));
            ptable = c->pal.as<uint16_t>();
        }
    }
    HIPCHK(hipEventRecord(c->ev[1], s));
    hrc = t1.launch(c, &nl);
    if (hrc) return hrc;
    HIPCHK(hipEventRecord(c->ev[2], s));
    HIPCHK(dwt_launch_plans(c, dplan, true, &nl));
    HIPCHK(hipEventRecord(c->ev[3], s));
    // the output as the copies and fills see it: `nout` regions (the planes,
    // or the one interleaved image) of elements `eb` bytes wide (a sample, or
    // a pixel of nc samples); region k holds ooff[k + 1] - ooff[k] samples
    // (interleaved: all ooff[nc] of them)
    const uint32_t nout = il ? 1 : no;
    const size_t eb = il ? (size_t)no * sb : sb;
    // upsampled: which components go through a staging plane -- all when they
    // share one subsampled grid (their MCT runs first); otherwise those with a
    // tile boundary that is no multiple of dx / dy, where the tile's first
    // pixels map to a sample of the neighbouring tile-component (it starts at
    // ceil(tx0 / dx)).  The others are read from the tile buffers, like the
    // full-resolution components.
    auto staged = [&](uint32_t k) {
        if (!up || (cp.dx[k] == 1 && cp.dy[k] == 1)) return false;
        const bool xseam = cp.tw > 1 && (cp.tx0 % cp.dx[k] || cp.tdx % cp.dx[k]);
        const bool yseam = cp.th > 1 && (cp.ty0 % cp.dy[k] || cp.tdy % cp.dy[k]);
        return !mixed || xseam || yseam;
    };
    DstPlanes dst{}, stg{};  // stg: the staging planes of an upsampled decode's subsampled components
    {
        // staging image (host planes) and staging planes: every region on a
        // 16-byte boundary, so that the kernel's packed stores stay aligned
        // whatever the sample width
        size_t off[GRKGPU_MAX_COMPS + 1] = {0}, soff[GRKGPU_MAX_COMPS + 1];
        if (!planes_on_device)
            for (uint32_t k = 0; k < nout; ++k) off[k + 1] = (off[k] + H.region_bytes(k) + 15) & ~(size_t)15;
        soff[0] = planes_on_device ? 0 : off[nout];
        for (uint32_t k = 0; k < nc; ++k)
            soff[k + 1] = soff[k] + (staged(k) ? ((size_t)(ooff[k + 1] - ooff[k]) * ssb + 15) & ~(size_t)15 : 0);
        if (soff[nc]) HIPCHK(c->img.ensure(soff[nc] + 256));
        for (uint32_t k = 0; k < nout; ++k)
            dst.p[k] = planes_on_device ? planes[k] : (void *)(c->img.as<uint8_t>() + off[k]);
        for (uint32_t k = 0; k < nc; ++k)
            if (staged(k)) stg.p[k] = c->img.as<uint8_t>() + soff[k];
        // tiles the stream never reached are zero in the staging planes; in
        // the output the upsampling launch writes their pixels
        for (uint32_t k = 0; missing && k < nc; ++k)
            if (staged(k)) HIPCHK(hipMemsetAsync(stg.p[k], 0, soff[k + 1] - soff[k], s));
    }
    auto at = [&](uint32_t k, uint64_t elem) { return (void *)((uint8_t *)dst.p[k] + elem * eb); };
    // where the launches on the components' own grids store component k: the
    // output, or (upsampled) its staging plane
    auto cat = [&](uint32_t k, uint64_t elem) { return up ? (void *)((uint8_t *)stg.p[k] + elem * ssb) : at(k, elem); };
    // The fills below stand for samples nothing decoded: zero, which every
    // precision op maps to zero.  The reference's colour step converts them
    // like any other sample, so with sYCC (no subsampling here: an upsampled
    // decode's launch writes such pixels itself, from null sources) the fill
    // is the converting store run over zero samples -- sYCC(0, 0, 0), then
    // the precision op -- in the output's format and layout.
    auto fill_converted = [&](const Rect &o) -> hipError_t {
        UpPlan zero{};
        for (uint32_t k = 0; k < nc; ++k) zero.c[k].dx = zero.c[k].dy = 1;
        const uint32_t ow = orect[0].w();
        DstPlanes fdst{};
        for (uint32_t k = 0; k < nout; ++k)
            fdst.p[k] = at(k, (uint64_t)(o.y0 - orect[0].y0) * ow + (o.x0 - orect[0].x0));
        return launch_upsample_ops(zero, nc, o.x0, o.y0, o.w(), o.h(), fdst, od.fmt, il, il ? ow * no : ow, dops, s);
    };
    // a channel map's fills: the palette store run over zero samples -- entry 0
    // of each looked-up channel, then the precision op -- since the
    // reference's pass maps the zeros it finds
    auto fill_mapped = [&](const Rect &o) -> hipError_t {
        const uint32_t ow = orect[0].w();
        DstPlanes fdst{};
        for (uint32_t k = 0; k < nout; ++k)
            fdst.p[k] = at(k, (uint64_t)(o.y0 - orect[0].y0) * ow + (o.x0 - orect[0].x0));
        PalMap z = pmap;
        z.zero = 1;
        return launch_palette(PlanePtrs{}, 0, o.w(), o.h(), fdst, od.fmt, il, il ? ow * no : ow, nc, ShiftArr{},
                              ShiftArr{}, ShiftArr{}, 0, 0, z, ptable, conv ? &dops : nullptr, s);
    };
    // A float destination has no zero to memset: samples nothing decoded
    // leave as the normalised precision op of zero (bias, where no colour step
    // runs) -- the same converting store over null sources, on each plane's
    // own grid where the grids differ (planar output, no colour step there).
    const bool fl = H.fl;
    auto fill_plane = [&](uint32_t k, const Rect &o) -> hipError_t {
        UpPlan zero{};
        zero.c[0].dx = zero.c[0].dy = 1;
        DstPlanes fdst{};
        fdst.p[0] = at(k, (uint64_t)(o.y0 - orect[k].y0) * orect[k].w() + (o.x0 - orect[k].x0));
        return launch_upsample_ops(zero, 1, o.x0, o.y0, o.w(), o.h(), fdst, od.fmt, false, orect[k].w(),
                                   plane_ops(dops, k), s);
    };
    if (fl && mixed && !up && (opad || missing)) {
        for (uint32_t k = 0; k < nc; ++k) {
            if (opad) {
                HIPCHK(fill_plane(k, orect[k]));
                continue;
            }
            for (uint32_t t = tb; t < te; ++t) {
                if (walk.decoded[t] || wskip[t]) continue;
                const Rect cr = comp_rect(tile_rect(cp, t), cp.dx[k], cp.dy[k]);
                const Rect o = intersect({ceil_pow2(cr.x0, reduce), ceil_pow2(cr.y0, reduce), ceil_pow2(cr.x1, reduce),
                                          ceil_pow2(cr.y1, reduce)}, orect[k]);
                if (!o.empty()) HIPCHK(fill_plane(k, o));
            }
        }
    } else if (cm && opad) {
        HIPCHK(fill_mapped(orect[0]));
    } else if (cm && missing) {
        for (uint32_t t = tb; t < te; ++t) {
            if (walk.decoded[t] || wskip[t]) continue;
            const Rect cr = tile_rect(cp, t);
            const Rect o = intersect({ceil_pow2(cr.x0, reduce), ceil_pow2(cr.y0, reduce), ceil_pow2(cr.x1, reduce),
                                      ceil_pow2(cr.y1, reduce)}, orect[0]);
            if (!o.empty()) HIPCHK(fill_mapped(o));
        }
    } else if ((colconv || fl) && !up && opad) {
        HIPCHK(fill_converted(orect[0]));
    } else if ((colconv || fl) && !up && missing) {
        for (uint32_t t = tb; t < te; ++t) {
            if (walk.decoded[t] || wskip[t]) continue;
            const Rect cr = comp_rect(tile_rect(cp, t), cp.dx[0], cp.dy[0]);  // (one grid; sYCC: the image's)
            const Rect o = intersect({ceil_pow2(cr.x0, reduce), ceil_pow2(cr.y0, reduce), ceil_pow2(cr.x1, reduce),
                                      ceil_pow2(cr.y1, reduce)}, orect[0]);
            if (!o.empty()) HIPCHK(fill_converted(o));
        }
    } else if (!fl) {  // (float, upsampled: the upsampling launch writes such pixels itself)
        HIPCHK(dec_zero_fills(H, dst.p, s, &nl));
    }
    ShiftArr sh{}, mn{}, mx{};
    for (uint32_t k = 0; k < nc; ++k) {
        sh.v[k] = cp.shift[k];
        clamp_bounds(cp, k, mn.v[k], mx.v[k]);
    }
    MctInv minv{};  // custom MCT (cp.mct == 2): the stream's matrix and offsets instead of the DC shifts
    ShiftArr moff{};
    if (cp.mct == 2) {
        set_mct_inv(minv, cp.mct_decoding, nc);
        for (uint32_t k = 0; k < nc; ++k) moff.v[k] = cp.mct_offsets[k];
    }
    for (auto &tile : tiles) {
        if (tile.comps.empty()) continue;  // outside the window
        if (mixed) {  // each tile-component on its own grid, no MCT
            for (uint32_t k = 0; k < nc; ++k) {
                const TileComp &tc = tile.comps[k];
                const Rect tr = tc.res[tc.numres - 1 - reduce].r;
                const Rect out = intersect(tr, orect[k]);
                if (out.empty() || (up && !staged(k))) continue;
                PlanePtrs tsrc{};
                DstPlanes tdst{};
                ShiftArr sk{}, mnk{}, mxk{};
                tsrc.p[0] = c->work.as<int32_t>() + tc.arena_off + (uint64_t)(out.y0 - tr.y0) * tr.w() + (out.x0 - tr.x0);
                tdst.p[0] = cat(k, (uint64_t)(out.y0 - orect[k].y0) * orect[k].w() + (out.x0 - orect[k].x0));
                sk.v[0] = sh.v[k];
                mnk.v[0] = mn.v[k];
                mxk.v[0] = mx.v[k];
                if (conv && !up) {  // each plane on its own grid, converted
                    const OutOps ok = plane_ops(dops, k);
                    HIPCHK(launch_mct_inv_dcshift_ops(tsrc, tr.w(), out.w(), out.h(), tdst, od.fmt, false,
                                                      orect[k].w(), 1, sk, mnk, mxk, 0, tc.irrev, ok, s));
                    continue;
                }
                HIPCHK(launch_mct_inv_dcshift_to(tsrc, tr.w(), out.w(), out.h(), tdst, up ? sfmt : od.fmt, false,
                                                 orect[k].w(), 1, sk, mnk, mxk, 0, tc.irrev, s));
            }
            continue;
        }
        // every component on one grid: one launch, MCT included (orect[k]
        // is the output on that grid -- the image itself without subsampling)
        PlanePtrs tsrc{};
        DstPlanes tdst{};
        const Rect tr = tile.comps[0].res[tile.comps[0].numres - 1 - reduce].r;  // the tile at the decoded resolution
        const Rect out = intersect(tr, orect[0]);             // its part of the output
        if (out.empty()) continue;
        const uint32_t ow = orect[0].w();
        for (uint32_t k = 0; k < nc; ++k)
            tsrc.p[k] = c->work.as<int32_t>() + tile.comps[k].arena_off + (uint64_t)(out.y0 - tr.y0) * tr.w() +
                        (out.x0 - tr.x0);
        for (uint32_t k = 0; k < (up ? nc : nout); ++k)
            tdst.p[k] = cat(k, (uint64_t)(out.y0 - orect[0].y0) * ow + (out.x0 - orect[0].x0));
        int32_t wmask = 0;  // components holding 9/7 (float) samples
        for (uint32_t k = 0; k < nc; ++k) wmask |= tile.comps[k].irrev << k;
        // row stride in samples: a row of an interleaved image holds ow pixels of nc samples
        if (cm)  // (every component at (1,1); a custom MCT is refused at the COD)
            HIPCHK(launch_palette(tsrc, tr.w(), out.w(), out.h(), tdst, od.fmt, il, il ? ow * no : ow, nc, sh, mn, mx,
                                  tmct[tile.index - tb], wmask, pmap, ptable, conv ? &dops : nullptr, s));
        else if (tmct[tile.index - tb] == 2)  // (every component at (1,1): never upsampled)
            HIPCHK(launch_mct_inv_custom(tsrc, tr.w(), out.w(), out.h(), tdst, od.fmt, il, il ? ow * no : ow, nc, minv,
                                         moff, mn, mx, conv ? &dops : nullptr, s));
        else if (conv && !up)
            HIPCHK(launch_mct_inv_dcshift_ops(tsrc, tr.w(), out.w(), out.h(), tdst, od.fmt, il, il ? ow * no : ow, nc,
                                              sh, mn, mx, tmct[tile.index - tb], wmask, dops, s));
        else
            HIPCHK(launch_mct_inv_dcshift_to(tsrc, tr.w(), out.w(), out.h(), tdst, up ? sfmt : od.fmt, il && !up,
                                             il && !up ? ow * nc : ow, nc, sh, mn, mx, tmct[tile.index - tb], wmask,
                                             s));
    }
    // upsampled: the output, tile by tile (the tiles never reached included)
    for (auto &tile : tiles) {
        const Rect out = intersect(tile.r, {ix0, iy0, ix1, iy1});  // the tile's pixels of the output
        if (!up || out.empty()) continue;
        UpPlan pl{};
        for (uint32_t k = 0; k < nc; ++k) {
            UpComp &u = pl.c[k];
            u.dx = (uint8_t)cp.dx[k];
            u.dy = (uint8_t)cp.dy[k];
            if (staged(k)) {
                u.src = stg.p[k];
                if (conv) u.raw = (uint8_t)(UPCOMP_FIN + sfmt);  // finished samples of the staging format
                u.stride = orect[k].w();
                u.gx0 = (int32_t)orect[k].x0;
                u.gy0 = (int32_t)orect[k].y0;
            } else {  // the tile buffer (a tile never reached: zeros)
                const Rect tr = comp_rect(tile.r, cp.dx[k], cp.dy[k]);
                u.raw = 1;
                u.gx0 = (int32_t)tr.x0;
                u.gy0 = (int32_t)tr.y0;
                u.stride = tr.w();
                if (!tile.comps.empty()) {
                    u.src = c->work.as<int32_t>() + tile.comps[k].arena_off;
                    u.irrev = (uint8_t)tile.comps[k].irrev;
                }
                u.shift = sh.v[k];
                u.mn = mn.v[k];
                u.mx = mx.v[k];
            }
            // the zero lead-in: left of / above the output rectangle's origin on the component's grid
            u.zx0 = std::max((int32_t)orect[k].x0, u.gx0);
            u.zy0 = std::max((int32_t)orect[k].y0, u.gy0);
        }
        DstPlanes tdst{};
        for (uint32_t k = 0; k < nout; ++k) tdst.p[k] = at(k, (uint64_t)(out.y0 - iy0) * iw + (out.x0 - ix0));
        if (conv)
            HIPCHK(launch_upsample_ops(pl, nc, out.x0, out.y0, out.w(), out.h(), tdst, od.fmt, il, il ? iw * no : iw,
                                       dops, s));
        else
            HIPCHK(launch_upsample_to(pl, nc, out.x0, out.y0, out.w(), out.h(), tdst, od.fmt, il, il ? iw * nc : iw,
                                      s));
    }
    HIPCHK(hipEventRecord(c->ev[4], s));
    if (!planes_on_device) {
        if (whole) {
            for (uint32_t k = 0; k < nout; ++k)
                HIPCHK(hipMemcpyAsync(planes[k], dst.p[k], H.region_bytes(k), hipMemcpyDeviceToHost, s));
        } else {  // only the shard's tiles
            for (auto &tile : tiles)
                for (uint32_t k = 0; k < nout; ++k) {
                    const uint64_t o = ((uint64_t)(tile.r.y0 - cp.image.y0) * iw + (tile.r.x0 - cp.image.x0)) * eb;
                    HIPCHK(hipMemcpy2DAsync((uint8_t *)planes[k] + o, (size_t)iw * eb, (uint8_t *)dst.p[k] + o,
                                            (size_t)iw * eb, (size_t)tile.r.w() * eb, tile.r.h(),
                                            hipMemcpyDeviceToHost, s));
                }
        }
    }
    HIPCHK(hipEventRecord(c->ev[5], s));
    HIPCHK(hipStreamSynchronize(s));
    fill_dec_stats(c, t_start, t1.t_tables, now_ms(), t1.nblk, len);
    return GRKGPU_OK;
}

extern "C" int grkgpu_decompress(grkgpu_ctx *c, const uint8_t *csb, size_t len, grkgpu_image_desc *img,
                                 int32_t *const *planes, int planes_on_device) {
    return decompress_impl(c, csb, len, img, i32_planes(planes, planes_on_device), 0, 0xffffffffu);
}

extern "C" int grkgpu_decompress_reduced(grkgpu_ctx *c, const uint8_t *csb, size_t len, uint32_t reduce,
                                         grkgpu_image_desc *img, int32_t *const *planes, int planes_on_device) {
    return decompress_impl(c, csb, len, img, i32_planes(planes, planes_on_device), 0, 0xffffffffu, reduce);
}

extern "C" int grkgpu_decompress_window(grkgpu_ctx *c, const uint8_t *csb, size_t len, uint32_t x0, uint32_t y0,
                                        uint32_t x1, uint32_t y1, grkgpu_image_desc *img, int32_t *const *planes,
                                        int planes_on_device) {
    const Rect w{x0, y0, x1, y1};
    return decompress_impl(c, csb, len, img, i32_planes(planes, planes_on_device), 0, 0xffffffffu, 0, &w);
}

extern "C" int grkgpu_decompress_ex(grkgpu_ctx *c, const uint8_t *csb, size_t len, const grkgpu_dparams *dp,
                                    grkgpu_image_desc *img, int32_t *const *planes, int planes_on_device) {
    if (!dp) return decompress_impl(c, csb, len, img, i32_planes(planes, planes_on_device), 0, 0xffffffffu);
    const bool win = dp->DA_x0 || dp->DA_y0 || dp->DA_x1 || dp->DA_y1;
    const Rect w{dp->DA_x0, dp->DA_y0, dp->DA_x1, dp->DA_y1};
    if (win && (dp->DA_x1 <= dp->DA_x0 || dp->DA_y1 <= dp->DA_y0)) return set_err(GRKGPU_EINVAL, "empty decode area");
    return decompress_impl(c, csb, len, img, i32_planes(planes, planes_on_device), 0, 0xffffffffu, dp->cp_reduce,
                           win ? &w : nullptr, dp->cp_layer);
}

extern "C" int grkgpu_walk_tiles(const uint8_t *csb, size_t len, uint8_t *decoded, uint32_t cap, uint32_t *ntiles) {
    if (!csb || !ntiles) return set_err(GRKGPU_EINVAL, "null argument");
    grkgpu_image_desc d{};
    int rc = grkgpu_read_header(csb, len, &d);
    if (rc) return rc;
    std::vector<uint8_t> dec;
    rc = decompress_impl(nullptr, csb, len, nullptr, i32_planes(nullptr, 0), 0, 0xffffffffu, 0, nullptr, 0, true, &dec);
    if (rc) return rc;
    *ntiles = (uint32_t)dec.size();
    if (decoded)
        for (uint32_t t = 0; t < dec.size() && t < cap; ++t) decoded[t] = dec[t];
    return GRKGPU_OK;
}

static_assert(sizeof(grkgpu_dec_block) == sizeof(DecBlock) && offsetof(grkgpu_dec_block, dst_off) == offsetof(DecBlock, dst_off) &&
                  offsetof(grkgpu_dec_block, numbps) == offsetof(DecBlock, numbps) &&
                  offsetof(grkgpu_dec_block, dstride) == offsetof(DecBlock, dstride) &&
                  offsetof(grkgpu_dec_block, stepsize) == offsetof(DecBlock, step),
              "grkgpu_dec_block is DecBlock");
static_assert(sizeof(grkgpu_dec_seg) == sizeof(DecSeg) && offsetof(grkgpu_dec_seg, npasses) == offsetof(DecSeg, npasses),
              "grkgpu_dec_seg is DecSeg");

extern "C" void grkgpu_dec_tables_free(grkgpu_dec_tables *t) {
    if (!t) return;
    free(t->blocks); free(t->segs); free(t->seg_first); free(t->style); free(t->roi);
    *t = grkgpu_dec_tables{};
}

extern "C" int grkgpu_dec_tables_of(const uint8_t *csb, size_t len, const grkgpu_dparams *dp, grkgpu_dec_tables *t) {
    if (!csb || !t) return set_err(GRKGPU_EINVAL, "null argument");
    *t = grkgpu_dec_tables{};
    const bool win = dp && (dp->DA_x0 || dp->DA_y0 || dp->DA_x1 || dp->DA_y1);
    const Rect w = win ? Rect{dp->DA_x0, dp->DA_y0, dp->DA_x1, dp->DA_y1} : Rect{};
    if (win && (dp->DA_x1 <= dp->DA_x0 || dp->DA_y1 <= dp->DA_y0)) return set_err(GRKGPU_EINVAL, "empty decode area");
    ActiveCall active;
    DecHost H;
    H.csb = csb; H.len = len; H.host_only = true;
    H.reduce = dp ? dp->cp_reduce : 0; H.max_layers = dp ? dp->cp_layer : 0; H.win = win ? &w : nullptr;
    int rc = H.begin();
    if (rc) return rc;
    host_parallel_for(H.nsh, 1, [&](size_t l0, size_t l1) { H.parse_tiles(l0, l1); });
    rc = H.finish();
    if (rc) return rc;
    const size_t nb = H.db.size(), ns = H.dsegs.size();
    if (nb > 0xfffffffeull || ns > 0xffffffffull) return set_err(GRKGPU_EUNSUPPORTED, "codestream too large for one call");
    t->n_blocks = (uint32_t)nb;
    t->n_segs = (uint32_t)ns;
    t->data_bytes = (uint64_t)len + H.extra.size();
    t->coef_elems = H.arena;
    t->ll_elems = H.llarena;
    t->blocks = (grkgpu_dec_block *)malloc(std::max<size_t>(nb, 1) * sizeof(DecBlock));
    t->segs = (grkgpu_dec_seg *)malloc(std::max<size_t>(ns, 1) * sizeof(DecSeg));
    t->seg_first = (uint32_t *)malloc((nb + 1) * sizeof(uint32_t));
    t->style = (uint8_t *)malloc(std::max<size_t>(nb, 1));
    if (!H.droi.empty()) t->roi = (uint8_t *)malloc(nb);
    if (!t->blocks || !t->segs || !t->seg_first || !t->style || (!H.droi.empty() && !t->roi)) {
        grkgpu_dec_tables_free(t);
        return set_err(GRKGPU_EUNSUPPORTED, "out of host memory for the decode tables");
    }
    if (nb) {
        memcpy(t->blocks, H.db.data(), nb * sizeof(DecBlock));
        memcpy(t->seg_first, H.seg_first.data(), nb * sizeof(uint32_t));
        memcpy(t->style, H.dsty.data(), nb);
        if (t->roi) memcpy(t->roi, H.droi.data(), nb);
    }
    if (ns) memcpy(t->segs, H.dsegs.data(), ns * sizeof(DecSeg));
    t->seg_first[nb] = (uint32_t)ns;
    return GRKGPU_OK;
}

extern "C" int grkgpu_decompress_tiles(grkgpu_ctx *c, const uint8_t *csb, size_t len, uint32_t tile_begin,
                                       uint32_t tile_end, int32_t *const *planes, int planes_on_device) {
    return decompress_impl(c, csb, len, nullptr, i32_planes(planes, planes_on_device), tile_begin, tile_end);
}

// grkgpu_out_planes' own rules, checked before anything touches a device
// (floats: the float entry points, which take the float formats and only those)
static const grkgpu_out_ops g_no_ops{};
static int check_out_planes(const grkgpu_out_planes *out, bool floats = false) {
    if (!out) return set_err(GRKGPU_EINVAL, "null argument");
    if (floats && !float_fmt((int32_t)out->sample_fmt))
        return set_err(GRKGPU_EINVAL, "a float decode needs GRKGPU_SAMPLE_F32 / _F16 / _BF16");
    if (!floats && out->sample_fmt > GRKGPU_SAMPLE_I16) return set_err(GRKGPU_EINVAL, "unknown sample format");
    if ((out->layout & ~GRKGPU_LAYOUT_UPSAMPLE) > GRKGPU_LAYOUT_INTERLEAVED)
        return set_err(GRKGPU_EINVAL, "unknown layout");
    return GRKGPU_OK;
}

static int decompress_to_impl(grkgpu_ctx *c, const uint8_t *csb, size_t len, const grkgpu_dparams *dp,
                              uint32_t tile_begin, uint32_t tile_end, grkgpu_image_desc *img,
                              const grkgpu_out_planes *out, const grkgpu_out_ops *ops, bool custom_mct = false,
                              const ChanMap *chan = nullptr, bool is_rgb = false, bool floats = false,
                              const grkgpu_out_norm *norm = nullptr) {
    int rc = check_out_planes(out, floats);
    if (rc) return rc;
    rc = check_out_ops(ops, out->sample_fmt);
    if (rc) return rc;
    if (floats && ops && (ops->colour & GRKGPU_COLOUR_FORCE_RGB))
        return set_err(GRKGPU_EUNSUPPORTED, "force-RGB is not supported with a float destination");
    const DecodeOut od{out->planes, (int32_t)out->sample_fmt,
                       (out->layout & ~GRKGPU_LAYOUT_UPSAMPLE) == GRKGPU_LAYOUT_INTERLEAVED, out->on_device,
                       (out->layout & GRKGPU_LAYOUT_UPSAMPLE) != 0,
                       out_ops_active(ops) ? ops : (floats ? &g_no_ops : nullptr),
                       custom_mct ? 1 : 0, chan, is_rgb ? 1 : 0, floats ? 1 : 0, floats ? norm : nullptr};
    if (!dp) return decompress_impl(c, csb, len, img, od, tile_begin, tile_end);
    const bool win = dp->DA_x0 || dp->DA_y0 || dp->DA_x1 || dp->DA_y1;
    const Rect w{dp->DA_x0, dp->DA_y0, dp->DA_x1, dp->DA_y1};
    if (win && (dp->DA_x1 <= dp->DA_x0 || dp->DA_y1 <= dp->DA_y0)) return set_err(GRKGPU_EINVAL, "empty decode area");
    return decompress_impl(c, csb, len, img, od, tile_begin, tile_end, dp->cp_reduce, win ? &w : nullptr,
                           dp->cp_layer);
}

extern "C" int grkgpu_decompress_to(grkgpu_ctx *c, const uint8_t *csb, size_t len, const grkgpu_dparams *dp,
                                    uint32_t tile_begin, uint32_t tile_end, grkgpu_image_desc *img,
                                    const grkgpu_out_planes *out) {
    return decompress_to_impl(c, csb, len, dp, tile_begin, tile_end, img, out, nullptr);
}

extern "C" int grkgpu_decompress_convert(grkgpu_ctx *c, const uint8_t *csb, size_t len, const grkgpu_dparams *dp,
                                         uint32_t tile_begin, uint32_t tile_end, grkgpu_image_desc *img,
                                         const grkgpu_out_planes *out, const grkgpu_out_ops *ops) {
    return decompress_to_impl(c, csb, len, dp, tile_begin, tile_end, img, out, ops);
}

extern "C" int grkgpu_decompress_float(grkgpu_ctx *c, const uint8_t *csb, size_t len, const grkgpu_dparams *dp,
                                       uint32_t tile_begin, uint32_t tile_end, grkgpu_image_desc *img,
                                       const grkgpu_out_planes *out, const grkgpu_out_ops *ops,
                                       const grkgpu_out_norm *norm) {
    return decompress_to_impl(c, csb, len, dp, tile_begin, tile_end, img, out, ops, false, nullptr, false, true, norm);
}

extern "C" int grkgpu_decompress_mct(grkgpu_ctx *c, const uint8_t *csb, size_t len, const grkgpu_dparams *dp,
                                     uint32_t tile_begin, uint32_t tile_end, grkgpu_image_desc *img,
                                     const grkgpu_out_planes *out, const grkgpu_out_ops *ops) {
    return decompress_to_impl(c, csb, len, dp, tile_begin, tile_end, img, out, ops, true);
}

// ---------------------------------------------------------------------------
// Batch decode (grkgpu_decompress_batch): the host half of decompress_impl
// (DecHost) per item, items and tiles in parallel on the host pool; the
// items' tables rebased into one DecBlock / DecSeg table and one DwtPlan per
// wavelet -- codestreams back to back in ctx->cs, each on a 16-byte boundary
// with its multi-chunk bytes behind it, the coef / work / ll arenas item
// after item -- then the device half once: one H2D of the packed streams, the
// Tier-1 launches of a single call of that many blocks, the inverse DWT, and
// the last store from a StoreJob table, one launch per (sample format,
// layout) present.
// ---------------------------------------------------------------------------
static_assert(sizeof(grkgpu_store_job) == sizeof(StoreJob) && offsetof(grkgpu_store_job, dst) == offsetof(StoreJob, dst) &&
                  offsetof(grkgpu_store_job, src_stride) == offsetof(StoreJob, sstride) &&
                  offsetof(grkgpu_store_job, numcomps) == offsetof(StoreJob, ncomp) &&
                  offsetof(grkgpu_store_job, wavelet_mask) == offsetof(StoreJob, irrev) &&
                  offsetof(grkgpu_store_job, shift) == offsetof(StoreJob, shift) &&
                  offsetof(grkgpu_store_job, max) == offsetof(StoreJob, mx),
              "grkgpu_store_job is StoreJob");

// A job table: the records of a launch set's jobs of one type, in groups.  A
// group's key selects its launch: the sample format, the layout (stores: 1
// interleaved) or load mode, and -- StoreJobs with ops -- the op class (OP_*:
// 1 precision, 2 sYCC, 3 eYCC, 4 CMYK) or -- ConvJobs -- the thread shape (bit
// 0 run shape, bit 1 sYCC).  Groups in order of first use; a group's records
// in table order, `first` their first-workgroup numbers.
struct JobKey {
    int32_t fmt;
    int mode, cls;
    bool operator==(const JobKey &o) const { return fmt == o.fmt && mode == o.mode && cls == o.cls; }
};
template <typename J>
struct JobTable {
    struct Group {
        JobKey key;
        std::vector<J> jobs;
        std::vector<uint32_t> first;
    };
    std::vector<Group> groups;
    uint32_t njobs = 0;
    // false: not tabled, the job takes a launch of its own -- more workgroups
    // than the kernels' 32-bit thread index holds, or than a grid takes
    bool add(const JobKey &key, const J &j, uint64_t wgs) {
        Group *g = nullptr;
        for (Group &q : groups)
            if (q.key == key) g = &q;
        if (wgs > STORE_JOB_MAX_WGS || (g ? g->first.back() : 0) + wgs > 0x7fffffffull) return false;
        if (!g) {
            groups.push_back(Group{key, {}, {0}});
            g = &groups.back();
        }
        g->jobs.push_back(j);
        g->first.push_back(g->first.back() + (uint32_t)wgs);
        ++njobs;
        return true;
    }
    // In a buffer the records of every group lie back to back from `rec` on and
    // the first arrays from `fst` on (alone in its buffer: fst = rec_bytes()).
    size_t rec_bytes() const { return (size_t)njobs * sizeof(J); }
    size_t first_bytes() const { return ((size_t)njobs + groups.size()) * 4; }
    size_t bytes() const { return rec_bytes() + first_bytes(); }
    // the one walk over that layout: f(group, offset of its records, offset of its first array)
    template <typename F>
    hipError_t walk(size_t rec, size_t fst, F &&f) const {
        for (const Group &g : groups) {
            const hipError_t e = f(g, rec, fst);
            if (e != hipSuccess) return e;
            rec += g.jobs.size() * sizeof(J);
            fst += g.first.size() * 4;
        }
        return hipSuccess;
    }
    // the table into a staging buffer -> the bytes written
    size_t fill(uint8_t *stage, size_t rec, size_t fst) const {
        size_t b = 0;
        walk(rec, fst, [&](const Group &g, size_t r, size_t f) {
            memcpy(stage + r, g.jobs.data(), g.jobs.size() * sizeof(J));
            memcpy(stage + f, g.first.data(), g.first.size() * 4);
            b += g.jobs.size() * sizeof(J) + g.first.size() * 4;
            return hipSuccess;
        });
        return b;
    }
    // launch(records, first, njobs, nwgs, key) for every group with workgroups, the table at `dev` as filled
    template <typename L>
    hipError_t launch(const void *dev, size_t rec, size_t fst, uint32_t *nl, L &&launch) const {
        return walk(rec, fst, [&](const Group &g, size_t r, size_t f) {
            if (!g.first.back()) return hipSuccess;
            const hipError_t e = launch((const J *)((const uint8_t *)dev + r), (const uint32_t *)((const uint8_t *)dev + f),
                                        (uint32_t)g.jobs.size(), g.first.back(), g.key);
            if (e == hipSuccess && nl) ++*nl;
            return e;
        });
    }
};
// `filled` bytes of tables, staged at `stage`, to the device (the fills' sum against the layout's size)
static hipError_t upload_tables(const uint8_t *stage, void *dev, size_t filled, size_t bytes, hipStream_t s) {
    assert(filled == bytes);
    return bytes ? hipMemcpyAsync(dev, stage, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
}

// What the job tables do not take (more than four components, or too many
// workgroups for one job), launched tile by tile: the arguments of
// launch_mct_inv_dcshift_to, of launch_mct_inv_dcshift_ops and of
// launch_upsample_to / _ops (conv).
struct TileStore {
    PlanePtrs src;
    DstPlanes dst;
    uint32_t sstride, w, h, dstride, nc;
    int32_t fmt, mct, wmask;
    bool il;
    ShiftArr sh, mn, mx;
};
struct TileOpsStore {
    TileStore ts;
    OutOps o;
};
struct TileConv {
    UpPlan pl;
    uint32_t nc;
    Rect r;
    DstPlanes dst;
    int32_t fmt;
    bool il;
    uint32_t dstride;
    OutOps o;
    bool conv;
};
// ... and of launch_palette (a mapped item's tile or fill that the PalJob table does not take): the ops when
// conv, the item's table `table_off` entries into the launch set's merged table (not read when map.ne = 0)
struct TilePal {
    TileStore ts;
    PalMap map;
    uint32_t table_off;
    bool conv;
    OutOps o;
};
// a tile as a record (nc <= 4) and back
static StoreJob store_job_of(const TileStore &ts) {
    StoreJob j{};
    for (uint32_t k = 0; k < 4; ++k) {
        j.src[k] = ts.src.p[k];
        j.dst[k] = ts.dst.p[k];
        j.shift[k] = ts.sh.v[k]; j.mn[k] = ts.mn.v[k]; j.mx[k] = ts.mx.v[k];
    }
    j.sstride = ts.sstride; j.dstride = ts.dstride; j.w = ts.w; j.h = ts.h;
    j.ncomp = ts.nc; j.mct = ts.mct; j.irrev = (uint32_t)ts.wmask;
    return j;
}
static TileStore tile_store_of(const StoreJob &j, int32_t fmt, bool il) {
    TileStore ts{};
    for (uint32_t k = 0; k < j.ncomp; ++k) {
        ts.src.p[k] = const_cast<int32_t *>(j.src[k]);
        ts.sh.v[k] = j.shift[k]; ts.mn.v[k] = j.mn[k]; ts.mx.v[k] = j.mx[k];
    }
    for (uint32_t k = 0; k < (il ? 1u : j.ncomp); ++k) ts.dst.p[k] = j.dst[k];
    ts.sstride = j.sstride; ts.w = j.w; ts.h = j.h; ts.dstride = j.dstride; ts.nc = j.ncomp;
    ts.fmt = fmt; ts.il = il; ts.mct = j.mct; ts.wmask = (int32_t)j.irrev;
    return ts;
}

// The last store of a launch set (grkgpu_decompress_batch / _convert and the
// two stage calls): plain StoreJobs, StoreJobs with ops, ConvJobs, the OutOps
// the jobs index, and the per-tile launches.  One device buffer holds the
// tables: the records of each (sizes multiples of 8, from a 16-byte
// boundary), the OutOps, then every first array.
//
// The stores through a channel map (a JP2 item with a palette, a channel swap
// or force-RGB) are PalJobs in two tables of their own: pal_fill, the zero jobs
// over samples nothing decoded, and pal, the tiles.  A fill that stands for a
// reduced decode's margin covers its item's whole output, tiles included, so
// every fill launches before every tile store: the fills are the earlier
// phase, and same-stream order carries the dependency.  A group's key: the
// sample format, mode = pal_job_shape, cls = the table's LDS class
// (pal_lds_class) + 4 with ops.  pal_table: the merged table on the device.
static_assert(sizeof(StoreJob) % 8 == 0 && sizeof(ConvJob) % 8 == 0 && sizeof(OutOps) % 8 == 0 && sizeof(PalJob) % 8 == 0,
              "table records stay aligned");
struct StorePlan {
    JobTable<StoreJob> plain, conv;
    JobTable<ConvJob> up;
    JobTable<PalJob> pal_fill, pal;
    std::vector<OutOps> ops;
    std::vector<TileStore> singles;
    std::vector<TileOpsStore> conv_singles;
    std::vector<TileConv> up_singles;
    std::vector<TilePal> pal_singles;  // (the fills among them have map.zero set)
    const uint16_t *pal_table = nullptr;

    uint32_t njobs() const { return plain.njobs + conv.njobs + up.njobs + pal_fill.njobs + pal.njobs; }
    // a store through a channel map: o = its ops (entry ops_index) or null; false: not tabled (the caller keeps
    // it as a TilePal)
    bool add_pal(int32_t fmt, bool il, const OutOps *o, PalJob j, uint32_t ops_index) {
        if (j.s.ncomp > 4 || j.map.nch > 4) return false;
        j.s.ops = ops_index;
        const int shape = pal_job_shape(j.map.nch, il);
        const JobKey key{fmt, shape, pal_lds_class(j.map.ne, j.map.npc) + (o ? 4 : 0)};
        return (j.map.zero ? pal_fill : pal).add(key, j, pal_job_wgs(j, sample_bytes(fmt), shape));
    }
    bool add_store(int32_t fmt, bool il, const StoreJob &j) {
        return plain.add({fmt, il, 0}, j, store_job_wgs(j, sample_bytes(fmt), il));
    }
    // the op class of a store on one grid is launch_mct_inv_dcshift_ops' choice
    bool add_conv_store(int32_t fmt, bool il, const OutOps &o, StoreJob j, uint32_t ops_index) {
        j.ops = ops_index;
        const int cls = o.col == COL_EYCC ? 3 : (o.col == COL_CMYK ? 4 : (o.sycc ? 2 : 1));
        return conv.add({fmt, il, cls}, j, store_job_wgs(j, sample_bytes(fmt), il));
    }
    bool add_up(int32_t fmt, bool il, const OutOps &o, ConvJob j, uint32_t ops_index) {
        j.ops = ops_index;
        const bool fast = conv_job_fast(j.c, j.ncomp, fmt, o.col);
        return up.add({fmt, il, (fast ? 1 : 0) | (fast && o.sycc ? 2 : 0)}, j, conv_job_wgs(j, sample_bytes(fmt), fast));
    }

    // the buffer: the five tables' records at rec[] (plain, conv, up, pal_fill, pal), the OutOps, the first
    // arrays at fst[]
    struct Places { size_t rec[5], ops, fst[5], end; };
    Places places() const {
        Places p{};
        p.rec[1] = plain.rec_bytes();
        p.rec[2] = p.rec[1] + conv.rec_bytes();
        p.rec[3] = p.rec[2] + up.rec_bytes();
        p.rec[4] = p.rec[3] + pal_fill.rec_bytes();
        p.ops = p.rec[4] + pal.rec_bytes();
        p.fst[0] = p.ops + ops.size() * sizeof(OutOps);
        p.fst[1] = p.fst[0] + plain.first_bytes();
        p.fst[2] = p.fst[1] + conv.first_bytes();
        p.fst[3] = p.fst[2] + up.first_bytes();
        p.fst[4] = p.fst[3] + pal_fill.first_bytes();
        p.end = p.fst[4] + pal.first_bytes();
        return p;
    }
    size_t bytes() const { return places().end; }
    hipError_t upload(uint8_t *stage, void *dev, hipStream_t s) const {
        const Places p = places();
        if (!ops.empty()) memcpy(stage + p.ops, ops.data(), ops.size() * sizeof(OutOps));
        const size_t filled = plain.fill(stage, p.rec[0], p.fst[0]) + conv.fill(stage, p.rec[1], p.fst[1]) +
                              up.fill(stage, p.rec[2], p.fst[2]) + pal_fill.fill(stage, p.rec[3], p.fst[3]) +
                              pal.fill(stage, p.rec[4], p.fst[4]) + ops.size() * sizeof(OutOps);
        return upload_tables(stage, dev, filled, p.end, s);
    }
    // Phase 1, the stores on the components' own grids, then phase 2, the
    // upsampling / converting stores (same-stream order carries the
    // dependency); in each the tables, then the per-tile launches.
    hipError_t launch(const void *dev, hipStream_t s, uint32_t *nl) const {
        const Places p = places();
        const OutOps *const dops = (const OutOps *)((const uint8_t *)dev + p.ops);
        hipError_t e = plain.launch(dev, p.rec[0], p.fst[0], nl,
                                    [&](const StoreJob *j, const uint32_t *first, uint32_t n, uint32_t nwg, const JobKey &k) {
                                        return launch_store_jobs(j, first, n, nwg, k.fmt, k.mode != 0, s);
                                    });
        if (e == hipSuccess)
            e = conv.launch(dev, p.rec[1], p.fst[1], nl,
                            [&](const StoreJob *j, const uint32_t *first, uint32_t n, uint32_t nwg, const JobKey &k) {
                                return launch_store_jobs(j, first, n, nwg, k.fmt, k.mode != 0, s, k.cls, dops);
                            });
        for (size_t i = 0; e == hipSuccess && i < singles.size(); ++i) {
            const TileStore &ts = singles[i];
            e = launch_mct_inv_dcshift_to(ts.src, ts.sstride, ts.w, ts.h, ts.dst, ts.fmt, ts.il, ts.dstride, ts.nc, ts.sh,
                                          ts.mn, ts.mx, ts.mct, ts.wmask, s);
            if (e == hipSuccess && nl) ++*nl;
        }
        for (size_t i = 0; e == hipSuccess && i < conv_singles.size(); ++i) {
            const TileStore &ts = conv_singles[i].ts;
            e = launch_mct_inv_dcshift_ops(ts.src, ts.sstride, ts.w, ts.h, ts.dst, ts.fmt, ts.il, ts.dstride, ts.nc, ts.sh,
                                           ts.mn, ts.mx, ts.mct, ts.wmask, conv_singles[i].o, s);
            if (e == hipSuccess && nl) ++*nl;
        }
        if (e == hipSuccess)
            e = up.launch(dev, p.rec[2], p.fst[2], nl,
                          [&](const ConvJob *j, const uint32_t *first, uint32_t n, uint32_t nwg, const JobKey &k) {
                              return launch_conv_jobs(j, first, n, nwg, dops, k.fmt, k.mode != 0, (k.cls & 1) != 0,
                                                      (k.cls & 2) != 0, s);
                          });
        for (size_t i = 0; e == hipSuccess && i < up_singles.size(); ++i) {
            const TileConv &t = up_singles[i];
            e = t.conv ? launch_upsample_ops(t.pl, t.nc, t.r.x0, t.r.y0, t.r.w(), t.r.h(), t.dst, t.fmt, t.il, t.dstride, t.o, s)
                       : launch_upsample_to(t.pl, t.nc, t.r.x0, t.r.y0, t.r.w(), t.r.h(), t.dst, t.fmt, t.il, t.dstride, s);
            if (e == hipSuccess && nl) ++*nl;
        }
        // the stores through a channel map (other items' outputs than the launches above write): the fills,
        // tabled and per rectangle, then the tiles
        const auto pal_launch = [&](const PalJob *j, const uint32_t *first, uint32_t n, uint32_t nwg, const JobKey &k) {
            return launch_palette_jobs(j, first, n, nwg, k.fmt, k.mode, (k.cls & 4) ? 1 : 0, (k.cls & 4) ? dops : nullptr,
                                       pal_table, pal_lds_bytes(k.cls & 3), s);
        };
        const auto pal_tiles = [&](bool zero) {
            for (size_t i = 0; e == hipSuccess && i < pal_singles.size(); ++i) {
                const TilePal &t = pal_singles[i];
                if ((t.map.zero != 0) != zero) continue;
                const TileStore &ts = t.ts;
                e = launch_palette(ts.src, ts.sstride, ts.w, ts.h, ts.dst, ts.fmt, ts.il, ts.dstride, ts.nc, ts.sh, ts.mn,
                                   ts.mx, ts.mct, ts.wmask, t.map, t.map.ne ? pal_table + t.table_off : nullptr,
                                   t.conv ? &t.o : nullptr, s);
                if (e == hipSuccess && nl) ++*nl;
            }
        };
        if (e == hipSuccess) e = pal_fill.launch(dev, p.rec[3], p.fst[3], nl, pal_launch);
        pal_tiles(true);
        if (e == hipSuccess) e = pal.launch(dev, p.rec[4], p.fst[4], nl, pal_launch);
        pal_tiles(false);
        return e;
    }

    // a stage call's run: the tables in a buffer of the call's own, freed once the stream has drained
    int run_alone(hipStream_t s) const {
        std::vector<uint8_t> stage(bytes());
        void *dev = nullptr;
        if (bytes()) HIPCHK(hipMalloc(&dev, bytes()));
        hipError_t e = upload(stage.data(), dev, s);
        if (e == hipSuccess) e = launch(dev, s, nullptr);
        const hipError_t es = hipStreamSynchronize(s);
        if (dev) hipFree(dev);
        HIPCHK(e);
        HIPCHK(es);
        return GRKGPU_OK;
    }
};


// Where an item of a batch lies on the device: its tile buffers from work0,
// its host-bound output regions at img0 + roff[k], its staging planes at
// img0 + stoff[k] (host half only: all null).
struct ItemBases {
    uintptr_t work0, img0;
    const size_t *roff, *stoff;
    bool host_only;
    uint32_t pal_off = 0;  // a mapped item's table in the merged table, in entries
    uintptr_t dst(const DecHost &h, uint32_t k) const {
        if (host_only) return 0;
        return h.planes_on_device ? (uintptr_t)h.planes[k] : img0 + roff[k];
    }
};
// The upsampling / converting store of rectangle r of the reference grid from
// pl to dst: a ConvJob where the table takes it -- indexing the item's entry
// of the OutOps table (all zero where it converts nothing), made when first
// needed --, else a per-tile launch.
static void plan_conv(StorePlan &P, const DecHost &h, uint32_t &ops_at, const UpPlan &pl, const Rect &r,
                      const DstPlanes &dst, uint32_t dstride) {
    if (h.nc <= 4) {
        ConvJob j{};
        for (uint32_t k = 0; k < h.nc; ++k) {
            j.c[k] = pl.c[k];
            if (h.staged(k)) j.c[k].raw = (uint8_t)(UPCOMP_FIN + h.sfmt);  // (a table's finished source names its format)
        }
        for (uint32_t k = 0; k < h.nout(); ++k) j.dst[k] = dst.p[k];
        j.X0 = r.x0; j.Y0 = r.y0; j.x1 = r.x1; j.y1 = r.y1;
        j.dstride = dstride; j.ncomp = h.nc;
        if (ops_at == 0xffffffffu) { ops_at = (uint32_t)P.ops.size(); P.ops.push_back(h.dops); }
        if (P.add_up(h.od.fmt, h.il, h.dops, j, ops_at)) return;
    }
    P.up_singles.push_back(TileConv{pl, h.nc, r, dst, h.od.fmt, h.il, dstride, h.dops, h.conv});
}
// The last store of one item, decompress_impl's launches as records: a
// StoreJob per tile (per tile-component of a mixed-grid item) for the stores on
// the components' own grids -- with an ops index where that store converts
// (DecHost::grid_ops) --, a ConvJob per tile of an upsampled item and per
// rectangle of converted zeros, and per-tile launches for what no table takes.
// An item with a channel map (h.cm: every component at (1,1), no colour
// conversion): a PalJob per decoded tile, where decompress_impl launches the
// palette store, and a zero PalJob where it calls fill_mapped -- the whole
// output when it extends past the decoded samples (opad), else the tiles the
// stream never reached; StorePlan launches the fills ahead of the tiles.
static void plan_item_stores(StorePlan &P, const DecHost &h, const ItemBases &B) {
    const uint32_t nc = h.nc, no = h.no, nout = h.nout(), ow = h.orect[0].w();
    const size_t eb = h.il ? (size_t)no * h.sb : h.sb;
    const bool gops = h.grid_ops();
    uint32_t ops_at = 0xffffffffu, kops_at[GRKGPU_MAX_COMPS];  // the item's entries of the OutOps table, made when first needed
    for (uint32_t k = 0; k < GRKGPU_MAX_COMPS; ++k) kops_at[k] = 0xffffffffu;
    // where the stores on the components' own grids put component k: the
    // output, or (upsampled) its staging plane, in format gfmt
    const int32_t gfmt = h.up ? h.sfmt : h.od.fmt;
    auto cat = [&](uint32_t k, uint64_t elem) {
        return h.up ? (void *)(B.img0 + B.stoff[k] + elem * h.ssb) : (void *)(B.dst(h, k) + elem * eb);
    };
    // a store on the components' own grids: tabled, plain or with ops o (entry ops_index), or per tile
    auto store = [&](const TileStore &ts, const OutOps *o, uint32_t ops_index) {
        const bool tabled = ts.nc <= 4 && (o ? P.add_conv_store(ts.fmt, ts.il, *o, store_job_of(ts), ops_index)
                                             : P.add_store(ts.fmt, ts.il, store_job_of(ts)));
        if (!tabled && o) P.conv_singles.push_back(TileOpsStore{ts, *o});
        else if (!tabled) P.singles.push_back(ts);
    };
    PalMap pmap{};
    if (h.cm) {
        pmap.nch = no;
        pmap.ne = h.cm->table ? h.cm->ne : 0;
        pmap.npc = h.cm->table ? h.cm->npc : 0;
        for (uint32_t ch = 0; ch < no; ++ch) {
            pmap.comp[ch] = (uint8_t)h.cm->comp[ch];
            pmap.pcol[ch] = (int8_t)h.cm->pcol[ch];
        }
        set_pal_used(pmap);
    }
    auto pal_store = [&](const TileStore &ts, bool zero) {
        PalJob j{};
        j.s = store_job_of(ts);
        j.map = pmap;
        j.map.zero = zero ? 1 : 0;
        j.table_off = pmap.ne ? B.pal_off : 0;
        if (h.conv && nc <= 4 && no <= 4 && ops_at == 0xffffffffu) { ops_at = (uint32_t)P.ops.size(); P.ops.push_back(h.dops); }
        if (!P.add_pal(ts.fmt, ts.il, h.conv ? &h.dops : nullptr, j, h.conv ? ops_at : 0))
            P.pal_singles.push_back(TilePal{ts, j.map, j.table_off, h.conv, h.dops});
    };
    auto pal_fill = [&](const Rect &o) {
        if (o.empty()) return;
        TileStore ts{};
        for (uint32_t k = 0; k < nout; ++k)
            ts.dst.p[k] = (void *)(B.dst(h, k) + ((uint64_t)(o.y0 - h.orect[0].y0) * ow + (o.x0 - h.orect[0].x0)) * eb);
        ts.w = o.w(); ts.h = o.h(); ts.dstride = h.il ? ow * no : ow; ts.nc = nc; ts.fmt = h.od.fmt; ts.il = h.il;
        pal_store(ts, true);
    };
    if (h.cm && h.opad) {
        pal_fill(h.orect[0]);
    } else if (h.cm && h.missing) {
        for (uint32_t t = h.tb; t < h.te; ++t) {
            if (h.walk.decoded[t] || h.wskip[t]) continue;
            const Rect cr = tile_rect(h.cp, t);
            pal_fill(intersect({ceil_pow2(cr.x0, h.reduce), ceil_pow2(cr.y0, h.reduce), ceil_pow2(cr.x1, h.reduce),
                                ceil_pow2(cr.y1, h.reduce)}, h.orect[0]));
        }
    }
    for (uint32_t lt = 0; lt < h.nsh; ++lt) {
        const Tile &tile = h.tiles[lt];
        if (!tile.comps.empty() && h.mixed) {  // each tile-component on its own grid, no MCT
            for (uint32_t k = 0; k < nc; ++k) {
                const TileComp &tc = tile.comps[k];
                const Rect tr = h.tile_res(lt, k), out = intersect(tr, h.orect[k]);
                if (out.empty() || (h.up && !h.staged(k))) continue;
                TileStore ts{};
                ts.src.p[0] = (int32_t *)(B.work0 + (tc.arena_off + (uint64_t)(out.y0 - tr.y0) * tr.w() + (out.x0 - tr.x0)) * 4);
                ts.dst.p[0] = cat(k, (uint64_t)(out.y0 - h.orect[k].y0) * h.orect[k].w() + (out.x0 - h.orect[k].x0));
                ts.sh.v[0] = h.cp.shift[k];
                clamp_bounds(h.cp, k, ts.mn.v[0], ts.mx.v[0]);
                ts.sstride = tr.w(); ts.dstride = h.orect[k].w(); ts.w = out.w(); ts.h = out.h();
                ts.nc = 1; ts.wmask = tc.irrev; ts.fmt = gops ? h.od.fmt : gfmt;
                if (gops) {  // each plane on its own grid, converted
                    const OutOps ok = plane_ops(h.dops, k);
                    if (kops_at[k] == 0xffffffffu) { kops_at[k] = (uint32_t)P.ops.size(); P.ops.push_back(ok); }
                    store(ts, &ok, kops_at[k]);
                } else {
                    store(ts, nullptr, 0);
                }
            }
        } else if (!tile.comps.empty()) {
            // every component on one grid: one job, MCT included (orect[k] is the
            // output on that grid -- the image itself without subsampling)
            const Rect tr = h.tile_res(lt, 0);            // the tile at the decoded resolution
            const Rect out = intersect(tr, h.orect[0]);  // its part of the output
            if (!out.empty()) {
                const uint64_t soff = (uint64_t)(out.y0 - tr.y0) * tr.w() + (out.x0 - tr.x0);
                const uint64_t delem = (uint64_t)(out.y0 - h.orect[0].y0) * ow + (out.x0 - h.orect[0].x0);
                const bool pil = h.il && !h.up;  // (staging planes are planes)
                int32_t wmask = 0;  // components holding 9/7 (float) samples
                for (uint32_t k = 0; k < nc; ++k) wmask |= tile.comps[k].irrev << k;
                TileStore ts{};
                for (uint32_t k = 0; k < nc; ++k) {
                    ts.src.p[k] = (int32_t *)(B.work0 + (tile.comps[k].arena_off + soff) * 4);
                    ts.sh.v[k] = h.cp.shift[k];
                    clamp_bounds(h.cp, k, ts.mn.v[k], ts.mx.v[k]);
                }
                for (uint32_t k = 0; k < (h.up ? nc : nout); ++k) ts.dst.p[k] = cat(k, delem);
                ts.sstride = tr.w(); ts.w = out.w(); ts.h = out.h();
                ts.dstride = pil ? ow * no : ow;  // (h.il: ow * no fits 32 bits, checked by begin())
                ts.nc = nc; ts.fmt = gops ? h.od.fmt : gfmt; ts.il = pil; ts.mct = h.tmct[lt]; ts.wmask = wmask;
                if (h.cm) {
                    ts.fmt = h.od.fmt;
                    pal_store(ts, false);
                } else if (gops) {
                    if (nc <= 4 && ops_at == 0xffffffffu) { ops_at = (uint32_t)P.ops.size(); P.ops.push_back(h.dops); }
                    store(ts, &h.dops, ops_at);
                } else {
                    store(ts, nullptr, 0);
                }
            }
        }
        // upsampled: the output, tile by tile (the tiles never reached included)
        const Rect uout = intersect(tile.r, {h.ix0, h.iy0, h.ix1, h.iy1});  // the tile's pixels of the output
        if (!h.up || uout.empty()) continue;
        UpPlan pl{};
        for (uint32_t k = 0; k < nc; ++k) {
            pl.c[k] = h.up_comp(lt, k, (const void *)(B.img0 + B.stoff[k]),
                                tile.comps.empty() ? nullptr : (const int32_t *)(B.work0 + tile.comps[k].arena_off * 4));
            if (h.staged(k) && h.conv) pl.c[k].raw = (uint8_t)(UPCOMP_FIN + h.sfmt);
        }
        const uint64_t delem = (uint64_t)(uout.y0 - h.iy0) * h.iw + (uout.x0 - h.ix0);
        DstPlanes tdst{};
        for (uint32_t k = 0; k < nout; ++k) tdst.p[k] = (void *)(B.dst(h, k) + delem * eb);
        plan_conv(P, h, ops_at, pl, uout, tdst, h.il ? h.iw * no : h.iw);
    }
    // Samples nothing decoded, where the colour step converts them
    // (decompress_impl's fill_converted): the converting store over null
    // sources -- on the margin of a reduced decode (the output beyond the
    // decoded rectangle cwin[0]) and on the tiles the stream never reached,
    // which no other job writes, so the order among the jobs is free.
    if (!h.converted_zeros()) return;
    // the rectangles nothing decoded on component g's grid
    auto zero_rects = [&](uint32_t g) {
        std::vector<Rect> zr;
        const Rect &o0 = h.orect[g], &cw = h.cwin[g];
        if (h.opad) {
            zr.push_back({std::max(cw.x1, o0.x0), o0.y0, o0.x1, o0.y1});
            zr.push_back({o0.x0, std::max(cw.y1, o0.y0), std::min(cw.x1, o0.x1), o0.y1});
        }
        for (uint32_t t = h.tb; h.missing && t < h.te; ++t) {
            if (h.walk.decoded[t] || h.wskip[t]) continue;
            const Rect cr = comp_rect(tile_rect(h.cp, t), h.cp.dx[g], h.cp.dy[g]);  // (one grid; sYCC: the image's)
            zr.push_back(intersect({ceil_pow2(cr.x0, h.reduce), ceil_pow2(cr.y0, h.reduce), ceil_pow2(cr.x1, h.reduce),
                                    ceil_pow2(cr.y1, h.reduce)}, o0));
        }
        return zr;
    };
    if (h.mixed) {
        // (a float destination only) each plane on its own grid: one-component jobs with the plane's own ops
        for (uint32_t k = 0; k < nc; ++k) {
            const Rect &ok_ = h.orect[k];
            const OutOps ok = plane_ops(h.dops, k);
            for (const Rect &o : zero_rects(k)) {
                if (o.empty()) continue;
                ConvJob j{};
                j.c[0].dx = j.c[0].dy = 1;
                j.dst[0] = (void *)(B.dst(h, k) + ((uint64_t)(o.y0 - ok_.y0) * ok_.w() + (o.x0 - ok_.x0)) * h.sb);
                j.X0 = o.x0; j.Y0 = o.y0; j.x1 = o.x1; j.y1 = o.y1;
                j.dstride = ok_.w(); j.ncomp = 1;
                if (kops_at[k] == 0xffffffffu) { kops_at[k] = (uint32_t)P.ops.size(); P.ops.push_back(ok); }
                if (P.add_up(h.od.fmt, false, ok, j, kops_at[k])) continue;
                UpPlan zero{};
                zero.c[0] = j.c[0];
                DstPlanes fdst{};
                fdst.p[0] = j.dst[0];
                P.up_singles.push_back(TileConv{zero, 1, o, fdst, h.od.fmt, false, j.dstride, ok, true});
            }
        }
        return;
    }
    const Rect &o0 = h.orect[0];
    for (const Rect &o : zero_rects(0)) {
        if (o.empty()) continue;
        UpPlan zero{};
        for (uint32_t k = 0; k < nc; ++k) zero.c[k].dx = zero.c[k].dy = 1;
        DstPlanes fdst{};
        for (uint32_t k = 0; k < nout; ++k)
            fdst.p[k] = (void *)(B.dst(h, k) + ((uint64_t)(o.y0 - o0.y0) * ow + (o.x0 - o0.x0)) * eb);
        plan_conv(P, h, ops_at, zero, o, fdst, h.il ? ow * no : ow);
    }
}

// What grkgpu_jp2_decompress_batch knows of item i beyond its bytes, filled by
// the entry point's `prep` on the host pool: the jp2c payload inside the file,
// the ops with GRKGPU_COLOUR_AUTO / _AUTO_RGB resolved (o; has_ops: the caller
// gave ops), the channel map of a file with a palette or a channel swap, and
// whether the file says sRGB.  chan and the table it points at live until the
// call returns.
struct Jp2Item {
    const uint8_t *cs = nullptr;
    size_t len = 0;
    grkgpu_out_ops o{};
    bool has_ops = false;
    const ChanMap *chan = nullptr;
    bool is_rgb = false;
};
using Jp2Prep = std::function<int(size_t, Jp2Item &)>;

// ops / convert: grkgpu_decompress_batch_convert (ops null: no item converts).
// jp2 (grkgpu_jp2_decompress_batch; implies convert): items[i].cs / len are a
// JP2 file, parsed by (*jp2)(i, ...); force-RGB is taken.
static int batch_impl(grkgpu_ctx *c, grkgpu_batch_item *items, uint32_t n, const grkgpu_dparams *p,
                      grkgpu_batch_info *info, bool host_only, bool convert = false,
                      const grkgpu_out_ops *ops = nullptr, const Jp2Prep *jp2 = nullptr, bool floats = false,
                      const grkgpu_out_norm *norms = nullptr) {
    if (info) *info = grkgpu_batch_info{};
    if ((!c && !host_only) || (n && !items)) return set_err(GRKGPU_EINVAL, "null argument");
    if (p && (p->DA_x0 || p->DA_y0 || p->DA_x1 || p->DA_y1))
        return set_err(GRKGPU_EINVAL, "a decode area is not supported in a batch");
    if (!n) return GRKGPU_OK;
    ActiveCall active;
    const double t_start = now_ms();
    const uint32_t reduce = p ? p->cp_reduce : 0, layers = p ? p->cp_layer : 0;
    std::vector<DecHost> H(n);
    std::vector<std::string> emsg(n);
    std::vector<Jp2Item> J(jp2 ? n : 0);
    // (called on the thread whose check failed: the message is thread-local)
    auto fail = [&](size_t i, int rc) { items[i].status = rc; emsg[i] = g_err; };
    host_parallel_for(n, 1, [&](size_t a, size_t b) {
        for (size_t i = a; i < b; ++i) {
            grkgpu_batch_item &it = items[i];
            it.status = GRKGPU_OK;
            it.img = grkgpu_image_desc{};
            DecHost &h = H[i];
            int rc = it.cs ? GRKGPU_OK : set_err(GRKGPU_EINVAL, "null argument");
            if (!rc && jp2) rc = (*jp2)(i, J[i]);  // (the boxes first, as grkgpu_jp2_decompress reads them)
            if (!rc) rc = check_out_planes(&it.out, floats);
            if (!rc && !convert && (it.out.layout & GRKGPU_LAYOUT_UPSAMPLE))
                rc = set_err(GRKGPU_EUNSUPPORTED, "upsampled output is not supported in a batch");
            const grkgpu_out_ops *const given = jp2 ? (J[i].has_ops ? &J[i].o : nullptr) : (convert && ops ? &ops[i] : nullptr);
            // (a float item always converts: its ops are never null)
            const grkgpu_out_ops *const o = out_ops_active(given) ? given : (floats ? &g_no_ops : nullptr);
            if (!rc && given) rc = check_out_ops(given, it.out.sample_fmt);
            if (!rc && !jp2 && o && (o->colour & GRKGPU_COLOUR_FORCE_RGB))
                rc = set_err(GRKGPU_EUNSUPPORTED, "force-RGB is not supported in a batch");
            if (!rc) {
                h.csb = jp2 ? J[i].cs : it.cs; h.len = jp2 ? J[i].len : it.len; h.img = &it.img;
                h.od = DecodeOut{it.out.planes, (int32_t)it.out.sample_fmt,
                                 (it.out.layout & ~GRKGPU_LAYOUT_UPSAMPLE) == GRKGPU_LAYOUT_INTERLEAVED,
                                 it.out.on_device, (it.out.layout & GRKGPU_LAYOUT_UPSAMPLE) != 0, o, 0,
                                 jp2 ? J[i].chan : nullptr, jp2 && J[i].is_rgb ? 1 : 0, floats ? 1 : 0,
                                 floats && norms ? &norms[i] : nullptr};
                h.reduce = reduce; h.max_layers = layers; h.host_only = host_only; h.batch = !convert;
                rc = h.begin();
            }
            if (rc) fail(i, rc);
        }
    });
    // packet headers over every (item, tile), then each item's tables
    std::vector<std::pair<uint32_t, uint32_t>> todo;
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t lt = 0; !items[i].status && lt < H[i].nsh; ++lt) todo.push_back({i, lt});
    host_parallel_for(todo.size(), 1, [&](size_t a, size_t b) {
        for (size_t q = a; q < b; ++q) H[todo[q].first].parse_tiles(todo[q].second, todo[q].second + 1);
    });
    host_parallel_for(n, 1, [&](size_t a, size_t b) {
        for (size_t i = a; i < b; ++i) {
            if (items[i].status) continue;
            const int rc = H[i].finish();
            if (rc) fail(i, rc);
        }
    });
    int first_rc = GRKGPU_OK;
    std::string first_msg;
    for (uint32_t i = 0; i < n && !first_rc; ++i)
        if (items[i].status) { first_rc = items[i].status; first_msg = "item " + std::to_string(i) + ": " + emsg[i]; }
    auto result = [&]() { return first_rc ? set_err(first_rc, first_msg) : GRKGPU_OK; };

    // the merged tables: item i's stream at cs_off[i], its arenas from abase[i] / llbase[i]
    std::vector<uint64_t> cs_off(n, 0), abase(n, 0), llbase(n, 0);
    uint64_t cs_total = 0, cs_sum = 0, arena = 0, llarena = 0, nblk64 = 0, nseg64 = 0;
    uint32_t n_ok = 0;
    bool any_roi = false;
    for (uint32_t i = 0; i < n; ++i) {
        if (items[i].status) continue;
        const DecHost &h = H[i];
        cs_off[i] = cs_total;
        cs_total = (cs_total + h.len + h.extra.size() + 15) & ~(uint64_t)15;
        abase[i] = arena;
        arena += h.arena;
        llbase[i] = llarena;
        llarena += h.llarena;
        nblk64 += h.db.size();
        nseg64 += h.dsegs.size();
        cs_sum += h.len;
        any_roi = any_roi || !h.droi.empty();
        ++n_ok;
    }
    // the items' palettes: one merged table of uint16 entries behind the
    // streams in the same pinned buffer and device buffer, so it reaches the
    // device in the streams' copy; each item's table (copies of one file
    // included) at an even entry
    std::vector<uint32_t> pal_off(n, 0);
    const uint64_t pal_base = cs_total;  // (a multiple of 16)
    uint64_t pal_entries = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const DecHost &h = H[i];
        if (items[i].status || !h.cm || !h.cm->table || !h.cm->ne) continue;
        pal_off[i] = (uint32_t)pal_entries;
        pal_entries = (pal_entries + (uint64_t)h.cm->ne * h.cm->npc + 1) & ~(uint64_t)1;
    }
    if (pal_entries > 0x7fffffffull) return set_err(GRKGPU_EUNSUPPORTED, "batch too large for one call");
    cs_total = (cs_total + pal_entries * 2 + 15) & ~(uint64_t)15;
    uint64_t uwords = 0;
    for (uint32_t i = 0; i < n; ++i)
        for (size_t q = 0; !items[i].status && q < H[i].dsegs.size(); ++q)
            uwords += t1_unstuff_region_words(H[i].dsegs[q].len);
    if (nblk64 > 0xffffffffull || nseg64 > 0xffffffffull || uwords / 4 > 0xffffffffull)
        return set_err(GRKGPU_EUNSUPPORTED, "batch too large for one call");
    const uint32_t nblk = (uint32_t)nblk64;
    std::vector<DecBlock> db;
    std::vector<DecSeg> dsegs;
    std::vector<uint8_t> droi, dsty;
    std::vector<uint32_t> seg_first;
    db.reserve(nblk);
    dsegs.reserve(nseg64);
    dsty.reserve(nblk);
    seg_first.reserve((size_t)nblk + 1);
    for (uint32_t i = 0; i < n; ++i) {
        if (items[i].status) continue;
        DecHost &h = H[i];
        const uint32_t s0 = (uint32_t)dsegs.size();
        for (DecBlock d : h.db) {
            d.dst_off += abase[i];
            d.data_off += cs_off[i];
            db.push_back(d);
        }
        for (DecSeg sg : h.dsegs) {
            sg.data_off += cs_off[i];
            dsegs.push_back(sg);
        }
        for (uint32_t f : h.seg_first) seg_first.push_back(s0 + f);
        dsty.insert(dsty.end(), h.dsty.begin(), h.dsty.end());
        if (any_roi) {
            if (h.droi.empty()) droi.insert(droi.end(), h.db.size(), 0);
            else droi.insert(droi.end(), h.droi.begin(), h.droi.end());
        }
        for (Tile &tile : h.tiles)
            for (TileComp &tc : tile.comps) tc.arena_off += abase[i];
        for (uint64_t &o : h.lloff) o += llbase[i];
    }
    seg_first.push_back((uint32_t)dsegs.size());

    // where the items' samples go on the device: their own planes, or the
    // staging image.  Host regions adjacent in the caller's memory are
    // adjacent there too and leave in one copy; every other region starts on
    // a 16-byte boundary (the store's packed writes).
    struct Region { uint8_t *host; size_t off, bytes; };
    std::vector<Region> regions;
    std::vector<std::array<size_t, GRKGPU_MAX_COMPS>> roff(n);
    size_t img_bytes = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const DecHost &h = H[i];
        if (items[i].status || h.planes_on_device || host_only) continue;
        for (uint32_t k = 0; k < h.nout(); ++k) {
            Region r{(uint8_t *)h.planes[k], 0, h.region_bytes(k)};
            const bool adj = !regions.empty() && regions.back().host + regions.back().bytes == r.host &&
                             (regions.back().off + regions.back().bytes) % h.sb == 0;
            r.off = adj ? regions.back().off + regions.back().bytes : (img_bytes + 15) & ~(size_t)15;
            img_bytes = r.off + r.bytes;
            roff[i][k] = r.off;
            regions.push_back(r);
        }
    }
    // the staging planes of the upsampled items' staged components, behind the
    // output staging, each on a 16-byte boundary
    std::vector<std::array<size_t, GRKGPU_MAX_COMPS>> stoff(n);
    // [zero0, zero1): the span from the first to the last staging plane of a
    // stream with tiles it never reached -- zeroed by one fill, the planes of
    // complete streams that lie between included (phase 1 writes every sample
    // of theirs afterwards), so that N copies take the fills of one
    size_t zero0 = 0, zero1 = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const DecHost &h = H[i];
        if (items[i].status || !h.up) continue;
        for (uint32_t k = 0; k < h.nc; ++k) {
            if (!h.staged(k)) continue;
            img_bytes = (img_bytes + 15) & ~(size_t)15;
            stoff[i][k] = img_bytes;
            img_bytes += h.stage_bytes(k);
            if (h.missing) {
                if (zero1 == 0) zero0 = stoff[i][k];
                zero1 = img_bytes;
            }
        }
    }
    if (!host_only) {
        HIPCHK(hipSetDevice(c->device));
        if (img_bytes) HIPCHK(c->img.ensure(img_bytes + 256));
        HIPCHK(c->work.ensure(arena * 4 + 256));
    }
    // the last store's records, item after item
    StorePlan stores;
    auto bases = [&](uint32_t i) {
        return ItemBases{host_only ? 0 : (uintptr_t)c->work.p, host_only ? 0 : (uintptr_t)c->img.p, roff[i].data(),
                         stoff[i].data(), host_only, pal_off[i]};
    };
    for (uint32_t i = 0; i < n; ++i)
        if (!items[i].status) plan_item_stores(stores, H[i], bases(i));
    if (info) {
        info->n_ok = n_ok;
        info->n_blocks = nblk;
        info->n_store_jobs = stores.njobs();
    }
    if (host_only || !n_ok) return result();

    hipStream_t s = c->stream;
    uint32_t nl = 0;  // kernel launches and fills of this call
    const int drc = [&]() -> int {
        DecT1Stage t1;
        int rc = t1.prepare(c, db, dsegs, seg_first, droi, dsty, "batch too large for one call");
        if (rc) return rc;
        HIPCHK(c->cs.ensure(cs_total + 256));
        HIPCHK(c->h_cs.ensure(cs_total + 256));
        HIPCHK(c->coef.ensure(arena * 4 + 256));
        HIPCHK(c->ll.ensure(llarena * 4 + 256));
        HIPCHK(c->storejobs.ensure(stores.bytes() + 256));
        HIPCHK(c->h_storejobs.ensure(stores.bytes() + 256));
        // the streams packed into the pinned buffer, on the host pool: the
        // bytes between them are never addressed by a segment
        host_parallel_for(n, 1, [&](size_t a, size_t b) {
            for (size_t i = a; i < b; ++i) {
                if (items[i].status) continue;
                uint8_t *d = c->h_cs.as<uint8_t>() + cs_off[i];
                memcpy(d, H[i].csb, H[i].len);
                if (!H[i].extra.empty()) memcpy(d + H[i].len, H[i].extra.data(), H[i].extra.size());
                if (const ChanMap *cm = H[i].cm; cm && cm->table && cm->ne)
                    memcpy(c->h_cs.as<uint8_t>() + pal_base + (size_t)pal_off[i] * 2, cm->table, (size_t)cm->ne * cm->npc * 2);
            }
        });
        stores.pal_table = (const uint16_t *)(c->cs.as<uint8_t>() + pal_base);

        HIPCHK(hipEventRecord(c->ev[0], s));
        HIPCHK(hipMemcpyAsync(c->cs.p, c->h_cs.p, cs_total, hipMemcpyHostToDevice, s));
        rc = t1.upload(c);
        if (rc) return rc;
        HIPCHK(stores.upload(c->h_storejobs.as<uint8_t>(), c->storejobs.p, s));
        DwtPlan dplan[2];  // one plan per wavelet over every item's tile-components
        for (uint32_t i = 0; i < n; ++i) {
            if (items[i].status) continue;
            const DecHost &h = H[i];
            for (uint32_t lt = 0; lt < h.nsh; ++lt)
                for (uint32_t k = 0; k < h.tiles[lt].comps.size(); ++k) {
                    const TileComp &tc = h.tiles[lt].comps[k];
                    dwt_plan_tc(dplan[tc.irrev], tc, c->work.as<int32_t>() + tc.arena_off,
                                c->coef.as<int32_t>() + tc.arena_off, c->ll.as<int32_t>() + h.lloff[lt * h.nc + k],
                                tc.irrev, true, tc.numres - reduce, nullptr);
                }
        }
        HIPCHK(dwt_upload_plans(c, dplan));
        HIPCHK(hipEventRecord(c->ev[1], s));
        rc = t1.launch(c, &nl);
        if (rc) return rc;
        HIPCHK(hipEventRecord(c->ev[2], s));
        HIPCHK(dwt_launch_plans(c, dplan, true, &nl));
        HIPCHK(hipEventRecord(c->ev[3], s));
        // tiles a stream never reached are zero in its staging planes; in the
        // output the upsampling store writes their pixels
        if (zero1 > zero0) {
            HIPCHK(hipMemsetAsync(c->img.as<uint8_t>() + zero0, 0, zero1 - zero0, s));
            ++nl;
        }
        for (uint32_t i = 0; i < n; ++i) {
            if (items[i].status) continue;
            const DecHost &h = H[i];
            if (h.converted_zeros()) continue;  // (ConvJobs over null sources)
            if (h.cm && (h.opad || h.missing)) continue;  // (zero PalJobs: entry 0 of the looked-up channels)
            void *dst[GRKGPU_MAX_COMPS];
            for (uint32_t k = 0; k < h.nout(); ++k) dst[k] = (void *)bases(i).dst(h, k);
            HIPCHK(dec_zero_fills(h, dst, s, &nl));
        }
        HIPCHK(stores.launch(c->storejobs.p, s, &nl));  // (phase 1, then phase 2)
        HIPCHK(hipEventRecord(c->ev[4], s));
        for (size_t r = 0; r < regions.size();) {  // one copy per run of adjacent regions
            size_t e = r + 1, bytes = regions[r].bytes;
            while (e < regions.size() && regions[e].off == regions[r].off + bytes &&
                   regions[e].host == regions[r].host + bytes)
                bytes += regions[e++].bytes;
            if (bytes)
                HIPCHK(hipMemcpyAsync(regions[r].host, c->img.as<uint8_t>() + regions[r].off, bytes,
                                      hipMemcpyDeviceToHost, s));
            r = e;
        }
        HIPCHK(hipEventRecord(c->ev[5], s));
        HIPCHK(hipStreamSynchronize(s));
        fill_dec_stats(c, t_start, t1.t_tables, now_ms(), nblk, cs_sum);
        return GRKGPU_OK;
    }();
    if (drc) {  // a device error leaves no item decoded
        const std::string msg = g_err;
        for (uint32_t i = 0; i < n; ++i)
            if (!items[i].status) items[i].status = drc;
        if (info) info->n_ok = 0;
        return set_err(drc, msg);
    }
    if (info) info->n_launches = nl;
    return result();
}

extern "C" int grkgpu_decompress_batch(grkgpu_ctx *c, grkgpu_batch_item *items, uint32_t n, const grkgpu_dparams *p,
                                       grkgpu_batch_info *info) {
    return batch_impl(c, items, n, p, info, false);
}

extern "C" int grkgpu_batch_plan(grkgpu_batch_item *items, uint32_t n, const grkgpu_dparams *p,
                                 grkgpu_batch_info *info) {
    return batch_impl(nullptr, items, n, p, info, true);
}

extern "C" int grkgpu_decompress_batch_convert(grkgpu_ctx *c, grkgpu_batch_item *items, const grkgpu_out_ops *ops,
                                               uint32_t n, const grkgpu_dparams *p, grkgpu_batch_info *info) {
    return batch_impl(c, items, n, p, info, false, true, ops);
}

extern "C" int grkgpu_batch_convert_plan(grkgpu_batch_item *items, const grkgpu_out_ops *ops, uint32_t n,
                                         const grkgpu_dparams *p, grkgpu_batch_info *info) {
    return batch_impl(nullptr, items, n, p, info, true, true, ops);
}

extern "C" int grkgpu_decompress_batch_float(grkgpu_ctx *c, grkgpu_batch_item *items, const grkgpu_out_ops *ops,
                                             const grkgpu_out_norm *norms, uint32_t n, const grkgpu_dparams *p,
                                             grkgpu_batch_info *info) {
    return batch_impl(c, items, n, p, info, false, true, ops, nullptr, true, norms);
}

extern "C" int grkgpu_batch_float_plan(grkgpu_batch_item *items, const grkgpu_out_ops *ops,
                                       const grkgpu_out_norm *norms, uint32_t n, const grkgpu_dparams *p,
                                       grkgpu_batch_info *info) {
    return batch_impl(nullptr, items, n, p, info, true, true, ops, nullptr, true, norms);
}

// ---------------------------------------------------------------------------
// Batch encode (grkgpu_compress_batch): the host half of compress_impl
// (EncHost) per item on the host pool; the items' tables rebased into one
// EncBlock / symoff table, one MQ slab, one coef / work / ll arena and one
// DwtPlan per wavelet -- then the device half once: one H2D of the host
// samples (staged into h_img, each plane on a 16-byte boundary), the DC shift
// + MCT from a LoadJob table, one launch per (sample format, mode) present,
// the forward DWT, one Tier-1 launch set per code-block style, the pass
// records and Tier-2 per item over (item, tile) pairs on the host pool, one
// gather and one D2H.
//
// Merged block order: style groups in order of first appearance; inside a
// group the items with rate control first, then the others, each in call
// order, so k_pass_records runs over a contiguous prefix of the group.
// k_t1_dist runs over the whole group when that prefix is not empty (the
// coders' scratch layout is the group's, t1_lane.h enc_scratch); the sums it
// leaves for blocks without rate control are not read.
// ---------------------------------------------------------------------------
static_assert(sizeof(grkgpu_load_job) == sizeof(LoadJob) && offsetof(grkgpu_load_job, dst) == offsetof(LoadJob, dst) &&
                  offsetof(grkgpu_load_job, src_stride) == offsetof(LoadJob, sstride) &&
                  offsetof(grkgpu_load_job, numcomps) == offsetof(LoadJob, ncomp) &&
                  offsetof(grkgpu_load_job, irreversible) == offsetof(LoadJob, irrev) &&
                  offsetof(grkgpu_load_job, shift) == offsetof(LoadJob, shift),
              "grkgpu_load_job is LoadJob");
static_assert(sizeof(DevPass) == sizeof(EncPass), "DevPass is EncPass");

// a tile the job table does not take (more than four components, or too many
// workgroups for one job): launch_dcshift_mct_fwd's arguments
struct TileLoad {
    SrcPlanes src;
    PlanePtrs dst;
    uint32_t sstride, w, h, dstride, nc;
    int32_t lfmt, mct, irrev;
    ShiftArr sh;
};
// a tile as a record (nc <= 4) and back
static LoadJob load_job_of(const TileLoad &tl) {
    LoadJob j{};
    for (uint32_t k = 0; k < 4; ++k) {
        j.src[k] = tl.src.p[k];
        j.dst[k] = tl.dst.p[k];
        j.shift[k] = tl.sh.v[k];
    }
    j.sstride = tl.sstride; j.dstride = tl.dstride; j.w = tl.w; j.h = tl.h;
    j.ncomp = tl.nc; j.mct = tl.mct; j.irrev = tl.irrev;
    return j;
}
static TileLoad tile_load_of(const LoadJob &j, int32_t lfmt) {
    TileLoad tl{};
    for (uint32_t k = 0; k < ((lfmt & SMP_INTERLEAVED) ? 1u : j.ncomp); ++k) tl.src.p[k] = j.src[k];
    for (uint32_t k = 0; k < j.ncomp; ++k) {
        tl.dst.p[k] = j.dst[k];
        tl.sh.v[k] = j.shift[k];
    }
    tl.sstride = j.sstride; tl.w = j.w; tl.h = j.h; tl.dstride = j.dstride; tl.nc = j.ncomp;
    tl.lfmt = lfmt; tl.mct = j.mct; tl.irrev = j.irrev;
    return tl;
}
// The DC shift + MCT of a launch set (grkgpu_compress_batch and its stage
// call): the LoadJob table, one group per (sample format, mode: bit 0
// big-endian, bit 1 interleaved), alone in its buffer, and the per-tile launches.
struct LoadPlan {
    JobTable<LoadJob> table;
    std::vector<TileLoad> singles;
    bool add(int32_t lfmt, const LoadJob &j) {
        const int mode = ((lfmt & SMP_BIG_ENDIAN) ? 1 : 0) | ((lfmt & SMP_INTERLEAVED) ? 2 : 0);
        return table.add({lfmt & 0xff, mode, 0}, j, load_job_wgs(j, (mode & 2) != 0));
    }
    hipError_t upload(uint8_t *stage, void *dev, hipStream_t s) const {
        return upload_tables(stage, dev, table.fill(stage, 0, table.rec_bytes()), table.bytes(), s);
    }
    hipError_t launch(const void *dev, hipStream_t s, uint32_t *nl) const {
        hipError_t e = table.launch(dev, 0, table.rec_bytes(), nl,
                                    [&](const LoadJob *j, const uint32_t *first, uint32_t n, uint32_t nwg, const JobKey &k) {
                                        return launch_load_jobs(j, first, n, nwg, k.fmt, k.mode, s);
                                    });
        for (size_t i = 0; e == hipSuccess && i < singles.size(); ++i) {
            const TileLoad &t = singles[i];
            e = t.dstride == t.w
                    ? launch_dcshift_mct_fwd(t.src, t.lfmt, t.sstride, t.dst, t.w, t.h, t.nc, t.sh, t.mct, t.irrev, s)
                    : launch_dcshift_mct_fwd_from(t.src, t.lfmt, t.sstride, t.dst, t.dstride, t.w, t.h, t.nc, t.sh, t.mct,
                                                  t.irrev, s);
            if (e == hipSuccess && nl) ++*nl;
        }
        return e;
    }
};

static int cbatch_impl(grkgpu_ctx *c, grkgpu_cbatch_item *items, uint32_t n, grkgpu_cbatch_info *info, bool host_only) {
    if (info) *info = grkgpu_cbatch_info{};
    if ((!c && !host_only) || (n && !items)) return set_err(GRKGPU_EINVAL, "null argument");
    if (!n) return GRKGPU_OK;
    ActiveCall active;
    const double t_start = now_ms();
    grkgpu_cparams defp;
    grkgpu_default_cparams(&defp);
    std::vector<EncHost> H(n);
    std::vector<std::string> emsg(n);
    // (called on the thread whose check failed: the message is thread-local)
    auto fail = [&](size_t i, int rc) {
        items[i].status = rc;
        items[i].cs = nullptr;
        items[i].len = 0;
        emsg[i] = g_err;
    };
    host_parallel_for(n, 1, [&](size_t a, size_t b) {
        for (size_t i = a; i < b; ++i) {
            grkgpu_cbatch_item &it = items[i];
            it.status = GRKGPU_OK;
            it.cs = nullptr;
            it.len = 0;
            EncHost &h = H[i];
            h.img = &it.img; h.p = it.p ? it.p : &defp; h.fmt_in = (int32_t)it.in.sample_fmt;
            h.row0 = it.in.row0; h.nrows = it.in.nrows; h.col0 = it.in.col0; h.ncols = it.in.ncols;
            h.batch = true;
            int rc = h.begin();
            for (uint32_t k = 0; !rc && !host_only && k < (h.il ? 1u : h.nc); ++k)
                if (!it.in.planes[k]) rc = set_err(GRKGPU_EINVAL, "null argument");
            if (rc) fail(i, rc);
        }
    });
    int first_rc = GRKGPU_OK;
    std::string first_msg;
    auto result = [&]() {
        for (uint32_t i = 0; i < n && !first_rc; ++i)
            if (items[i].status) { first_rc = items[i].status; first_msg = "item " + std::to_string(i) + ": " + emsg[i]; }
        return first_rc ? set_err(first_rc, first_msg) : GRKGPU_OK;
    };

    // the merged order (style groups; rate-controlled items first in each)
    // and the items' places in the merged tables (EncHost::mb0 / rcb0 / slot0)
    std::vector<StyGroup> sg;
    for (uint32_t i = 0; i < n; ++i) {
        if (items[i].status) continue;
        size_t g = 0;
        while (g < sg.size() && sg[g].sty != H[i].cp.cblksty) ++g;
        if (g == sg.size()) { sg.emplace_back(); sg[g].sty = H[i].cp.cblksty; }
        sg[g].items.push_back(i);
    }
    std::vector<uint32_t> order;
    uint64_t arena = 0, llarena = 0, out_total = 0, sym_total = 0, nblk64 = 0, nrc64 = 0, slots = 0, slots_all = 0,
             runs_bound = 0, scr_bytes = 0, ord_words = 0;
    for (StyGroup &g : sg) {
        std::stable_partition(g.items.begin(), g.items.end(), [&](uint32_t i) { return H[i].need_rc; });
        g.b0 = (uint32_t)std::min<uint64_t>(nblk64, 0xffffffffu);
        g.rc0 = (uint32_t)std::min<uint64_t>(nrc64, 0xffffffffu);
        for (uint32_t i : g.items) {
            EncHost &h = H[i];
            h.rebase(arena, llarena, out_total, sym_total);
            h.mb0 = nblk64;
            arena += h.arena;
            llarena += h.llarena;
            out_total += h.out_total;
            sym_total += h.sym_total;
            nblk64 += h.nblk;
            slots_all += h.ptotal;
            runs_bound += (uint64_t)h.nblk * h.cp.numlayers;
            g.maxdepth = std::max(g.maxdepth, h.maxdepth);
            if (h.need_rc) {
                h.rcb0 = nrc64;
                h.slot0 = slots;
                nrc64 += h.nblk;
                slots += h.ptotal;
            }
            order.push_back(i);
        }
        g.n = (uint32_t)std::min<uint64_t>(nblk64 - g.b0, 0xffffffffu);
        g.nrc = (uint32_t)std::min<uint64_t>(nrc64 - g.rc0, 0xffffffffu);
        g.scr0 = scr_bytes;
        scr_bytes += t1e_scratch_bytes(g.n, g.maxdepth);
        g.ord0 = ord_words;
        ord_words += t1_order_words(g.n);
    }
    // the 32-bit limits compress_impl relies on: the block count, the
    // pass-record slots (EncCblkState::pass0) and the gather runs (at least a
    // run per block and layer; the exact count is checked again before the launch)
    if (nblk64 > 0xffffffffull || slots_all > 0xffffffffull || runs_bound > 0x7fffffffull)
        return set_err(GRKGPU_EUNSUPPORTED, "batch too large for one call");
    const uint32_t nblk = (uint32_t)nblk64, nrc = (uint32_t)nrc64, n_ok = (uint32_t)order.size();

    // host samples: each plane (interleaved: the pixels) at a 16-byte-aligned
    // offset of the staging image
    struct Region { const uint8_t *host; size_t off, bytes; };
    std::vector<Region> regions;
    std::vector<std::array<size_t, GRKGPU_MAX_COMPS>> roff(n);
    size_t img_bytes = 0;
    for (uint32_t i : order) {
        const EncHost &h = H[i];
        if (items[i].in.on_device || host_only) continue;
        for (uint32_t k = 0; k < (h.il ? 1u : h.nc); ++k) {
            Region r{(const uint8_t *)items[i].in.planes[k], (img_bytes + 15) & ~(size_t)15,
                     (size_t)(h.il ? h.poff[h.nc] : h.poff[k + 1] - h.poff[k]) * h.sb};
            img_bytes = r.off + r.bytes;
            roff[i][k] = r.off;
            regions.push_back(r);
        }
    }
    if (!host_only) {
        HIPCHK(hipSetDevice(c->device));
        if (img_bytes) {
            HIPCHK(c->img.ensure(img_bytes + 256));
            HIPCHK(c->h_img.ensure(img_bytes + 256));
        }
        HIPCHK(c->work.ensure(arena * 4 + 256));
    }
    // the DC shift + MCT: a LoadJob per tile of every item of up to four
    // components, per-tile launches for the others
    LoadPlan loads;
    const uintptr_t work0 = host_only ? 0 : (uintptr_t)c->work.p, img0 = host_only ? 0 : (uintptr_t)c->img.p;
    for (uint32_t i : order) {
        const EncHost &h = H[i];
        const uint32_t nc = h.nc;
        auto src_at = [&](uint32_t k, uint64_t off) {  // sample `off` of component k's plane (compress_impl's src_at)
            const uintptr_t p0 = items[i].in.on_device ? (uintptr_t)items[i].in.planes[h.il ? 0 : k]
                                                       : img0 + roff[i][h.il ? 0 : k];
            return (const void *)(h.il ? p0 + (off * nc + k) * h.sb : p0 + off * h.sb);
        };
        for (const Tile &tile : h.tiles) {
            const Rect &tcr = tile.comps[0].r;
            TileLoad tl{};
            for (uint32_t k = 0; k < nc; ++k) {
                tl.src.p[k] = src_at(k, h.plane_org(k, tile.comps[k]));
                tl.dst.p[k] = (int32_t *)(work0 + tile.comps[k].arena_off * 4);
                tl.sh.v[k] = h.cp.shift[k];
            }
            tl.sstride = h.prect[0].w() * (h.il ? nc : 1);  // interleaved: src.p[0] = the tile's first pixel
            tl.w = tcr.w(); tl.h = tcr.h(); tl.dstride = tcr.w(); tl.nc = nc;
            tl.lfmt = h.lfmt; tl.mct = h.cp.mct; tl.irrev = h.cp.irrev;
            if (nc > 4 || !loads.add(h.lfmt, load_job_of(tl))) loads.singles.push_back(tl);
        }
    }
    if (info) {
        info->n_ok = n_ok;
        info->n_blocks = nblk;
        info->n_load_jobs = loads.table.njobs;
    }
    if (host_only || !n_ok) return result();

    hipStream_t s = c->stream;
    uint32_t nl = 0;  // kernel launches and fills of this call
    const int drc = [&]() -> int {
        int rc = enc_ensure(c, arena, llarena, scr_bytes, ord_words, out_total, sym_total, nblk);
        if (rc) return rc;
        HIPCHK(c->loadjobs.ensure(loads.table.bytes() + 256));
        HIPCHK(c->h_loadjobs.ensure(loads.table.bytes() + 256));
        // the samples packed into the pinned buffer, on the host pool: the pad
        // bytes between planes are uploaded as they are and never addressed
        host_parallel_for(regions.size(), 1, [&](size_t a, size_t b) {
            for (size_t r = a; r < b; ++r) memcpy(c->h_img.as<uint8_t>() + regions[r].off, regions[r].host, regions[r].bytes);
        });
        // the merged block table and symbol-stream offsets
        {
            EncBlock *hb = c->h_blocks.as<EncBlock>();
            uint64_t *hs = c->h_symoff.as<uint64_t>();
            for (uint32_t i : order) {
                const EncHost &h = H[i];
                if (h.nblk) memcpy(hb + h.mb0, h.eb.data(), (size_t)h.nblk * sizeof(EncBlock));
                if (h.nblk) memcpy(hs + h.mb0, h.symoff.data(), (size_t)h.nblk * 8);
            }
            hs[nblk] = sym_total;
        }
        HIPCHK(hipEventRecord(c->ev[0], s));
        if (img_bytes) HIPCHK(hipMemcpyAsync(c->img.p, c->h_img.p, img_bytes, hipMemcpyHostToDevice, s));
        HIPCHK(loads.upload(c->h_loadjobs.as<uint8_t>(), c->loadjobs.p, s));
        HIPCHK(hipEventRecord(c->ev[1], s));
        HIPCHK(loads.launch(c->loadjobs.p, s, &nl));
        HIPCHK(hipEventRecord(c->ev[2], s));
        DwtPlan dplan[2];  // one plan per wavelet over every item's tile-components (never fused with the load)
        for (uint32_t i : order) {
            const EncHost &h = H[i];
            for (uint32_t t = 0; t < h.ntiles; ++t)
                for (uint32_t k = 0; k < h.nc; ++k) {
                    const TileComp &tc = h.tiles[t].comps[k];
                    dwt_plan_tc(dplan[h.cp.irrev ? 1 : 0], tc, c->work.as<int32_t>() + tc.arena_off,
                                c->coef.as<int32_t>() + tc.arena_off, c->ll.as<int32_t>() + h.lloff[t * h.nc + k],
                                h.cp.irrev, false);
                }
        }
        HIPCHK(dwt_upload_plans(c, dplan));
        HIPCHK(dwt_launch_plans(c, dplan, false, &nl));
        HIPCHK(hipEventRecord(c->ev[3], s));
        rc = enc_t1_stage(c, sg, H.data(), nblk, nrc, slots, &nl);
        if (rc) return rc;

        // pass records per item, then rate allocation and packets over
        // (item, tile) pairs, all on the host pool
        const double t_t2 = now_ms();
        const EncResult *res = c->h_results.as<EncResult>();
        const PassSum *sm = c->h_psum.as<PassSum>();
        const uint64_t *hp0 = (const uint64_t *)(c->h_pinfo.as<double>() + nrc);
        std::vector<uint32_t> gidx(n, 0);  // the item's style group
        for (size_t gi = 0; gi < sg.size(); ++gi)
            for (uint32_t i : sg[gi].items) gidx[i] = (uint32_t)gi;
        std::vector<uint64_t> hpass0(n, 0);  // first host-formed record of the items without rate control
        host_parallel_for(order.size(), 1, [&](size_t a, size_t b) {
            for (size_t q = a; q < b; ++q) {
                const uint32_t i = order[q];
                EncHost &h = H[i];
                const int rc = h.need_rc ? h.records_dev(sm + h.rcb0, hp0 + h.rcb0 + gidx[i],
                                                         c->h_precs.as<EncPass>() + h.slot0)
                                         : h.records_host_count(res + h.mb0);
                if (rc) fail(i, rc);
            }
        });
        uint64_t hpasses = 0;
        for (uint32_t i : order) {
            if (items[i].status || H[i].need_rc) continue;
            hpass0[i] = hpasses;
            hpasses += H[i].npass;
        }
        if (c->enc_passes.size() < hpasses) c->enc_passes.resize(hpasses);
        host_parallel_for(order.size(), 1, [&](size_t a, size_t b) {
            for (size_t q = a; q < b; ++q) {
                const uint32_t i = order[q];
                if (items[i].status) continue;
                EncHost &h = H[i];
                if (!h.need_rc) h.records_host_fill(res + h.mb0, c->enc_passes.data() + hpass0[i]);
                const int rc = h.finish_begin();
                if (rc) fail(i, rc);
            }
        });
        const double t_passrec = now_ms() - t_t2;
        std::vector<std::pair<uint32_t, uint32_t>> todo;
        for (uint32_t i : order)
            for (uint32_t t = 0; !items[i].status && t < H[i].ntiles; ++t) todo.push_back({i, t});
        host_parallel_for(todo.size(), 1, [&](size_t a, size_t b) {
            for (size_t q = a; q < b; ++q) H[todo[q].first].finish_tile(todo[q].second);
        });
        // the items' header blobs and plans in call order: header runs rebased
        // onto the shared blob, each stream's bytes from a 16-byte boundary
        ByteBuf hdr;
        std::vector<GatherItem> gi;
        std::vector<uint64_t> cs_off(n, 0), cs_len(n, 0);
        uint64_t total = 0, nsym = 0, cs_sum = 0;
        double t_rate = 0, t_packets = 0;
        RateStats rsum;
        uint32_t n_done = 0;
        for (uint32_t i = 0; i < n; ++i) {
            if (items[i].status) continue;
            EncHost &h = H[i];
            const int rc = h.finish_end();
            if (rc) { fail(i, rc); continue; }
            const uint64_t base = hdr.size();
            hdr.putn(h.hdr.v.data(), h.hdr.size());
            total = (total + 15) & ~(uint64_t)15;
            cs_off[i] = total;
            gather_append(gi, h.plan, base, total);
            cs_len[i] = total - cs_off[i];
            cs_sum += cs_len[i];
            nsym += h.nsym;
            t_rate += h.t_rate;
            t_packets += h.t_packets;
            rsum.probes += h.rsum.probes;
            rsum.skipped += h.rsum.skipped;
            rsum.evals += h.rsum.evals;
            rsum.sims += h.rsum.sims;
            rsum.form_ms += h.rsum.form_ms;
            rsum.sim_ms += h.rsum.sim_ms;
            ++n_done;
        }
        if (gi.size() > 0x7fffffffull) return set_err(GRKGPU_EUNSUPPORTED, "batch too large for one call");
        const double t_t2_end = now_ms();
        std::unique_lock<std::mutex> out_lk(c->out_mu, std::defer_lock);
        rc = enc_output_stage(c, gi, hdr, total, out_lk, &nl);
        if (rc) return rc;
        const double t_end = now_ms();
        for (uint32_t i = 0; i < n; ++i) {
            if (items[i].status) continue;
            items[i].cs = c->h_out.as<uint8_t>() + cs_off[i];
            items[i].len = (size_t)cs_len[i];
        }
        if (info) info->n_ok = n_done;

        const EncStatsTail tail{t_t2, t_t2_end, t_passrec, t_rate, t_packets, cs_sum, rsum};
        fill_enc_stats(c, t_start, t_end, nblk, nsym, &tail);
        return GRKGPU_OK;
    }();
    if (drc) {  // a device error leaves no item encoded
        const std::string msg = g_err;
        for (uint32_t i = 0; i < n; ++i)
            if (!items[i].status) { items[i].status = drc; items[i].cs = nullptr; items[i].len = 0; }
        if (info) info->n_ok = 0;
        return set_err(drc, msg);
    }
    if (info) info->n_launches = nl;
    return result();
}

extern "C" int grkgpu_compress_batch(grkgpu_ctx *c, grkgpu_cbatch_item *items, uint32_t n, grkgpu_cbatch_info *info) {
    return cbatch_impl(c, items, n, info, false);
}

extern "C" int grkgpu_compress_batch_plan(grkgpu_cbatch_item *items, uint32_t n, grkgpu_cbatch_info *info) {
    return cbatch_impl(nullptr, items, n, info, true);
}

// ---------------------------------------------------------------------------
// JP2 files: the box layer (jp2.cpp) around the entry points above
// ---------------------------------------------------------------------------
namespace {
struct Jp2Parsed {
    Jp2Boxes boxes;
    Jp2Channels ch;
    CodingParams cp;
    std::vector<uint16_t> table;  // the applied palette, ne x npc
};
}  // namespace

// boxes, the codestream's main header and the channel list; info / img (either may be null) filled
static int jp2_parse(const uint8_t *file, size_t len, Jp2Parsed &j, grkgpu_jp2_info *info, grkgpu_image_desc *img) {
    if (!file) return set_err(GRKGPU_EINVAL, "null argument");
    std::string err;
    Jp2Status st = jp2_read_boxes(file, len, j.boxes, err);
    if (st) return set_err(st == JP2_CORRUPT ? GRKGPU_ECORRUPT : GRKGPU_EUNSUPPORTED, err);
    Jp2Boxes &b = j.boxes;
    size_t sot = 0;
    if (!parse_main_header(file + b.cs_off, (size_t)b.cs_len, j.cp, sot, err)) return set_err(GRKGPU_EUNSUPPORTED, err);
    const CodingParams &cp = j.cp;
    st = jp2_resolve_channels(b, cp.numcomps, cp.prec, cp.sgnd, cp.dx, cp.dy, GRKGPU_MAX_COMPS, j.ch, err);
    if (st) return set_err(st == JP2_CORRUPT ? GRKGPU_ECORRUPT : GRKGPU_EUNSUPPORTED, err);
    if (b.have_cdef && b.cdef.size() > GRKGPU_JP2_MAX_CDEF)
        return set_err(GRKGPU_EUNSUPPORTED, "JP2: more channel definitions than this decoder keeps");
    if (j.ch.mapped)
        for (uint32_t k = 0; k < cp.numcomps; ++k)
            if (cp.dx[k] != 1 || cp.dy[k] != 1)
                return set_err(GRKGPU_EUNSUPPORTED, "JP2: palette / channel swap on an image with subsampled components");
    if (j.ch.palette) {
        j.table.resize(b.entries.size());
        for (size_t i = 0; i < b.entries.size(); ++i) j.table[i] = (uint16_t)b.entries[i];  // (columns of <= 16 bits)
    }
    const uint32_t nch = (uint32_t)j.ch.ch.size();
    if (info) {
        memset(info, 0, sizeof(*info));
        info->cs_offset = b.cs_off;
        info->cs_length = b.cs_len;
        info->ihdr_w = b.w; info->ihdr_h = b.h; info->ihdr_nc = b.numcomps; info->ihdr_bpc = b.bpc;
        if (b.have_colr) { info->meth = b.meth; info->enumcs = b.meth == 1 ? b.enumcs : 0; }
        info->colour_space = j.ch.colour_space;
        info->icc_offset = b.icc_off;
        info->icc_length = b.icc_len;
        info->cielab_words = b.ncielab;
        for (uint32_t i = 0; i < b.ncielab; ++i) info->cielab[i] = b.cielab[i];
        if (j.ch.palette) {
            info->pal_entries = b.ne;
            info->pal_columns = b.npc;
            for (uint32_t i = 0; i < b.npc; ++i) {
                info->pal_prec[i] = b.pal_size[i];
                info->pal_sgnd[i] = b.pal_sign[i];
                info->cmap_cmp[i] = b.cmap[i].cmp;
                info->cmap_mtyp[i] = b.cmap[i].mtyp;
                info->cmap_pcol[i] = b.cmap[i].pcol;
            }
        }
        info->cdef_n = b.have_cdef ? (uint32_t)b.cdef.size() : 0;
        for (uint32_t i = 0; i < info->cdef_n; ++i) {
            info->cdef_cn[i] = b.cdef[i].cn;
            info->cdef_typ[i] = b.cdef[i].typ;
            info->cdef_asoc[i] = b.cdef[i].asoc;
        }
        info->numchannels = nch;
        for (uint32_t i = 0; i < nch; ++i) {
            const Jp2Channel &ch = j.ch.ch[i];
            info->chan_prec[i] = ch.prec;
            info->chan_sgnd[i] = ch.sgnd;
            info->chan_alpha[i] = ch.alpha;
            info->chan_comp[i] = ch.comp;
            info->chan_pcol[i] = ch.pcol;
        }
        info->mapped = j.ch.mapped ? 1 : 0;
    }
    if (img) {
        image_desc_of(cp, img);
        img->numcomps = nch;
        for (uint32_t i = 0; i < nch; ++i) {
            const Jp2Channel &ch = j.ch.ch[i];
            img->prec[i] = ch.prec;
            img->sgnd[i] = ch.sgnd;
            img->dx[i] = ch.dx;
            img->dy[i] = ch.dy;
        }
    }
    return GRKGPU_OK;
}

extern "C" int grkgpu_jp2_read_info(const uint8_t *file, size_t len, grkgpu_jp2_info *info, grkgpu_image_desc *img) {
    if (!file || !info) return set_err(GRKGPU_EINVAL, "null argument");
    Jp2Parsed j;
    return jp2_parse(file, len, j, info, img);
}

extern "C" int grkgpu_jp2_read_palette(const uint8_t *file, size_t len, uint16_t *entries, uint32_t cap, uint32_t *n) {
    if (!file || !n) return set_err(GRKGPU_EINVAL, "null argument");
    Jp2Parsed j;
    int rc = jp2_parse(file, len, j, nullptr, nullptr);
    if (rc) return rc;
    *n = (uint32_t)j.table.size();
    if (*n && (!entries || cap < *n)) return set_err(GRKGPU_EINVAL, "palette buffer too small");
    for (uint32_t i = 0; i < *n; ++i) entries[i] = j.table[i];
    return GRKGPU_OK;
}

// What a decode of the parsed file j hands the codec, for grkgpu_jp2_decompress
// and every item of grkgpu_jp2_decompress_batch: the caller's ops with
// GRKGPU_COLOUR_AUTO / _AUTO_RGB resolved by the file's colour space (o; ops
// null: untouched), the refusal of force-RGB on a file with a profile, and the
// channel map of a file with a palette or a channel swap (mapped; cm.table
// points into j).
static int jp2_resolve(const Jp2Parsed &j, const grkgpu_out_ops *ops, grkgpu_out_ops &o, ChanMap &cm, bool &mapped) {
    o = grkgpu_out_ops{};
    if (ops) {
        o = *ops;
        const uint32_t force = o.colour & GRKGPU_COLOUR_FORCE_RGB, col = o.colour & ~GRKGPU_COLOUR_FORCE_RGB;
        const uint32_t space = j.ch.colour_space;
        if (col == GRKGPU_COLOUR_AUTO)
            o.colour = force | (space == JP2_CS_SYCC ? GRKGPU_COLOUR_SYCC : GRKGPU_COLOUR_NONE);
        else if (col == GRKGPU_COLOUR_AUTO_RGB)
            o.colour = force | (space == JP2_CS_SYCC   ? GRKGPU_COLOUR_SYCC
                                : space == JP2_CS_EYCC ? GRKGPU_COLOUR_EYCC
                                : space == JP2_CS_CMYK ? GRKGPU_COLOUR_CMYK
                                                       : GRKGPU_COLOUR_NONE);
        // grk_decompress --force-rgb on a file with a profile goes through its colour management library
        if (force && (j.boxes.icc_len || space == JP2_CS_ICC))
            return set_err(GRKGPU_EUNSUPPORTED, "JP2: force-RGB on a file with an ICC profile");
    }
    mapped = j.ch.mapped;
    cm = ChanMap{};
    if (!mapped) return GRKGPU_OK;
    cm.nch = (uint32_t)j.ch.ch.size();
    for (uint32_t i = 0; i < cm.nch; ++i) {
        cm.comp[i] = j.ch.ch[i].comp;
        cm.pcol[i] = j.ch.ch[i].pcol;
        cm.prec[i] = j.ch.ch[i].prec;
        cm.sgnd[i] = j.ch.ch[i].sgnd;
    }
    if (j.ch.palette) {
        cm.ne = j.boxes.ne;
        cm.npc = j.boxes.npc;
        cm.table = j.table.data();
    }
    return GRKGPU_OK;
}

extern "C" int grkgpu_jp2_decompress(grkgpu_ctx *c, const uint8_t *file, size_t len, const grkgpu_dparams *dp,
                                     uint32_t tile_begin, uint32_t tile_end, grkgpu_image_desc *img,
                                     const grkgpu_out_planes *out, const grkgpu_out_ops *ops, grkgpu_jp2_info *info) {
    if (!c || !file || !out) return set_err(GRKGPU_EINVAL, "null argument");
    Jp2Parsed j;
    int rc = jp2_parse(file, len, j, info, nullptr);
    if (rc) return rc;
    grkgpu_out_ops o{};
    ChanMap cm{};
    bool mapped = false;
    rc = jp2_resolve(j, ops, o, cm, mapped);
    if (rc) return rc;
    return decompress_to_impl(c, file + j.boxes.cs_off, (size_t)j.boxes.cs_len, dp, tile_begin, tile_end, img, out,
                              ops ? &o : nullptr, false, mapped ? &cm : nullptr, j.ch.colour_space == JP2_CS_SRGB);
}

// grkgpu_jp2_decompress_batch / grkgpu_jp2_batch_plan: batch_impl with the box
// layer per item (parsed on the host pool, each item's Jp2Parsed and ChanMap
// its own and alive until the call returns)
static int jp2_batch(grkgpu_ctx *c, grkgpu_batch_item *items, const grkgpu_out_ops *ops, uint32_t n,
                     const grkgpu_dparams *p, grkgpu_batch_info *info, grkgpu_jp2_info *infos, bool host_only) {
    std::vector<Jp2Parsed> parsed(items ? n : 0);
    std::vector<ChanMap> maps(items ? n : 0);
    const Jp2Prep prep = [&](size_t i, Jp2Item &it) -> int {
        if (infos) memset(&infos[i], 0, sizeof(infos[i]));
        Jp2Parsed &j = parsed[i];
        int rc = jp2_parse(items[i].cs, items[i].len, j, infos ? &infos[i] : nullptr, nullptr);
        if (rc) return rc;
        bool mapped = false;
        rc = jp2_resolve(j, ops ? &ops[i] : nullptr, it.o, maps[i], mapped);
        if (rc) return rc;
        it.cs = items[i].cs + j.boxes.cs_off;
        it.len = (size_t)j.boxes.cs_len;
        it.has_ops = ops != nullptr;
        it.chan = mapped ? &maps[i] : nullptr;
        it.is_rgb = j.ch.colour_space == JP2_CS_SRGB;
        return GRKGPU_OK;
    };
    return batch_impl(c, items, n, p, info, host_only, true, nullptr, &prep);
}

extern "C" int grkgpu_jp2_decompress_batch(grkgpu_ctx *c, grkgpu_batch_item *items, const grkgpu_out_ops *ops,
                                           uint32_t n, const grkgpu_dparams *p, grkgpu_batch_info *info,
                                           grkgpu_jp2_info *infos) {
    return jp2_batch(c, items, ops, n, p, info, infos, false);
}

extern "C" int grkgpu_jp2_batch_plan(grkgpu_batch_item *items, const grkgpu_out_ops *ops, uint32_t n,
                                     const grkgpu_dparams *p, grkgpu_batch_info *info, grkgpu_jp2_info *infos) {
    return jp2_batch(nullptr, items, ops, n, p, info, infos, true);
}

static int jp2_wparams_of(const grkgpu_image_desc *img, const grkgpu_jp2_wparams *wp, Jp2WriteParams &w) {
    if (!img || !wp) return set_err(GRKGPU_EINVAL, "null argument");
    if (img->numcomps < 1 || img->numcomps > GRKGPU_MAX_COMPS || img->x1 <= img->x0 || img->y1 <= img->y0)
        return set_err(GRKGPU_EINVAL, "bad image");
    if (wp->colour_space > GRKGPU_CS_ICC) return set_err(GRKGPU_EINVAL, "unknown colour space");
    w.w = img->x1 - img->x0;
    w.h = img->y1 - img->y0;
    w.numcomps = img->numcomps;
    uint64_t bytes = 0;  // jp2_start_compress (:2681-2688): above 2^30 the reference writes an XL jp2c
    for (uint32_t k = 0; k < img->numcomps; ++k) {
        if (img->prec[k] < 1 || img->prec[k] > 16) return set_err(GRKGPU_EINVAL, "bad component precision");
        if (wp->alpha[k] > 0xffff) return set_err(GRKGPU_EINVAL, "alpha type out of range");
        w.prec[k] = img->prec[k];
        w.sgnd[k] = img->sgnd[k];
        w.alpha[k] = wp->alpha[k];
        const uint32_t dx = img->dx[k] ? img->dx[k] : 1, dy = img->dy[k] ? img->dy[k] : 1;
        const uint64_t cw = ((uint64_t)img->x1 + dx - 1) / dx - ((uint64_t)img->x0 + dx - 1) / dx;
        const uint64_t chh = ((uint64_t)img->y1 + dy - 1) / dy - ((uint64_t)img->y0 + dy - 1) / dy;
        bytes += cw * chh * ((img->prec[k] + 7) / 8);
    }
    if (bytes > (1ull << 30)) return set_err(GRKGPU_EUNSUPPORTED, "JP2: an image this large needs an XL jp2c box, which is not written");
    w.colour_space = wp->colour_space;
    w.icc = wp->icc;
    w.icc_len = wp->icc_len;
    return GRKGPU_OK;
}

extern "C" int grkgpu_jp2_write_boxes(const grkgpu_image_desc *img, const grkgpu_jp2_wparams *wp, uint64_t cs_len,
                                      uint8_t *buf, size_t cap, size_t *n) {
    if (!n) return set_err(GRKGPU_EINVAL, "null argument");
    Jp2WriteParams w;
    int rc = jp2_wparams_of(img, wp, w);
    if (rc) return rc;
    std::vector<uint8_t> boxes;
    std::string err;
    if (!jp2_write_boxes(w, boxes, err)) return set_err(GRKGPU_EINVAL, err);
    if (cs_len + 8 >= (1ull << 32)) return set_err(GRKGPU_EUNSUPPORTED, "JP2: codestream too long for a 32-bit LBox");
    const uint32_t lbox = (uint32_t)(cs_len + 8);
    for (int i = 0; i < 4; ++i) boxes[boxes.size() - 8 + i] = (uint8_t)(lbox >> (8 * (3 - i)));
    *n = boxes.size();
    if (!buf || cap < boxes.size()) return set_err(GRKGPU_EINVAL, "box buffer too small");
    memcpy(buf, boxes.data(), boxes.size());
    return GRKGPU_OK;
}

extern "C" int grkgpu_jp2_compress(grkgpu_ctx *c, const grkgpu_image_desc *img, const grkgpu_cparams *p,
                                   const grkgpu_jp2_wparams *wp, const grkgpu_planes *in, const uint8_t **out,
                                   size_t *outlen) {
    if (!c || !in || !out || !outlen) return set_err(GRKGPU_EINVAL, "null argument");
    if (in->nrows || in->row0 || in->ncols || in->col0) return set_err(GRKGPU_EINVAL, "a JP2 file holds the whole image");
    Jp2WriteParams w;
    int rc = jp2_wparams_of(img, wp, w);
    if (rc) return rc;
    std::vector<uint8_t> boxes;
    std::string err;
    if (!jp2_write_boxes(w, boxes, err)) return set_err(GRKGPU_EINVAL, err);
    return compress_impl(c, img, p, in->planes, in->on_device, (int32_t)in->sample_fmt, out, outlen, 0, 0xffffffffu,
                         GRKGPU_PART_ALL, false, 0, 0, 0, 0, 0, &boxes);
}

// ---------------------------------------------------------------------------
// stage entry points
// ---------------------------------------------------------------------------
extern "C" int grkgpu_dcshift_mct_fwd(int32_t *const *planes, uint32_t numcomps, uint32_t w, uint32_t h,
                                      uint32_t stride, const int32_t *shift, int32_t mct, int32_t irreversible,
                                      void *stream) {
    if (!planes || !shift || numcomps < 1 || numcomps > 16) return set_err(GRKGPU_EINVAL, "bad arguments");
    int rc = check_device(-1);
    if (rc) return rc;
    PlanePtrs p{};
    SrcPlanes ps{};
    ShiftArr sh{};
    for (uint32_t k = 0; k < numcomps; ++k) { p.p[k] = planes[k]; ps.p[k] = planes[k]; sh.v[k] = shift[k]; }
    HIPCHK(launch_dcshift_mct_fwd(ps, SMP_I32, stride, p, w, h, numcomps, sh, mct, irreversible, (hipStream_t)stream));
    return GRKGPU_OK;
}

extern "C" int grkgpu_dcshift_mct_fwd_from(const grkgpu_planes *src, uint32_t numcomps, uint32_t w, uint32_t h,
                                           uint32_t src_stride, const int32_t *shift, int32_t mct,
                                           int32_t irreversible, int32_t *const *dst, uint32_t dst_stride,
                                           void *stream) {
    if (!src || !shift || !dst || numcomps < 1 || numcomps > 16) return set_err(GRKGPU_EINVAL, "bad arguments");
    const int32_t fmt = (int32_t)(src->sample_fmt & 0xffu), flags = (int32_t)(src->sample_fmt & ~0xffu);
    if (flags & ~(SMP_INTERLEAVED | SMP_BIG_ENDIAN)) return set_err(GRKGPU_EINVAL, "unknown sample format flags");
    if (fmt > SMP_I16) return set_err(GRKGPU_EINVAL, "unknown sample format");
    if ((flags & SMP_BIG_ENDIAN) && fmt != SMP_U16 && fmt != SMP_I16)
        return set_err(GRKGPU_EINVAL, "big-endian samples are 16-bit (U16 / I16)");
    const bool il = (flags & SMP_INTERLEAVED) != 0;
    if ((uint64_t)src_stride < (uint64_t)w * (il ? numcomps : 1) || dst_stride < w)
        return set_err(GRKGPU_EINVAL, "bad arguments (strides must hold a row)");
    SrcPlanes ps{};
    PlanePtrs p{};
    ShiftArr sh{};
    for (uint32_t k = 0; k < numcomps; ++k) {
        if (!dst[k] || (uintptr_t)dst[k] % 4 || (!(il && k) && !src->planes[k]))
            return set_err(GRKGPU_EINVAL, "null or misaligned plane");
        p.p[k] = dst[k];
        ps.p[k] = il ? src->planes[0] : src->planes[k];
        sh.v[k] = shift[k];
    }
    int rc = check_device(-1);
    if (rc) return rc;
    HIPCHK(launch_dcshift_mct_fwd_from(ps, fmt | flags, src_stride, p, dst_stride, w, h, numcomps, sh, mct,
                                       irreversible, (hipStream_t)stream));
    return GRKGPU_OK;
}

extern "C" int grkgpu_mct_inv_dcshift(int32_t *const *planes, uint32_t numcomps, uint32_t w, uint32_t h,
                                      uint32_t stride, const uint32_t *prec, const int32_t *sgnd, int32_t mct,
                                      int32_t irreversible, void *stream) {
    if (!planes || !prec || !sgnd || numcomps < 1 || numcomps > 16 || stride < w)
        return set_err(GRKGPU_EINVAL, "bad arguments (stride must be >= w)");
    int rc = check_device(-1);
    if (rc) return rc;
    PlanePtrs p{};
    ShiftArr sh{}, mn{}, mx{};
    for (uint32_t k = 0; k < numcomps; ++k) {
        p.p[k] = planes[k];
        set_range(k, prec[k], sgnd[k], mn, mx, &sh);
    }
    HIPCHK(launch_mct_inv_dcshift(p, stride, w, h, p, stride, numcomps, sh, mn, mx, mct, irreversible ? 0xFFFF : 0,
                                  (hipStream_t)stream));
    return GRKGPU_OK;
}

extern "C" int grkgpu_mct_inv_dcshift_to(const int32_t *const *src, uint32_t numcomps, uint32_t w, uint32_t h,
                                         uint32_t src_stride, const uint32_t *prec, const int32_t *sgnd, int32_t mct,
                                         int32_t irreversible, const grkgpu_out_planes *dst, uint32_t dst_stride,
                                         void *stream) {
    int rc = check_out_planes(dst);
    if (rc) return rc;
    if (dst->layout & GRKGPU_LAYOUT_UPSAMPLE) return set_err(GRKGPU_EINVAL, "unknown layout");
    const bool il = dst->layout == GRKGPU_LAYOUT_INTERLEAVED;
    const int32_t fmt = (int32_t)dst->sample_fmt;
    if (!src || !prec || !sgnd || numcomps < 1 || numcomps > 16 || src_stride < w ||
        (uint64_t)dst_stride < (uint64_t)w * (il ? numcomps : 1))
        return set_err(GRKGPU_EINVAL, "bad arguments (strides must hold a row)");
    PlanePtrs p{};
    DstPlanes d{};
    ShiftArr sh{}, mn{}, mx{};
    for (uint32_t k = 0; k < numcomps; ++k) {
        if (prec[k] < 1 || prec[k] > 31 || !src[k]) return set_err(GRKGPU_EINVAL, "bad arguments");
        if (!fmt_holds(fmt, prec[k], sgnd[k]))
            return set_err(GRKGPU_EINVAL, "sample format does not hold the component's precision / signedness");
        p.p[k] = const_cast<int32_t *>(src[k]);
        set_range(k, prec[k], sgnd[k], mn, mx, &sh);
    }
    rc = bind_dst(dst->planes, il ? 1u : numcomps, fmt, &d);
    if (rc) return rc;
    rc = check_device(-1);
    if (rc) return rc;
    HIPCHK(launch_mct_inv_dcshift_to(p, src_stride, w, h, d, fmt, il, dst_stride, numcomps, sh, mn, mx, mct,
                                     irreversible ? 0xFFFF : 0, (hipStream_t)stream));
    return GRKGPU_OK;
}

extern "C" int grkgpu_mct_inv_dcshift_jobs_to(const grkgpu_store_job *jobs, uint32_t n, uint32_t sample_fmt,
                                              uint32_t layout, void *stream) {
    if (sample_fmt > GRKGPU_SAMPLE_I16) return set_err(GRKGPU_EINVAL, "unknown sample format");
    if (layout > GRKGPU_LAYOUT_INTERLEAVED) return set_err(GRKGPU_EINVAL, "unknown layout");
    if (!n) return GRKGPU_OK;
    if (!jobs) return set_err(GRKGPU_EINVAL, "null argument");
    const int32_t fmt = (int32_t)sample_fmt;
    const bool il = layout == GRKGPU_LAYOUT_INTERLEAVED;
    const uint32_t sb = sample_bytes(fmt);
    const bool sg = fmt == SMP_I8 || fmt == SMP_I16;
    const int64_t lo = fmt == SMP_I32 ? INT32_MIN : (sg ? -((int64_t)1 << (8 * sb - 1)) : 0);
    const int64_t hi = fmt == SMP_I32 ? INT32_MAX : (sg ? ((int64_t)1 << (8 * sb - 1)) - 1 : ((int64_t)1 << (8 * sb)) - 1);
    StorePlan stores;
    for (uint32_t i = 0; i < n; ++i) {
        const grkgpu_store_job &q = jobs[i];
        const uint32_t nc = q.numcomps;
        if (nc < 1 || nc > 4 || q.src_stride < q.w || (uint64_t)q.dst_stride < (uint64_t)q.w * (il ? nc : 1))
            return set_err(GRKGPU_EINVAL, "bad arguments (1 .. 4 components, strides must hold a row)");
        if (q.wavelet_mask >> nc) return set_err(GRKGPU_EINVAL, "wavelet mask names a component the job does not have");
        StoreJob j;
        static_assert(sizeof(j) == sizeof(q), "grkgpu_store_job is StoreJob");
        memcpy(&j, &q, sizeof(j));
        for (uint32_t k = nc; k < 4; ++k) j.src[k] = nullptr;
        for (uint32_t k = 0; k < nc; ++k) {
            if (!q.src[k] || (uintptr_t)q.src[k] % 4) return set_err(GRKGPU_EINVAL, "null or misaligned source plane");
            if (q.min[k] > q.max[k] || q.min[k] < lo || q.max[k] > hi)
                return set_err(GRKGPU_EINVAL, "sample format does not hold the component's range");
        }
        if (int rc = bind_dst(q.dst, il ? 1u : nc, fmt)) return rc;
        if (!stores.add_store(fmt, il, j)) stores.singles.push_back(tile_store_of(j, fmt, il));
    }
    int rc = check_device(-1);
    if (rc) return rc;
    return stores.run_alone((hipStream_t)stream);
}

static_assert(sizeof(grkgpu_palette_job) == sizeof(PalJob) && offsetof(grkgpu_palette_job, ops_) == offsetof(PalJob, s.ops) &&
                  offsetof(grkgpu_palette_job, max) == offsetof(PalJob, s.mx) &&
                  offsetof(grkgpu_palette_job, chan_comp) == offsetof(PalJob, map.comp) &&
                  offsetof(grkgpu_palette_job, chan_pcol) == offsetof(PalJob, map.pcol) &&
                  offsetof(grkgpu_palette_job, numchannels) == offsetof(PalJob, map.nch) &&
                  offsetof(grkgpu_palette_job, ne) == offsetof(PalJob, map.ne) &&
                  offsetof(grkgpu_palette_job, npc) == offsetof(PalJob, map.npc) &&
                  offsetof(grkgpu_palette_job, used_) == offsetof(PalJob, map.used) &&
                  offsetof(grkgpu_palette_job, zero) == offsetof(PalJob, map.zero) &&
                  offsetof(grkgpu_palette_job, table_off) == offsetof(PalJob, table_off),
              "grkgpu_palette_job is PalJob");

extern "C" int grkgpu_palette_jobs_to(const grkgpu_palette_job *jobs, uint32_t n, const uint16_t *table,
                                      uint32_t table_entries, uint32_t sample_fmt, uint32_t layout, void *stream) {
    if (sample_fmt > GRKGPU_SAMPLE_I16) return set_err(GRKGPU_EINVAL, "unknown sample format");
    if (layout > GRKGPU_LAYOUT_INTERLEAVED) return set_err(GRKGPU_EINVAL, "unknown layout");
    if (!n) return GRKGPU_OK;
    if (!jobs) return set_err(GRKGPU_EINVAL, "null argument");
    if (table && (uintptr_t)table % 4) return set_err(GRKGPU_EINVAL, "misaligned palette table");
    const int32_t fmt = (int32_t)sample_fmt;
    const bool il = layout == GRKGPU_LAYOUT_INTERLEAVED;
    const uint32_t sb = sample_bytes(fmt);
    const bool sg = fmt == SMP_I8 || fmt == SMP_I16;
    const int64_t lo = fmt == SMP_I32 ? INT32_MIN : (sg ? -((int64_t)1 << (8 * sb - 1)) : 0);
    const int64_t hi = fmt == SMP_I32 ? INT32_MAX : (sg ? ((int64_t)1 << (8 * sb - 1)) - 1 : ((int64_t)1 << (8 * sb)) - 1);
    StorePlan stores;
    stores.pal_table = table;
    for (uint32_t i = 0; i < n; ++i) {
        const grkgpu_palette_job &q = jobs[i];
        const uint32_t nc = q.numcomps, nch = q.numchannels;
        if (nc < 1 || nc > 4 || nch < 1 || nch > 4 || (!q.zero && q.src_stride < q.w) ||
            (uint64_t)q.dst_stride < (uint64_t)q.w * (il ? nch : 1))
            return set_err(GRKGPU_EINVAL, "bad arguments (1 .. 4 components and channels, strides must hold a row)");
        if (q.wavelet_mask >> nc) return set_err(GRKGPU_EINVAL, "wavelet mask names a component the job does not have");
        if (q.ne > 1024 || q.npc > 16 || (q.ne != 0) != (q.npc != 0))
            return set_err(GRKGPU_EINVAL, "palette of 1 .. 1024 x 1 .. 16 entries");
        // every entry the kernel reads lies inside the merged table
        if (q.ne && (!table || (q.table_off & 1) || (uint64_t)q.table_off + (uint64_t)q.ne * q.npc > table_entries))
            return set_err(GRKGPU_EINVAL, "palette table outside the merged table (table_off must be even)");
        PalJob j;
        memcpy(&j, &q, sizeof(j));
        j.s.ops = 0;
        j.map.zero = q.zero ? 1 : 0;
        for (uint32_t k = q.zero ? 0 : nc; k < 4; ++k) j.s.src[k] = nullptr;
        for (uint32_t k = il ? 1u : nch; k < 4; ++k) j.s.dst[k] = nullptr;
        bool looks_up = false;
        for (uint32_t ch = 0; ch < nch; ++ch) {
            const uint32_t k = q.chan_comp[ch];
            if (k >= nc || q.chan_pcol[ch] >= (int32_t)q.npc)
                return set_err(GRKGPU_EINVAL, "channel map outside the components / the palette");
            if (q.chan_pcol[ch] < 0) {
                j.map.pcol[ch] = -1;
                if (q.min[k] > q.max[k] || q.min[k] < lo || q.max[k] > hi)
                    return set_err(GRKGPU_EINVAL, "sample format does not hold the component's range");
            } else {
                looks_up = true;
            }
        }
        if (looks_up != (q.ne != 0)) return set_err(GRKGPU_EINVAL, "a table exactly when a channel looks up");
        set_pal_used(j.map);
        for (uint32_t k = 0; !q.zero && k < nc; ++k)
            if (((j.map.used >> k) & 1 || (q.mct && nc >= 3 && k < 3)) && (!q.src[k] || (uintptr_t)q.src[k] % 4))
                return set_err(GRKGPU_EINVAL, "null or misaligned source plane");
        if (int rc = bind_dst(q.dst, il ? 1u : nch, fmt)) return rc;
        if (!stores.add_pal(fmt, il, nullptr, j, 0)) {
            TilePal t{};
            t.ts = tile_store_of(j.s, fmt, il);
            for (uint32_t k = 0; k < (il ? 1u : nch); ++k) t.ts.dst.p[k] = q.dst[k];
            t.map = j.map;
            t.table_off = j.table_off;
            stores.pal_singles.push_back(t);
        }
    }
    int rc = check_device(-1);
    if (rc) return rc;
    return stores.run_alone((hipStream_t)stream);
}

extern "C" int grkgpu_dcshift_mct_fwd_jobs(grkgpu_ctx *c, const grkgpu_load_job *jobs, uint32_t n,
                                           uint32_t sample_fmt) {
    if (!c) return set_err(GRKGPU_EINVAL, "null ctx");
    const int32_t fflags = (int32_t)sample_fmt & ~0xff, fmt = (int32_t)sample_fmt & 0xff;
    if (fflags & ~(SMP_INTERLEAVED | SMP_BIG_ENDIAN)) return set_err(GRKGPU_EINVAL, "unknown sample format flags");
    if (fmt < SMP_I32 || fmt > SMP_I16) return set_err(GRKGPU_EINVAL, "unknown sample format");
    if ((fflags & SMP_BIG_ENDIAN) && fmt != SMP_U16 && fmt != SMP_I16)
        return set_err(GRKGPU_EINVAL, "big-endian samples are 16-bit (U16 / I16)");
    if (!n) return GRKGPU_OK;
    if (!jobs) return set_err(GRKGPU_EINVAL, "null argument");
    const int32_t lfmt = fmt | fflags;
    const bool il = (fflags & SMP_INTERLEAVED) != 0;
    const uint32_t sb = sample_bytes(fmt);
    LoadPlan loads;
    for (uint32_t i = 0; i < n; ++i) {
        const grkgpu_load_job &q = jobs[i];
        const uint32_t nc = q.numcomps;
        if (nc < 1 || nc > 4 || q.dst_stride < q.w || (uint64_t)q.src_stride < (uint64_t)q.w * (il ? nc : 1))
            return set_err(GRKGPU_EINVAL, "bad arguments (1 .. 4 components, strides must hold a row)");
        LoadJob j;
        memcpy(&j, &q, sizeof(j));
        j.pad_ = 0;
        for (uint32_t k = nc; k < 4; ++k) { j.src[k] = nullptr; j.dst[k] = nullptr; }
        for (uint32_t k = 0; k < (il ? 1u : nc); ++k)
            // planar samples in host byte order are read with typed loads
            if (!q.src[k] || (!fflags && (uintptr_t)q.src[k] % sb))
                return set_err(GRKGPU_EINVAL, "null or misaligned source plane");
        for (uint32_t k = 0; k < nc; ++k)
            if (!q.dst[k] || (uintptr_t)q.dst[k] % 4) return set_err(GRKGPU_EINVAL, "null or misaligned output plane");
        if (!loads.add(lfmt, j)) loads.singles.push_back(tile_load_of(j, lfmt));
    }
    int rc = check_device(c->device);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HIPCHK(c->loadjobs.ensure(loads.table.bytes() + 256));
    HIPCHK(c->h_loadjobs.ensure(loads.table.bytes() + 256));
    HIPCHK(loads.upload(c->h_loadjobs.as<uint8_t>(), c->loadjobs.p, s));
    HIPCHK(loads.launch(c->loadjobs.p, s, nullptr));
    HIPCHK(hipStreamSynchronize(s));  // the staging is the context's: free for the next call
    return GRKGPU_OK;
}

extern "C" int grkgpu_mct_inv_custom_to(const float *const *src, uint32_t numcomps, uint32_t w, uint32_t h,
                                        uint32_t src_stride, const float *matrix, const int32_t *offsets,
                                        const uint32_t *prec, const int32_t *sgnd, const grkgpu_out_planes *dst,
                                        uint32_t dst_stride, void *stream) {
    int rc = check_out_planes(dst);
    if (rc) return rc;
    if (dst->layout & GRKGPU_LAYOUT_UPSAMPLE) return set_err(GRKGPU_EINVAL, "unknown layout");
    const bool il = dst->layout == GRKGPU_LAYOUT_INTERLEAVED;
    const int32_t fmt = (int32_t)dst->sample_fmt;
    if (!src || !matrix || !prec || !sgnd || numcomps < 1 || numcomps > 16 || src_stride < w ||
        (uint64_t)dst_stride < (uint64_t)w * (il ? numcomps : 1))
        return set_err(GRKGPU_EINVAL, "bad arguments (strides must hold a row)");
    PlanePtrs p{};
    DstPlanes d{};
    ShiftArr off{}, mn{}, mx{};
    MctInv m{};
    for (uint32_t i = 0; i < numcomps * numcomps; ++i)
        if (!(matrix[i] - matrix[i] == 0.0f)) return set_err(GRKGPU_EINVAL, "non-finite matrix entry");
    set_mct_inv(m, matrix, numcomps);
    for (uint32_t k = 0; k < numcomps; ++k) {
        if (prec[k] < 1 || prec[k] > 31 || !src[k] || (uintptr_t)src[k] % 4)
            return set_err(GRKGPU_EINVAL, "bad arguments");
        if (!fmt_holds(fmt, prec[k], sgnd[k]))
            return set_err(GRKGPU_EINVAL, "sample format does not hold the component's precision / signedness");
        p.p[k] = reinterpret_cast<int32_t *>(const_cast<float *>(src[k]));
        off.v[k] = offsets ? offsets[k] : 0;
        set_range(k, prec[k], sgnd[k], mn, mx);
    }
    rc = bind_dst(dst->planes, il ? 1u : numcomps, fmt, &d);
    if (rc) return rc;
    rc = check_device(-1);
    if (rc) return rc;
    HIPCHK(launch_mct_inv_custom(p, src_stride, w, h, d, fmt, il, dst_stride, numcomps, m, off, mn, mx, nullptr,
                                 (hipStream_t)stream));
    return GRKGPU_OK;
}

extern "C" int grkgpu_palette_to(const int32_t *const *src, uint32_t numcomps, uint32_t w, uint32_t h,
                                 uint32_t src_stride, const uint32_t *prec, const int32_t *sgnd, uint32_t numchannels,
                                 const uint32_t *chan_comp, const int32_t *chan_pcol, const uint32_t *chan_prec,
                                 const uint16_t *table, uint32_t ne, uint32_t npc, const grkgpu_out_planes *dst,
                                 uint32_t dst_stride, void *stream) {
    int rc = check_out_planes(dst);
    if (rc) return rc;
    if (dst->layout & GRKGPU_LAYOUT_UPSAMPLE) return set_err(GRKGPU_EINVAL, "unknown layout");
    const bool il = dst->layout == GRKGPU_LAYOUT_INTERLEAVED;
    const int32_t fmt = (int32_t)dst->sample_fmt;
    if (!src || !prec || !sgnd || !chan_comp || !chan_pcol || !chan_prec || numcomps < 1 || numcomps > 16 ||
        numchannels < 1 || numchannels > 16 || src_stride < w ||
        (uint64_t)dst_stride < (uint64_t)w * (il ? numchannels : 1))
        return set_err(GRKGPU_EINVAL, "bad arguments (strides must hold a row)");
    if (ne > 1024 || npc > 16 || (table && (!ne || !npc))) return set_err(GRKGPU_EINVAL, "palette of 1 .. 1024 x 1 .. 16 entries");
    PlanePtrs p{};
    DstPlanes d{};
    ShiftArr sh{}, mn{}, mx{};
    for (uint32_t k = 0; k < numcomps; ++k) {
        if (prec[k] < 1 || prec[k] > 31 || !src[k] || (uintptr_t)src[k] % 4) return set_err(GRKGPU_EINVAL, "bad arguments");
        p.p[k] = const_cast<int32_t *>(src[k]);
        set_range(k, prec[k], sgnd[k], mn, mx, &sh);
    }
    PalMap map{};
    map.nch = numchannels;
    map.ne = table ? ne : 0;
    map.npc = table ? npc : 0;
    for (uint32_t ch = 0; ch < numchannels; ++ch) {
        if (chan_comp[ch] >= numcomps || chan_pcol[ch] >= (int32_t)map.npc || chan_prec[ch] < 1 || chan_prec[ch] > 31)
            return set_err(GRKGPU_EINVAL, "channel map outside the components / the palette");
        const bool chs = chan_pcol[ch] < 0 && sgnd[chan_comp[ch]];
        const uint32_t chp = chan_pcol[ch] < 0 ? std::max(chan_prec[ch], prec[chan_comp[ch]]) : chan_prec[ch];
        if (!fmt_holds(fmt, chp, chs))
            return set_err(GRKGPU_EINVAL, "sample format does not hold the channel's precision / signedness");
        map.comp[ch] = (uint8_t)chan_comp[ch];
        map.pcol[ch] = (int8_t)(chan_pcol[ch] < 0 ? -1 : chan_pcol[ch]);
    }
    set_pal_used(map);
    rc = bind_dst(dst->planes, il ? 1u : numchannels, fmt, &d);
    if (rc) return rc;
    rc = check_device(-1);
    if (rc) return rc;
    HIPCHK(launch_palette(p, src_stride, w, h, d, fmt, il, dst_stride, numcomps, sh, mn, mx, 0, 0, map, table, nullptr,
                          (hipStream_t)stream));
    return GRKGPU_OK;
}

extern "C" int grkgpu_upsample_to(const void *const *src, const uint32_t *src_stride, uint32_t numcomps,
                                  const uint32_t *dx, const uint32_t *dy, uint32_t x0, uint32_t y0, uint32_t x1,
                                  uint32_t y1, const grkgpu_out_planes *dst, uint32_t dst_stride, void *stream) {
    int rc = check_out_planes(dst);
    if (rc) return rc;
    const bool il = (dst->layout & ~GRKGPU_LAYOUT_UPSAMPLE) == GRKGPU_LAYOUT_INTERLEAVED;
    const int32_t fmt = (int32_t)dst->sample_fmt;
    const uint32_t sb = sample_bytes(fmt);
    if (!src || !src_stride || !dx || !dy || numcomps < 1 || numcomps > 16 || x1 <= x0 || y1 <= y0 ||
        x1 > 0x7fffffffu || y1 > 0x7fffffffu)
        return set_err(GRKGPU_EINVAL, "bad arguments");
    if ((uint64_t)dst_stride < (uint64_t)(x1 - x0) * (il ? numcomps : 1))
        return set_err(GRKGPU_EINVAL, "bad arguments (strides must hold a row)");
    UpPlan pl{};
    DstPlanes d{};
    for (uint32_t k = 0; k < numcomps; ++k) {
        if (dx[k] < 1 || dx[k] > 255 || dy[k] < 1 || dy[k] > 255)
            return set_err(GRKGPU_EINVAL, "bad arguments (dx / dy must be 1 .. 255)");
        const Rect cr = comp_rect({x0, y0, x1, y1}, dx[k], dy[k]);
        if (src_stride[k] < cr.w()) return set_err(GRKGPU_EINVAL, "bad arguments (strides must hold a row)");
        // (a grid without a sample inside the rectangle has no plane: every index is negative)
        if ((!src[k] && !cr.empty()) || (uintptr_t)src[k] % sb)
            return set_err(GRKGPU_EINVAL, "null or misaligned plane");
        pl.c[k] = UpComp{src[k], src_stride[k], (int32_t)cr.x0, (int32_t)cr.y0, (int32_t)cr.x0, (int32_t)cr.y0,
                         (uint8_t)dx[k], (uint8_t)dy[k], 0, 0, 0, 0, 0};
    }
    rc = bind_dst(dst->planes, il ? 1u : numcomps, fmt, &d);
    if (rc) return rc;
    rc = check_device(-1);
    if (rc) return rc;
    HIPCHK(launch_upsample_to(pl, numcomps, x0, y0, x1 - x0, y1 - y0, d, fmt, il, dst_stride, (hipStream_t)stream));
    return GRKGPU_OK;
}

extern "C" int grkgpu_convert_to(const void *const *src, const uint32_t *src_stride, uint32_t src_fmt,
                                 uint32_t numcomps, const uint32_t *dx, const uint32_t *dy, const uint32_t *prec,
                                 const int32_t *sgnd, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                                 const grkgpu_out_planes *dst, uint32_t dst_stride, const grkgpu_out_ops *ops,
                                 void *stream) {
    int rc = check_out_planes(dst);
    if (rc) return rc;
    rc = check_out_ops(ops, dst->sample_fmt);
    if (rc) return rc;
    if (src_fmt > GRKGPU_SAMPLE_I16) return set_err(GRKGPU_EINVAL, "unknown sample format");
    const bool il = (dst->layout & ~GRKGPU_LAYOUT_UPSAMPLE) == GRKGPU_LAYOUT_INTERLEAVED;
    const int32_t fmt = (int32_t)dst->sample_fmt, sfmt = (int32_t)src_fmt;
    const uint32_t ssb = sample_bytes(sfmt);
    if (!src || !src_stride || !dx || !dy || !prec || !sgnd || numcomps < 1 || numcomps > 16 || x1 <= x0 ||
        y1 <= y0 || x1 > 0x7fffffffu || y1 > 0x7fffffffu)
        return set_err(GRKGPU_EINVAL, "bad arguments");
    // the channels dst describes: the components, one fewer after CMYK, and
    // channel 0 three times where force-RGB finds one or two
    const bool force_rgb = ops && (ops->colour & GRKGPU_COLOUR_FORCE_RGB);
    const bool colconv = ops && colour_of(ops) != GRKGPU_COLOUR_NONE;
    const uint32_t nbefore = ops && colour_of(ops) == GRKGPU_COLOUR_CMYK && numcomps >= 4 ? numcomps - 1 : numcomps;
    const bool forced = force_rgb && nbefore <= 2;
    const uint32_t nch = forced ? nbefore + 2 : nbefore;
    if (force_rgb && !forced && !colconv)
        return set_err(GRKGPU_EINVAL, "force-RGB: don't know how to convert these channels to RGB");
    if ((uint64_t)dst_stride < (uint64_t)(x1 - x0) * (il ? nch : 1))
        return set_err(GRKGPU_EINVAL, "bad arguments (strides must hold a row)");
    bool full = true;  // every component at (1,1)
    for (uint32_t k = 0; k < numcomps; ++k) {
        if (dx[k] < 1 || dx[k] > 255 || dy[k] < 1 || dy[k] > 255)
            return set_err(GRKGPU_EINVAL, "bad arguments (dx / dy must be 1 .. 255)");
        if (prec[k] < 1 || prec[k] > 31) return set_err(GRKGPU_EINVAL, "bad arguments (prec must be 1 .. 31)");
        if (!fmt_holds(sfmt, prec[k], sgnd[k]))
            return set_err(GRKGPU_EINVAL, "source format does not hold the component's precision / signedness");
        full = full && dx[k] == 1 && dy[k] == 1;
    }
    const grkgpu_out_ops none{};
    OutOps dops{};
    uint32_t oprec[GRKGPU_MAX_COMPS], no = numcomps;
    int32_t osgnd[GRKGPU_MAX_COMPS];
    uint32_t fprec[4] = {prec[0], prec[0], prec[0], numcomps > 1 ? prec[1] : 0};  // (forced: the channels)
    int32_t fsgnd[4] = {sgnd[0], sgnd[0], sgnd[0], numcomps > 1 ? sgnd[1] : 0};
    if (forced) {
        const uint32_t one[4] = {1, 1, 1, 1};
        if (colconv) {  // (no conversion takes one or two components: its own refusal)
            rc = resolve_out_ops(ops, numcomps, prec, sgnd, dx, dy, dops, no, oprec, osgnd);
            return rc ? rc : set_err(GRKGPU_EINVAL, "bad arguments");
        }
        rc = resolve_out_ops(ops, nch, fprec, fsgnd, one, one, dops, no, oprec, osgnd);
    } else {
        rc = resolve_out_ops(ops ? ops : &none, numcomps, prec, sgnd, dx, dy, dops, no, oprec, osgnd);
    }
    if (rc) return rc;
    UpPlan pl{};
    DstPlanes d{};
    for (uint32_t k = 0; k < no; ++k)
        if (!fmt_holds(fmt, oprec[k], osgnd[k]))
            return set_err(GRKGPU_EINVAL, "sample format does not hold the output precision / signedness");
    for (uint32_t k = 0; k < numcomps; ++k) {
        const Rect cr = comp_rect({x0, y0, x1, y1}, dx[k], dy[k]);
        if (src_stride[k] < cr.w()) return set_err(GRKGPU_EINVAL, "bad arguments (strides must hold a row)");
        // (a grid without a sample inside the rectangle has no plane: every index is negative)
        if ((!src[k] && !cr.empty()) || (uintptr_t)src[k] % ssb)
            return set_err(GRKGPU_EINVAL, "null or misaligned plane");
        pl.c[k] = UpComp{src[k], src_stride[k], (int32_t)cr.x0, (int32_t)cr.y0, (int32_t)cr.x0, (int32_t)cr.y0,
                         (uint8_t)dx[k], (uint8_t)dy[k], (uint8_t)(UPCOMP_FIN + sfmt), 0, 0, 0, 0};
    }
    rc = bind_dst(dst->planes, il ? 1u : no, fmt, &d);
    if (rc) return rc;
    if (forced) {
        // channel 0 three times, a second one behind it: the palette kernels' direct map on finished int32 planes
        for (uint32_t k = 0; k < numcomps; ++k) full = full && src_stride[k] == src_stride[0];
        if (!full || sfmt != SMP_I32)
            return set_err(GRKGPU_EUNSUPPORTED, "force-RGB needs int32 sources at (1,1) with one row stride");
        rc = check_device(-1);
        if (rc) return rc;
        PlanePtrs p{};
        ShiftArr sh{}, mn{}, mx{};
        PalMap map{};
        map.nch = no;
        for (uint32_t ch = 0; ch < no; ++ch) { map.comp[ch] = ch < 3 ? 0 : 1; map.pcol[ch] = -1; }
        set_pal_used(map);
        for (uint32_t k = 0; k < numcomps; ++k) {
            p.p[k] = (int32_t *)const_cast<void *>(src[k]);
            set_range(k, prec[k], sgnd[k], mn, mx);
        }
        HIPCHK(launch_palette(p, src_stride[0], x1 - x0, y1 - y0, d, fmt, il, dst_stride, numcomps, sh, mn, mx, 0, 0, map,
                              nullptr, &dops, (hipStream_t)stream));
        return GRKGPU_OK;
    }
    rc = check_device(-1);
    if (rc) return rc;
    if (full && sfmt == SMP_I32) {
        // finished int32 samples on the image grid: the inverse-MCT kernels'
        // stores, their shift 0 and their clamp the component's own range
        PlanePtrs p{};
        ShiftArr sh{}, mn{}, mx{};
        uint32_t ss = src_stride[0];
        for (uint32_t k = 0; k < numcomps; ++k) {
            p.p[k] = (int32_t *)const_cast<void *>(src[k]);
            set_range(k, prec[k], sgnd[k], mn, mx);
            full = full && src_stride[k] == ss;
        }
        if (full) {
            HIPCHK(launch_mct_inv_dcshift_ops(p, ss, x1 - x0, y1 - y0, d, fmt, il, dst_stride, numcomps, sh, mn, mx, 0,
                                              0, dops, (hipStream_t)stream));
            return GRKGPU_OK;
        }
    }
    HIPCHK(launch_upsample_ops(pl, numcomps, x0, y0, x1 - x0, y1 - y0, d, fmt, il, dst_stride, dops,
                               (hipStream_t)stream));
    return GRKGPU_OK;
}

static_assert(sizeof(grkgpu_convert_comp) == sizeof(UpComp) && offsetof(grkgpu_convert_comp, stride) == offsetof(UpComp, stride) &&
                  offsetof(grkgpu_convert_comp, gx0) == offsetof(UpComp, gx0) &&
                  offsetof(grkgpu_convert_comp, zy0) == offsetof(UpComp, zy0) &&
                  offsetof(grkgpu_convert_comp, dx) == offsetof(UpComp, dx) &&
                  offsetof(grkgpu_convert_comp, kind) == offsetof(UpComp, raw) &&
                  offsetof(grkgpu_convert_comp, wavelet) == offsetof(UpComp, irrev) &&
                  offsetof(grkgpu_convert_comp, shift) == offsetof(UpComp, shift) &&
                  offsetof(grkgpu_convert_comp, max) == offsetof(UpComp, mx),
              "grkgpu_convert_comp is UpComp");
static_assert(sizeof(grkgpu_convert_job) == sizeof(ConvJob) + sizeof(grkgpu_out_ops) &&
                  offsetof(grkgpu_convert_job, ops) == sizeof(ConvJob) &&
                  offsetof(grkgpu_convert_job, dst) == offsetof(ConvJob, dst) &&
                  offsetof(grkgpu_convert_job, x0) == offsetof(ConvJob, X0) &&
                  offsetof(grkgpu_convert_job, y1) == offsetof(ConvJob, y1) &&
                  offsetof(grkgpu_convert_job, dst_stride) == offsetof(ConvJob, dstride) &&
                  offsetof(grkgpu_convert_job, numcomps) == offsetof(ConvJob, ncomp) &&
                  offsetof(grkgpu_convert_job, mct) == offsetof(ConvJob, mct_) &&
                  offsetof(grkgpu_convert_job, pad_) == offsetof(ConvJob, ops),
              "grkgpu_convert_job is ConvJob with its ops behind it");
static_assert(GRKGPU_SRC_RAW == 1 && GRKGPU_SRC_SAMPLES == UPCOMP_FIN, "grkgpu_convert_comp.kind is UpComp::raw");

// the precision and sign whose range [mn, mx] is
static bool range_prec(int32_t mn, int32_t mx, uint32_t &prec, int32_t &sgnd) {
    if (mx < 0 || ((uint32_t)mx & ((uint32_t)mx + 1))) return false;  // 2^q - 1
    const uint32_t q = (uint32_t)__builtin_popcount((uint32_t)mx);
    if (mn == 0 && q >= 1) { prec = q; sgnd = 0; return true; }
    if (mn == -mx - 1 && q <= 30) { prec = q + 1; sgnd = 1; return true; }
    return false;
}

extern "C" int grkgpu_convert_jobs_to(const grkgpu_convert_job *jobs, uint32_t n, uint32_t sample_fmt, uint32_t layout,
                                      void *stream) {
    if (sample_fmt > GRKGPU_SAMPLE_I16) return set_err(GRKGPU_EINVAL, "unknown sample format");
    if (layout > GRKGPU_LAYOUT_INTERLEAVED) return set_err(GRKGPU_EINVAL, "unknown layout");
    if (!n) return GRKGPU_OK;
    if (!jobs) return set_err(GRKGPU_EINVAL, "null argument");
    const int32_t fmt = (int32_t)sample_fmt;
    const bool il = layout == GRKGPU_LAYOUT_INTERLEAVED;
    StorePlan T;
    for (uint32_t i = 0; i < n; ++i) {
        const grkgpu_convert_job &q = jobs[i];
        const uint32_t nc = q.numcomps;
        int rc = check_out_ops(&q.ops, sample_fmt);
        if (rc) return rc;
        if (q.ops.colour & GRKGPU_COLOUR_FORCE_RGB)
            return set_err(GRKGPU_EUNSUPPORTED, "force-RGB is not supported in a job table");
        if (nc < 1 || nc > 4 || q.x1 > 0x7fffffffu || q.y1 > 0x7fffffffu)
            return set_err(GRKGPU_EINVAL, "bad arguments (1 .. 4 components)");
        const bool empty = q.x1 <= q.x0 || q.y1 <= q.y0;
        uint32_t prec[4], dx[4], dy[4];
        int32_t sgnd[4];
        bool grid1 = true;  // raw sources on one grid, no lead-in inside the rectangle: a StoreJob
        for (uint32_t k = 0; k < nc; ++k) {
            const grkgpu_convert_comp &u = q.comp[k];
            if (!u.dx || !u.dy) return set_err(GRKGPU_EINVAL, "bad arguments (dx / dy must be 1 .. 255)");
            const bool raw = u.kind == GRKGPU_SRC_RAW;
            if (!raw && (u.kind < GRKGPU_SRC_SAMPLES || u.kind > GRKGPU_SRC_SAMPLES + GRKGPU_SAMPLE_I16))
                return set_err(GRKGPU_EINVAL, "unknown source kind");
            if (!range_prec(u.min, u.max, prec[k], sgnd[k]))
                return set_err(GRKGPU_EINVAL, "min / max must be the range of a precision and sign");
            const int32_t sf = raw ? (int32_t)SMP_I32 : (int32_t)(u.kind - GRKGPU_SRC_SAMPLES);
            if (!fmt_holds(sf, prec[k], sgnd[k]))
                return set_err(GRKGPU_EINVAL, "source format does not hold the component's precision / signedness");
            if ((uintptr_t)u.src % sample_bytes(sf)) return set_err(GRKGPU_EINVAL, "misaligned source");
            if (u.zx0 < u.gx0 || u.zy0 < u.gy0 || u.gx0 < 0 || u.gy0 < 0)
                return set_err(GRKGPU_EINVAL, "bad arguments (0 <= gx0 <= zx0, 0 <= gy0 <= zy0)");
            if (u.src && !empty && (int64_t)((q.x1 - 1) / u.dx) - u.gx0 >= (int64_t)u.stride)
                return set_err(GRKGPU_EINVAL, "bad arguments (strides must hold a row)");
            if (u.dx == 1 && u.dy == 1 && !empty && ((int64_t)u.zx0 > (int64_t)q.x0 || (int64_t)u.zy0 > (int64_t)q.y0))
                return set_err(GRKGPU_EINVAL, "bad arguments (a component at (1,1) has no lead-in)");
            dx[k] = u.dx; dy[k] = u.dy;
            grid1 = grid1 && raw && u.src && u.dx == 1 && u.dy == 1 && u.stride == q.comp[0].stride &&
                    u.gx0 == q.comp[0].gx0 && u.gy0 == q.comp[0].gy0 && (int64_t)u.zx0 <= (int64_t)q.x0 &&
                    (int64_t)u.zy0 <= (int64_t)q.y0;
        }
        if (q.mct && (!grid1 || nc < 3)) return set_err(GRKGPU_EINVAL, "an MCT needs three raw sources on one grid");
        OutOps dops{};
        uint32_t no = nc, oprec[GRKGPU_MAX_COMPS];
        int32_t osgnd[GRKGPU_MAX_COMPS];
        rc = resolve_out_ops(&q.ops, nc, prec, sgnd, dx, dy, dops, no, oprec, osgnd);
        if (rc) return rc;
        for (uint32_t k = 0; k < no; ++k)
            if (!fmt_holds(fmt, oprec[k], osgnd[k]))
                return set_err(GRKGPU_EINVAL, "sample format does not hold the output precision / signedness");
        if (empty) continue;
        const uint32_t w = q.x1 - q.x0;
        if ((uint64_t)q.dst_stride < (uint64_t)w * (il ? no : 1))
            return set_err(GRKGPU_EINVAL, "bad arguments (strides must hold a row)");
        rc = bind_dst(q.dst, il ? 1u : no, fmt);
        if (rc) return rc;
        const uint32_t ops_at = (uint32_t)T.ops.size();
        T.ops.push_back(dops);
        if (grid1) {
            StoreJob j{};
            for (uint32_t k = 0; k < nc; ++k) {
                const grkgpu_convert_comp &u = q.comp[k];
                j.src[k] = (const int32_t *)u.src + ((uint64_t)(q.y0 - (uint32_t)u.gy0) * u.stride + (q.x0 - (uint32_t)u.gx0));
                j.shift[k] = u.shift; j.mn[k] = u.min; j.mx[k] = u.max;
                j.irrev |= (u.wavelet ? 1u : 0u) << k;
            }
            for (uint32_t k = 0; k < (il ? 1u : no); ++k) j.dst[k] = q.dst[k];
            j.sstride = q.comp[0].stride; j.dstride = q.dst_stride; j.w = w; j.h = q.y1 - q.y0;
            j.ncomp = nc; j.mct = q.mct;
            if (!T.add_conv_store(fmt, il, dops, j, ops_at)) T.conv_singles.push_back({tile_store_of(j, fmt, il), dops});
            continue;
        }
        ConvJob j{};
        memcpy((void *)&j, &q, sizeof(j));  // (grkgpu_convert_job is ConvJob with its ops behind it)
        for (uint32_t k = nc; k < 4; ++k) j.c[k] = UpComp{};
        for (uint32_t k = il ? 1 : no; k < 4; ++k) j.dst[k] = nullptr;
        j.mct_ = 0;
        if (T.add_up(fmt, il, dops, j, ops_at)) continue;
        TileConv tc{UpPlan{}, nc, Rect{j.X0, j.Y0, j.x1, j.y1}, DstPlanes{}, fmt, il, j.dstride, dops, true};
        for (uint32_t k = 0; k < 4; ++k) { tc.pl.c[k] = j.c[k]; tc.dst.p[k] = j.dst[k]; }
        T.up_singles.push_back(tc);
    }
    int rc = check_device(-1);
    if (rc) return rc;
    return T.run_alone((hipStream_t)stream);
}

static void dwt_stage_geom(uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, uint32_t numres, int32_t irrev,
                           bool inverse, TileComp &tc) {
    CodingParams cp;
    cp.numcomps = 1;
    cp.image = {x0, y0, x1, y1};
    cp.prec[0] = 8;
    cp.numres = numres;
    cp.irrev = irrev;
    generate_qcd(cp);
    build_tilecomp(tc, cp.image, cp, 0, !inverse);
}

// scratch layout: [temporary copy of buf | LL ping-pong | job table]
extern "C" size_t grkgpu_dwt_scratch_bytes(uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, uint32_t numres) {
    if (x1 <= x0 || y1 <= y0 || numres < 1 || numres > 33) return 0;
    TileComp tc;
    dwt_stage_geom(x0, y0, x1, y1, numres, 0, false, tc);
    const uint64_t area = ((uint64_t)(x1 - x0) * (y1 - y0) + 63) / 64 * 64;
    return (size_t)(area + ll_geom(tc).elems) * 4 + 64 * sizeof(DwtJob) + 512;
}

static int dwt_common(int32_t *buf, int32_t *scratch, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                      uint32_t numres, int32_t irrev, void *stream, bool inverse) {
    if (!buf || !scratch || x1 <= x0 || y1 <= y0 || numres < 1 || numres > 33)
        return set_err(GRKGPU_EINVAL, "bad arguments");
    int rc = check_device(-1);
    if (rc) return rc;
    TileComp tc;
    dwt_stage_geom(x0, y0, x1, y1, numres, irrev, inverse, tc);
    const uint64_t area = ((uint64_t)(x1 - x0) * (y1 - y0) + 63) / 64 * 64;
    int32_t *tmp = scratch, *ll = scratch + area;
    DwtJob *djobs = (DwtJob *)(((uintptr_t)(ll + ll_geom(tc).elems) + 255) & ~(uintptr_t)255);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(tmp, buf, (uint64_t)(x1 - x0) * (y1 - y0) * 4, hipMemcpyDeviceToDevice, s));
    DwtPlan P;
    if (!inverse) dwt_plan_tc(P, tc, tmp, buf, ll, irrev, false);
    else dwt_plan_tc(P, tc, buf, tmp, ll, irrev, true);
    dwt_finalize(P, irrev);
    std::vector<DwtJob> flat;
    for (auto &l : P.levels) flat.insert(flat.end(), l.begin(), l.end());
    if (!flat.empty()) {
        HIPCHK(hipMemcpyAsync(djobs, flat.data(), flat.size() * sizeof(DwtJob), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    for (auto &cpy : P.copies) HIPCHK(hipMemcpyAsync(cpy.dst, cpy.src, cpy.elems * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(dwt_run_levels(P, djobs, irrev, inverse, s));
    return GRKGPU_OK;
}

extern "C" int grkgpu_dwt_fwd(int32_t *buf, int32_t *scratch, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                              uint32_t numres, int32_t irreversible, void *stream) {
    return dwt_common(buf, scratch, x0, y0, x1, y1, numres, irreversible, stream, false);
}

extern "C" int grkgpu_dwt_inv(int32_t *buf, int32_t *scratch, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                              uint32_t numres, int32_t irreversible, void *stream) {
    return dwt_common(buf, scratch, x0, y0, x1, y1, numres, irreversible, stream, true);
}

static_assert(sizeof(grkgpu_enc_block) == sizeof(EncBlock), "EncBlock ABI");
// the device's pass records are read in place as the host's (launch_pass_records)
static_assert(sizeof(DevPass) == sizeof(EncPass) && offsetof(DevPass, dd) == offsetof(EncPass, dd) &&
                  offsetof(DevPass, slope) == offsetof(EncPass, slope) && offsetof(DevPass, term) == offsetof(EncPass, term),
              "DevPass layout");
static_assert(sizeof(grkgpu_enc_result) == sizeof(EncResult), "EncResult ABI");
static_assert(sizeof(grkgpu_dec_block) == sizeof(DecBlock), "DecBlock ABI");

extern "C" int grkgpu_t1_encode_blocks(const grkgpu_enc_block *blocks, uint32_t nblocks, const int32_t *coef,
                                       void *scratch, uint8_t *out, grkgpu_enc_result *results, int with_distortion,
                                       void *stream) {
    return grkgpu_t1_encode_blocks_sty(blocks, nblocks, coef, scratch, out, results, with_distortion, 0, stream);
}

extern "C" int grkgpu_t1_encode_blocks_sty(const grkgpu_enc_block *blocks, uint32_t nblocks, const int32_t *coef,
                                           void *scratch, uint8_t *out, grkgpu_enc_result *results,
                                           int with_distortion, uint32_t cblk_sty, void *stream) {
    if (!blocks || !coef || !scratch || !out || !results) return set_err(GRKGPU_EINVAL, "null argument");
    if (cblk_sty & ~0x3Fu) return set_err(GRKGPU_EINVAL, "code-block style outside 0..63");
    int rc = check_device(-1);
    if (rc) return rc;
    // scratch layout: the encoder's rows for nblocks (rounded up to 64) blocks
    // of 32 planes, then 32 fixed symbol slots per block
    uint8_t *sym = (uint8_t *)scratch + t1e_scratch_bytes(nblocks, 32);
    HIPCHK(launch_t1_encode((const EncBlock *)blocks, nblocks, coef, scratch, sym, nullptr, 32, out,
                            (EncResult *)results, (hipStream_t)stream, cblk_sty));
    if (with_distortion)
        HIPCHK(launch_t1_dist((const EncBlock *)blocks, nblocks, 32, coef, scratch, (EncResult *)results,
                              (hipStream_t)stream));
    return GRKGPU_OK;
}

extern "C" int grkgpu_t1_decode_blocks(const grkgpu_dec_block *blocks, uint32_t nblocks, const uint8_t *data,
                                       void *scratch, int32_t *dst, void *stream) {
    if (!blocks || !data || !scratch || !dst) return set_err(GRKGPU_EINVAL, "null argument");
    int rc = check_device(-1);
    if (rc) return rc;
    // scratch layout: nblocks rounded up to a multiple of 64 T1Scratch
    // records (the decoder's lane-interleaved groups), then one fixed-size
    // unstuffed-stream region per block
    uint32_t *ubuf = (uint32_t *)((uint8_t *)scratch + (size_t)t1_scratch_records(nblocks) * sizeof(T1Scratch));
    HIPCHK(launch_t1_decode((const DecBlock *)blocks, nblocks, data, (T1Scratch *)scratch, dst, (hipStream_t)stream,
                            ubuf, t1_stage_dec_words()));
    return GRKGPU_OK;
}
