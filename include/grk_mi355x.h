/*
 * grk_mi355x.h -- C ABI of the MI355X-native JPEG 2000 hot path
 * (libgrk_mi355x.so).  Plain C types only: no HIP/torch types cross this
 * boundary (streams are passed as void*).
 *
 * What each entry point replaces in the reference (Grok v5.1.0; paths under
 * /root/reference/src/lib/jp2/):
 *
 *   grkgpu_compress        grk_compress's in-library path  grk_setup_encoder +
 *                          grk_start_compress + grk_encode + grk_end_compress
 *                          (grok.h:1660-1748, grok.cpp:545-600 ->
 *                          codestream/j2k.cpp:1609 j2k_setup_encoder,
 *                          :2059 j2k_encode) for the default coding options
 *                          (1 layer, LRCP, 2^15 precincts, cblksty 0).
 *   grkgpu_decompress      grk_read_header + grk_decode (grok.h:1571-1600,
 *                          grok.cpp:381 -> j2k.cpp:1136 j2k_decode_tiles).
 *   grkgpu_read_header     grk_read_header (grok.h:1571, j2k.cpp:406).
 *   (stage entry points below = the tile hot path inside
 *                          TileProcessor::encode_tile (TileProcessor.cpp:
 *                          994-1012: dc_level_shift_encode :1449, mct_encode
 *                          :1473, dwt_encode :1520, t1_encode :1535) and
 *                          decode_tile (:1127-1176).)
 *   grkgpu_dwt_fwd/_inv    Wavelet::encode / Wavelet::decode
 *                          (transform/Wavelet.cpp:35-56, WaveletForward.h:40,
 *                          dwt.cpp:1208 decode_53, :2154 decode_97).
 *   grkgpu_dcshift_mct_fwd mct::encode_rev / encode_irrev + DC shift
 *                          (mct/mct.cpp:85, :195; TileProcessor.cpp:1449).
 *   grkgpu_mct_inv_dcshift mct::decode_rev / decode_irrev + DC shift + clamp
 *                          (mct/mct.cpp:143, :352; TileProcessor.cpp:1377).
 *   grkgpu_decompress_to / grkgpu_mct_inv_dcshift_to
 *                          the same decode, its samples stored as the 8 / 16-bit
 *                          planar or interleaved samples the reference's image
 *                          writers produce from the int32 planes
 *                          (bin/jp2/PNMFormat.cpp, RAWFormat.cpp).
 *   grkgpu_t1_encode_blocks  Tier1::encodeCodeblocks -> T1Encoder::encode ->
 *                          T1Part1::preEncode/encode (t1/Tier1.cpp:24,
 *                          T1Encoder.cpp:40-85, t1_part1/T1Part1.cpp:58-127,
 *                          t1.cpp:1182 t1_encode_cblk).
 *   grkgpu_t1_decode_blocks  Tier1::decodeCodeblocks -> T1Part1::decode +
 *                          postDecode (t1/Tier1.cpp:177, T1Decoder.cpp:43,
 *                          T1Part1.cpp:129-330, t1.cpp:1038 t1_decode_cblk).
 *
 * Error behaviour mirrors the reference: functions return 0 on success and a
 * negative code on failure (the reference returns bool false / nullptr and
 * logs through its error handler); grkgpu_last_error() returns the message.
 * Every function fails loudly (GRKGPU_ENODEV) when no gfx950 device is
 * usable -- there is no CPU fallback.
 */
#ifndef GRK_MI355X_H
#define GRK_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GRKGPU_MAX_COMPS 16

enum {
    GRKGPU_OK = 0,
    GRKGPU_EINVAL = -1,
    GRKGPU_ENODEV = -2,
    GRKGPU_EHIP = -3,
    GRKGPU_EUNSUPPORTED = -4,
    GRKGPU_ECORRUPT = -5
};

/* grk_image subset (grok.h:851-918): planar components.  [x0, x1) x [y0, y1)
 * is the image on the reference grid; component k is subsampled by dx[k],
 * dy[k] (SIZ XRsiz / YRsiz; 0 reads as 1), so its plane covers
 * [ceil(x0 / dx), ceil(x1 / dx)) x [ceil(y0 / dy), ceil(y1 / dy)) -- rows of
 * that width, planes[k] holding only component k (grk_image_comp w, h,
 * TileComponent.cpp:150-163).  A reduced / window decode reports the reduced
 * / window rectangle here, and component planes follow the same rule, except
 * that a reduced decode of the whole image sizes its planes as the reference
 * does (grk_image_comp_header_update, image.cpp:124-155): ceil(size / 2^r),
 * with x1 = x0 + that -- one more row / column than the decoded samples when
 * the origin is not a multiple of 2^r, left zero. */
typedef struct {
    uint32_t x0, y0, x1, y1;
    uint32_t numcomps;
    uint32_t prec[GRKGPU_MAX_COMPS];
    int32_t sgnd[GRKGPU_MAX_COMPS];
    uint32_t dx[GRKGPU_MAX_COMPS], dy[GRKGPU_MAX_COMPS];
} grkgpu_image_desc;

/* One progression-order change (grk_poc, grok.h:393-410; grk_compress -P
 * "T<tile>=resno0,compno0,layno1,resno1,compno1,PROG"). */
typedef struct {
    uint32_t tile;                       /* 1-based tile index the entry applies to */
    uint32_t resno0, compno0, layno1, resno1, compno1;
    int32_t prog;                        /* GRKGPU_LRCP .. GRKGPU_CPRL */
} grkgpu_poc;

enum { GRKGPU_LRCP = 0, GRKGPU_RLCP = 1, GRKGPU_RPCL = 2, GRKGPU_PCRL = 3, GRKGPU_CPRL = 4 };
#define GRKGPU_CSTY_PRT 0x01 /* user precinct sizes (grk_compress -c) */
#define GRKGPU_CSTY_SOP 0x02 /* SOP marker before each packet (-SOP) */
#define GRKGPU_CSTY_EPH 0x04 /* EPH marker after each packet header (-EPH) */
#define GRKGPU_PROFILE_CINEMA_2K 0x0003 /* grok.h:160 */
#define GRKGPU_PROFILE_CINEMA_4K 0x0004 /* grok.h:161 */

/* grk_cparameters subset (grok.h:447-570); field meaning as there */
typedef struct {
    uint32_t numresolution;                /* default 6 */
    uint32_t cblockw_init, cblockh_init;   /* default 64, 64 (powers of 2, <= 64) */
    int32_t irreversible;                  /* 0: 5/3, 1: 9/7 (-I) */
    int32_t tcp_mct;                       /* -1: auto (RGB->YCC iff >= 3 comps), 0, 1; 2: the custom
                                              matrix below (grkgpu_set_mct) */
    int32_t tile_size_on;
    uint32_t cp_tdx, cp_tdy, cp_tx0, cp_ty0;
    /* quality layers and rate control (grk_compress -r / -q / -A) */
    uint32_t tcp_numlayers;                /* 0: one lossless layer */
    double tcp_rates[100];                 /* per layer compression ratio, decreasing; 0 = lossless */
    double tcp_distoratio[100];            /* per layer PSNR (fixed quality) */
    int32_t cp_disto_alloc, cp_fixed_quality;
    int32_t rate_control_algorithm;        /* 0: bisect all passes, 1: feasible truncation points */
    /* coding style, precincts, progression (-c, -SOP, -EPH, -p, -P, -u) */
    uint32_t csty;                         /* GRKGPU_CSTY_* */
    uint32_t res_spec;                     /* precinct sizes given, highest resolution first */
    uint32_t prcw_init[33], prch_init[33];
    int32_t prog_order;                    /* GRKGPU_LRCP .. */
    uint32_t numpocs;
    grkgpu_poc POC[32];
    int32_t tp_on;                         /* tile-parts: one per change of tp_flag's dimension */
    int32_t tp_flag;                       /* 'R', 'L', 'C' */
    /* profiles (-cinema2K / -cinema4K fps): rsiz + the size caps */
    uint32_t rsiz;
    uint32_t framerate;
    uint64_t max_cs_size, max_comp_size;
    /* code-block style (-M): 0x01 BYPASS (lazy), 0x02 RESET, 0x04 TERMALL
     * (restart), 0x08 VSC, 0x10 PTERM (ERTERM), 0x20 SEGSYM */
    uint32_t cblk_sty;
    /* ROI up-shift (-ROI c=compno,U=shift; the RGN marker): roi_shift 0 = none */
    int32_t roi_compno;
    uint32_t roi_shift;
    uint32_t pad_;
    /* custom (Part 2 array-based) MCT, grk_set_MCT's mct_data: mct_ncomp x
     * mct_ncomp encoding matrix (row-major) and per-component DC shifts;
     * mct_ncomp 0 = none */
    uint32_t mct_ncomp;
    float mct_matrix[GRKGPU_MAX_COMPS * GRKGPU_MAX_COMPS];
    int32_t mct_dc_shift[GRKGPU_MAX_COMPS];
} grkgpu_cparams;

typedef struct grkgpu_ctx grkgpu_ctx;

/* Per-stage timings of the last call (device time from HIP events, ms). */
typedef struct {
    float h2d_ms, dcshift_mct_ms, dwt_ms, t1_ms, gather_ms, d2h_ms, host_t2_ms, total_ms;
    uint64_t num_cblks, cs_bytes;
    uint64_t mq_symbols;  /* MQ symbols coded (encode) */
    float rate_ms;        /* host rate allocation (PCRD) time (summed over tiles) */
    float packet_ms;      /* host packet / tile-part writing time (summed over tiles) */
    /* the PCRD bisection, summed over tiles: probes (thresholds tried), those
     * decided by their code-block bytes alone (no packet simulation), block
     * evaluations, precinct simulations, and the time forming layers /
     * simulating packets (part of rate_ms) */
    uint32_t rate_probes, rate_probes_skipped;
    uint64_t rate_block_evals, rate_precinct_sims;
    float rate_form_ms, rate_sim_ms;
    float passrec_ms;     /* host: per-pass rate / distortion records from the T1 results (part of host_t2_ms) */
    uint32_t pad_;
} grkgpu_stats;

/* One kernel launch of the last call's forward DWT, timed with HIP events on
 * the context's stream (grkgpu_set_launch_timing): kernel name, first level
 * and level count it computes, device time, and its algorithmic bytes
 * (8 B -- an int32 read and written -- per sample of every level it
 * computes: SURVEY.md 8(d)'s B_DWT split per launch). */
typedef struct {
    char kernel[48];
    uint32_t level0, levels;
    float ms;
    uint32_t pad;
    uint64_t bytes;
} grkgpu_launch_time;

const char *grkgpu_version(void);
const char *grkgpu_last_error(void);
int grkgpu_device_count(void);

int grkgpu_create(int device, grkgpu_ctx **out);
void grkgpu_destroy(grkgpu_ctx *ctx);
/* Order all work of ctx after/with this HIP stream (hipStream_t as void*). */
int grkgpu_set_stream(grkgpu_ctx *ctx, void *stream);
int grkgpu_get_stats(grkgpu_ctx *ctx, grkgpu_stats *out);
/* Time every DWT launch of later compress (forward) and decompress (inverse)
 * calls (off by default: two events per launch), and read the launches of the
 * last call: *n = their count, the first min(max, *n) are copied to out. */
int grkgpu_set_launch_timing(grkgpu_ctx *ctx, int on);

/* DWT plan options, process-wide (later calls; not while other threads are
 * inside a call).  The defaults are the plans measured fastest on the MI355X
 * (DESIGN.md 3); the others stay selectable so the parity suite can check
 * every kernel the library carries.
 *   fuse_level0      -1 (default): the DC shift + RCT of a 3-component 5/3
 *                    tile runs inside DWT level 0 (k_dwt_fwd_mct3); 0: never
 *                    (separate k_dcshift_mct_fwd pass); 1: always (also 9/7
 *                    and single components: DC shift in level 0's loads).
 *   f01_rows         9/7 levels 0 + 1 in one launch (k_dwt_fwd01) with 2 / 4
 *                    (default) / 6 level-0 row windows per workgroup; 0: one
 *                    launch per level.
 *   f01_min_samples  fuse a level pair only from this many level-l samples
 *                    (default 2^23; 0: every qualifying pair).
 *   f01_small_min_samples  fuse smaller pairs too, from this many samples,
 *                    with 2 row windows per workgroup (default all ones:
 *                    never -- the 8K frame's levels 2 + 3 fused this way
 *                    took 26 us of kernel time against 14 + 7 apart).
 *   inv01            2 (default) / 4: the two largest inverse levels in one
 *                    launch (k_dwt_inv01, with 2 / 4 row windows for the
 *                    smaller level per workgroup) when the larger has at
 *                    least inv01_min_samples samples (default 2^23; 0: any
 *                    size); 0: one launch per level.
 *   pair_group       workgroup order of the fused level pairs (k_dwt_fwd01,
 *                    k_dwt_inv01): 0 (default) row-major; G > 0: groups of G
 *                    workgroup columns, each walked top to bottom.
 *   f64_lift         forward 9/7 lifting arithmetic (fused pair and per-level
 *                    kernel, not the fused DC-shift loads): 0 the
 *                    64-bit integer multiply (v_mad_i64_i32), 1 f64 FMA +
 *                    floor (bit-identical results).
 *   t1_dec_sort      T1 decode: 1 (default) = code-blocks handed to the
 *                    lanes in decreasing order of expected work (passes,
 *                    bytes), so a wavefront's lanes finish close together;
 *                    0 = stream order; -1 = only for a call that is the only
 *                    one in progress in the process.  Same output.
 *   t1_dec_bpw       T1 decode: code-blocks per wavefront (1, 2, 4 .. 64);
 *                    0 (default) = a lone call spreads its blocks to give
 *                    every SIMD 1.5 wavefronts, concurrent calls pack 64 (from
 *                    4096 blocks).
 *   mid_th           window rows (8, 16, 24) of the per-level DWT kernels for
 *                    a level of 2^21 .. 2^23 samples; 0 (default) = 8.
 *   t1_enc_bpw       T1 encode (MQ coder): code-blocks per wavefront, as
 *                    t1_dec_bpw.
 *   t1_enc_sort      T1 encode: 1 = the MQ coder's lanes take the code-blocks
 *                    in decreasing order of their symbol count (a counting
 *                    sort on the device after the modelling kernel); 0
 *                    (default, measured as fast) = block order.  Same
 *                    codestream.
 *   pair_kernel      fused forward level pairs: k_dwt_fwd_pair (workgroups
 *                    stream column strips top to bottom, the vertical lifting
 *                    carried in registers, the LL rows through an LDS ring)
 *                    for pairs of at least pair_min_samples level-l samples
 *                    (default 2^20) -- 1 (default): 5/3 pairs, 9/7 pairs by
 *                    k_dwt_fwd01's windows (f01_rows); 2: both wavelets
 *                    streamed; 0: no 5/3 pairs, 9/7 by k_dwt_fwd01.
 *                    f01_rows = 0 turns every fused pair off.
 *   pair_rows        k_dwt_fwd_pair: level-(l+1) rows per segment (even); 0
 *                    (default) = sized for one resident wave of workgroups.
 *   pair_waves       k_dwt_fwd_pair: level-l wavefronts per workgroup, 3 or 4;
 *                    0 (default) = whichever wastes fewer columns.
 *   t1_lone          which T1 plan a call takes: 0 (default) = by the calls in
 *                    progress in the process (a call that is alone spreads
 *                    its code-blocks over the chip, concurrent calls pack
 *                    full wavefronts); 1 = every call takes the lone plan;
 *                    -1 = every call takes the batch plan (the wide MQ coder
 *                    and the lane-per-block unstuff from 4096 blocks), so
 *                    the parity suite reaches the batch kernels without
 *                    overlapping calls.  Same output. */
typedef struct {
    int32_t fuse_level0;
    int32_t f01_rows;
    uint64_t f01_min_samples;
    uint64_t f01_small_min_samples;
    int32_t inv01;
    int32_t pair_group;
    uint64_t inv01_min_samples;
    int32_t f64_lift;
    int32_t t1_dec_sort;
    int32_t t1_dec_bpw;
    int32_t mid_th;
    int32_t t1_enc_bpw;
    int32_t t1_enc_sort;
    int32_t pair_kernel;
    int32_t pair_rows;
    int32_t pair_waves;
    uint64_t pair_min_samples;
    int32_t t1_lone;
    int32_t pad_;
} grkgpu_dwt_options;
void grkgpu_get_dwt_options(grkgpu_dwt_options *out);  /* current values */
int grkgpu_set_dwt_options(const grkgpu_dwt_options *opts);  /* NULL: the defaults */
int grkgpu_get_launch_times(grkgpu_ctx *ctx, grkgpu_launch_time *out, uint32_t max, uint32_t *n);
void grkgpu_default_cparams(grkgpu_cparams *p);
/* grk_set_MCT (grok.cpp:606-630): a custom array-based MCT -- rsiz gains the
 * Part-2 MCT extension (0x8000 | 0x0100), 9/7, tcp_mct = 2, the n x n
 * encoding matrix (row-major, applied in 13-bit fixed point,
 * mct.cpp:429-475) and the per-component DC shifts.  The codestream then
 * carries its inverse (float, j2k.cpp:1932) in CBD / MCT / MCC / MCO marker
 * segments (j2k.cpp:5615-6333). */
int grkgpu_set_mct(grkgpu_cparams *p, const float *matrix, const int32_t *dc_shift, uint32_t n);

/* Whole-codestream encode.  planes[c] = (y1-y0)*(x1-x0) int32 samples, on
 * the device when planes_on_device != 0, else host memory.  The .j2k
 * codestream is returned in *out (free with grkgpu_free). */
int grkgpu_compress(grkgpu_ctx *ctx, const grkgpu_image_desc *img, const grkgpu_cparams *p,
                    const int32_t *const *planes, int planes_on_device, uint8_t **out, size_t *outlen);

/* Same, zero-copy: *out points into the context's pinned output buffer and
 * stays valid until the next call on ctx (like the reference's memory stream). */
int grkgpu_compress_view(grkgpu_ctx *ctx, const grkgpu_image_desc *img, const grkgpu_cparams *p,
                         const int32_t *const *planes, int planes_on_device, const uint8_t **out, size_t *outlen);

/* Output-buffer hand-off for views that must outlive later calls: take the
 * context's pinned output buffer (holding the last compress's codestream) out
 * of the context -- its next compress allocates a buffer of its own -- and
 * give a taken buffer back when done with it (the context keeps the larger of
 * it and its current buffer and frees the other; with ctx = NULL, or after
 * grkgpu_destroy, use grkgpu_free_output).  *buf = NULL if the context holds
 * no buffer. */
int grkgpu_take_output(grkgpu_ctx *ctx, void **buf, size_t *cap);
int grkgpu_give_output(grkgpu_ctx *ctx, void *buf, size_t cap);
void grkgpu_free_output(void *buf);

/* Test hook: after synchronising the context's stream, set every byte of every
 * device and pinned host buffer the context owns (their whole capacity) to
 * `byte`, and every kept host record (enc_passes, bexp*, ltimes) to that
 * pattern or empty.  Views and pointers returned by earlier calls on the
 * context are invalid afterwards.  Buffers taken with grkgpu_take_output are
 * the caller's and are not touched.  Returns the number of bytes filled in
 * *filled (may be NULL).  The next call on the context must give the result
 * it gives on a fresh one: no call may read what it has not written. */
int grkgpu_debug_fill(grkgpu_ctx *ctx, int byte, size_t *filled);

/* Tile shards (multi-GPU): tiles are independent through the
 * whole path, and a codestream is [main header][tile-parts in tile order]
 * [EOC] (j2k.cpp:2088-2111, 2376-2435), so each GPU encodes a contiguous
 * tile range and the host concatenates.  grkgpu_compress_tiles encodes tiles
 * [tile_begin, tile_end) and emits the parts selected by `parts`;
 * grkgpu_compress == grkgpu_compress_tiles(0, n, GRKGPU_PART_ALL). */
#define GRKGPU_PART_HEADER 1u
#define GRKGPU_PART_TILES 0u
#define GRKGPU_PART_EOC 2u
#define GRKGPU_PART_ALL 3u
int grkgpu_num_tiles(const grkgpu_image_desc *img, const grkgpu_cparams *p, uint32_t *ntiles);
int grkgpu_compress_tiles(grkgpu_ctx *ctx, const grkgpu_image_desc *img, const grkgpu_cparams *p,
                          const int32_t *const *planes, int planes_on_device, uint32_t tile_begin,
                          uint32_t tile_end, uint32_t parts, uint8_t **out, size_t *outlen);

/* Multi-device calls: one call shards the tiles over several devices
 *  -- what the reference's callers ask for with
 * deviceId = -1 (grk_cparameters.deviceId, grok.h:565; grk_compress -G "A
 * value of -1 will specify all devices", grk_compress.cpp:423-426; the
 * decompress parameters and the plugin init info carry the same field,
 * grok.h:789, 1817).  A device set lists the workers: one host thread and
 * one context (pooled per device across calls) each; a device may appear
 * more than once.
 *   grkgpu_device_set_for: device >= 0 -> {device}; device = -1 -> the
 *     environment's GRKGPU_DEVICES ("0,1,2,3", "0,0", or "all"), else every
 *     visible device.
 *   grkgpu_compress_multi: the whole codestream.  Worker k encodes the k-th
 *     contiguous tile range from just the image rows of its tiles (host
 *     planes; worker 0 also writes the main header, the last one the EOC);
 *     the pieces are concatenated in tile order and the TLM records filled in
 *     from the tile-parts (j2k_write_updated_tlm, j2k.cpp:2555-2577).  Bytes
 *     identical to grkgpu_compress.  One worker does it all when the image
 *     has one tile, the planes are on a device, hold a window of the image,
 *     or a component is subsampled.  *out: free with grkgpu_free.
 *   grkgpu_decompress_multi: whole-image decode into host planes, each worker
 *     decoding its tile range (grkgpu_decompress_tiles).
 *   grkgpu_multi_release: destroy the pooled contexts. */
#define GRKGPU_MAX_DEVICES 64
typedef struct {
    uint32_t n;
    int32_t dev[GRKGPU_MAX_DEVICES];
} grkgpu_device_set;
int grkgpu_device_set_for(int device, grkgpu_device_set *out);
void grkgpu_multi_release(void);
/* Host only: fill in the TLM records of a codestream concatenated from tile
 * shards (j2k_write_updated_tlm, j2k.cpp:2555-2577) from its tile-parts' SOT
 * headers, in place -- records across all of the main header's TLM markers,
 * in order.  GRKGPU_EINVAL when the records do not match the tile-parts one
 * to one (or a tile-part has Psot = 0); a stream without TLM is unchanged. */
int grkgpu_patch_tlm(uint8_t *cs, size_t len);

/* Same, with planes holding only image rows [row0, row0 + nrows) (relative to
 * img->y0): a rank of a tile-row shard loads just the rows of its tiles.
 * Every tile of [tile_begin, tile_end) must lie inside those rows. */
int grkgpu_compress_tile_rows(grkgpu_ctx *ctx, const grkgpu_image_desc *img, const grkgpu_cparams *p,
                              const int32_t *const *planes, int planes_on_device, uint32_t row0, uint32_t nrows,
                              uint32_t tile_begin, uint32_t tile_end, uint32_t parts, uint8_t **out, size_t *outlen);

/* The general encode entry point: image samples in the width the image file
 * holds them (grk_image's planes are int32, grok.h:851-918; the PGM / PPM /
 * raw files grk_compress and the plugin read are 1 or 2 bytes per sample,
 * PNMFormat.cpp), widened to int32 on the GPU by the kernel that first reads
 * them -- so a 12-bit frame crosses PCIe as 2 B/sample.  planes[c] holds
 * rows [row0, row0 + nrows) x columns [col0, col0 + ncols) of component c
 * (nrows / ncols = 0: every row / column; a tile-row shard gives only its
 * tiles' rows, see grkgpu_compress_tile_rows; grk_write_tile one tile), on
 * the device when on_device != 0.  Every tile encoded must lie inside them.  Encodes tiles [tile_begin, tile_end) and
 * emits the parts `parts` selects (GRKGPU_PART_*; 0, 0xffffffff, ALL = the
 * whole codestream, as grkgpu_compress).  *out points into the context's
 * pinned output buffer, valid until the next call on ctx (as
 * grkgpu_compress_view).  A sample format must hold the component's
 * precision and signedness (U16: unsigned, prec <= 16), else GRKGPU_EINVAL.
 *
 * sample_fmt = a GRKGPU_SAMPLE_* width in its low byte, or'ed with flags (the
 * struct keeps its size and offsets; a plain width means what it always has):
 *   GRKGPU_SAMPLE_INTERLEAVED  planes[0] holds pixels, as image loaders, video
 *     capture and the PPM raster hold them (PNMFormat.cpp reads "P6" so):
 *     sample (y, x, c) of the rows and columns held is at
 *     planes[0][((y - row0) * ncols + (x - col0)) * numcomps + c], rows tight
 *     (ncols * numcomps samples); planes[1..] are not read.  Every component
 *     must be on one grid (equal dx, equal dy), else GRKGPU_EUNSUPPORTED --
 *     grkgpu_decompress_to's rule for interleaved output.
 *   GRKGPU_SAMPLE_BIG_ENDIAN   16-bit samples stored most-significant byte
 *     first, as the 16-bit PGM / PPM raster is; with U16 / I16 only, planar or
 *     interleaved (any other width: GRKGPU_EINVAL).  The swap is one permute
 *     per dword in the kernel that first reads the samples.
 * Unknown flag bits: GRKGPU_EINVAL.  All of this is checked before the context
 * or a device is touched.  The codestream does not depend on the format or
 * layout the samples arrive in. */
enum {
    GRKGPU_SAMPLE_I32 = 0, /* int32_t (grk_image) */
    GRKGPU_SAMPLE_U8 = 1,
    GRKGPU_SAMPLE_I8 = 2,
    GRKGPU_SAMPLE_U16 = 3,
    GRKGPU_SAMPLE_I16 = 4
};
#define GRKGPU_SAMPLE_INTERLEAVED 0x100u
#define GRKGPU_SAMPLE_BIG_ENDIAN 0x200u
typedef struct {
    const void *planes[GRKGPU_MAX_COMPS]; /* planar: one per component; interleaved: planes[0] */
    uint32_t sample_fmt;  /* GRKGPU_SAMPLE_* | GRKGPU_SAMPLE_INTERLEAVED | GRKGPU_SAMPLE_BIG_ENDIAN */
    int32_t on_device;
    uint32_t row0, nrows; /* rows held (relative to y0); nrows = 0: every row */
    uint32_t col0, ncols; /* columns held (relative to x0), = the row stride; ncols = 0: every column
                             (grk_write_tile hands one tile's samples: its rows and columns only) */
} grkgpu_planes;
int grkgpu_compress_ex(grkgpu_ctx *ctx, const grkgpu_image_desc *img, const grkgpu_cparams *p,
                       const grkgpu_planes *planes, uint32_t tile_begin, uint32_t tile_end, uint32_t parts,
                       const uint8_t **out, size_t *outlen);
/* (multi-device encode: see grkgpu_device_set above) */
int grkgpu_compress_multi(const grkgpu_device_set *devs, const grkgpu_image_desc *img, const grkgpu_cparams *p,
                          const grkgpu_planes *planes, uint8_t **out, size_t *outlen);

/* Tier-1 only (the tile hot path of TileProcessor::encode_tile up to and
 * including t1_encode, TileProcessor.cpp:994-1012; SURVEY 8(b)
 * "grkgpu_encode_tile"): DC shift + MCT + DWT + T1 of every tile on the GPU,
 * results handed back per code-block in the reference's order (tile,
 * component, resolution, band, precinct, code-block) so a host Tier-2 -- the
 * reference's own, through its plugin interface -- can finish the
 * codestream.  Rates are the cumulative pass rates after the reference's
 * fix-ups (t1.cpp:1299-1325); distortion the cumulative distortion decrease
 * (t1.cpp:1249-1254), computed when with_distortion != 0.  Pointers stay
 * valid until the next call on ctx. */
typedef struct {
    uint32_t tileno, compno, resno, bandno, precno, cblkno;
    uint32_t x0, y0, x1, y1;             /* code-block rectangle, band coordinates */
    uint32_t numbps, numpasses, len;
    float stepsize;                      /* the band's encoder step size (Quantizer.cpp:65-104) */
    const uint8_t *data;                 /* len MQ bytes */
    const uint32_t *rate;                /* numpasses cumulative rates */
    const double *distortion;            /* numpasses cumulative distortion decrease */
} grkgpu_block_info;
int grkgpu_encode_blocks(grkgpu_ctx *ctx, const grkgpu_image_desc *img, const grkgpu_cparams *p,
                         const int32_t *const *planes, int planes_on_device, int with_distortion,
                         const grkgpu_block_info **blocks, uint32_t *nblocks);
/* The same from a grkgpu_planes: the samples at the file's width, planar or
 * interleaved, host byte order or big-endian (what the plugin hands over: the
 * PGM / PPM raster as it stands in the file).  Every tile is encoded, so the
 * planes hold the whole image.  grkgpu_encode_blocks forwards here. */
int grkgpu_encode_blocks_ex(grkgpu_ctx *ctx, const grkgpu_image_desc *img, const grkgpu_cparams *p,
                            const grkgpu_planes *planes, int with_distortion, const grkgpu_block_info **blocks,
                            uint32_t *nblocks);

/* After grkgpu_encode_blocks on ctx (and before any other call on it): the
 * forward DWT output of one tile-component -- the reference's tile buffer
 * after dwt_encode (Mallat layout, dwt_utils.cpp:84-127), rows of the
 * tile-component's width, before T1's quantisation -- copied into dst (host
 * memory, h rows of dst_stride elements).  This is what the reference's plugin
 * debug state hands its host as image data so that both T1s start from the
 * same coefficients (TileProcessor.cpp:985-1012, grok.h:1790-1808). */
int grkgpu_encode_blocks_coefficients(grkgpu_ctx *ctx, uint32_t tileno, uint32_t compno, int32_t *dst,
                                      uint32_t dst_stride);

/* Parse the main header only. */
int grkgpu_read_header(const uint8_t *cs, size_t len, grkgpu_image_desc *img);
/* The coding parameters of the main header (grk_header_info, grok.h:620-689),
 * plus its quantisation (QCD: Sqcd guard bits and style, the step sizes as
 * read) and ROI shifts (RGN) -- what grk_get_cstr_info reports. */
typedef struct {
    uint32_t cblockw_init, cblockh_init, irreversible, mct, rsiz, numresolutions, csty, cblk_sty;
    uint32_t prcw_init[33], prch_init[33];  /* precinct size per resolution (samples) */
    uint32_t tx0, ty0, tdx, tdy, tw, th;   /* tile grid */
    uint32_t numlayers, prog;
    uint32_t numcomps, numgbits, qntsty, nsteps;  /* QCD: guard bits, style, step sizes read */
    uint32_t step_expn[97], step_mant[97];
    uint32_t roishift[16];                 /* RGN per component */
} grkgpu_header_info;
int grkgpu_read_header_info(const uint8_t *cs, size_t len, grkgpu_header_info *info);
/* One component's coding style and quantisation as the main header sets them
 * (COD / QCD, or that component's COC / QCC; the reference's default tcp
 * tccps[compno], j2k_dump.cpp:357-390 reads the same): precinct flag, levels,
 * log2 code-block size, mode switches, wavelet (qmfbid 1 = 5/3), log2
 * precinct sizes, QCD / QCC style, guard bits and step sizes, ROI shift. */
typedef struct {
    uint32_t csty, numresolutions, cblkw, cblkh, cblk_sty, qmfbid;
    uint32_t prcw[33], prch[33];
    uint32_t qntsty, numgbits, nsteps;
    uint32_t step_expn[100], step_mant[100];
    uint32_t roishift;
} grkgpu_comp_info;
int grkgpu_read_comp_info(const uint8_t *cs, size_t len, uint32_t compno, grkgpu_comp_info *info);

/* Whole-codestream decode into caller-provided planes (device or host). */
int grkgpu_decompress(grkgpu_ctx *ctx, const uint8_t *cs, size_t len, grkgpu_image_desc *img,
                      int32_t *const *planes, int planes_on_device);
/* Reduced-resolution decode (grk_decompress -r; grk_decompress_parameters
 * cp_reduce, grok.h:698-702, applied in j2k.cpp:1464-1476 and
 * TileComponent.cpp:199-204): the image at resolution numres-1-reduce, the
 * samples from ceil(x0 / 2^reduce), planes of ceil(size / 2^reduce) a side
 * (see grkgpu_image_desc); img (if given) receives the reduced geometry.
 * reduce must be < the number of resolutions (GRKGPU_EINVAL). */
int grkgpu_decompress_reduced(grkgpu_ctx *ctx, const uint8_t *cs, size_t len, uint32_t reduce,
                              grkgpu_image_desc *img, int32_t *const *planes, int planes_on_device);
/* Window decode (grk_set_decode_area, grok.h:1587; grk_decompress -d):
 * decode only the samples of [x0, x1) x [y0, y1) (image coordinates, clipped
 * to the image) into planes of the window's size; img (if given) receives the
 * window geometry.  Same samples as a full decode, cropped.  Only the tiles
 * meeting the window and the code-blocks reaching it are decoded. */
int grkgpu_decompress_window(grkgpu_ctx *ctx, const uint8_t *cs, size_t len, uint32_t x0, uint32_t y0, uint32_t x1,
                             uint32_t y1, grkgpu_image_desc *img, int32_t *const *planes, int planes_on_device);
/* Decode with grk_decompress's options (grk_dparameters, grok.h:694-735):
 * cp_reduce (-r), cp_layer (-l, 0 = all layers) and the decode area (-d,
 * grk_set_decode_area; all four 0 = the whole image).  A window at a reduced
 * resolution spans ceil(x1 / 2^r) - ceil(x0 / 2^r) (update_image_dimensions,
 * image.cpp:207-246).  img (if given) receives the decoded geometry. */
typedef struct {
    uint32_t cp_reduce, cp_layer;
    uint32_t DA_x0, DA_y0, DA_x1, DA_y1;
} grkgpu_dparams;
int grkgpu_decompress_ex(grkgpu_ctx *ctx, const uint8_t *cs, size_t len, const grkgpu_dparams *p,
                         grkgpu_image_desc *img, int32_t *const *planes, int planes_on_device);
/* Decode only tiles [tile_begin, tile_end) (a tile shard; the reference's
 * tile-by-tile decode, grk_decode_tile_data / j2k.cpp decode_tiles); the
 * other tiles' samples in planes are left untouched.  Host planes are written
 * for the shard's tiles only. */
int grkgpu_decompress_tiles(grkgpu_ctx *ctx, const uint8_t *cs, size_t len, uint32_t tile_begin,
                            uint32_t tile_end, int32_t *const *planes, int planes_on_device);
/* Decode straight to the samples a consumer holds: 8 / 16-bit (or int32)
 * samples, planar or pixel-interleaved -- the decode-side counterpart of
 * grkgpu_planes.  The reference decodes to grk_image's int32 planes and leaves
 * the narrowing to whoever writes the file: its PNM / raw writers walk the
 * planes and emit 1 or 2 bytes per sample, interleaving the components as
 * they go (PNMFormat.cpp, RAWFormat.cpp encode paths).  Here the last decode
 * kernel (inverse MCT + DC shift + clamp) stores the samples in that form, so
 * a 12-bit frame leaves the GPU at 2 B/sample.  The clamp to the component's
 * [min, max] comes first and sample_fmt must hold every component's
 * precision and signedness (grkgpu_compress_ex's rule, else GRKGPU_EINVAL),
 * so the narrowing is exact -- the values are those of the int32 decode.
 * Rows are tight: w samples (planar), w * numcomps samples (interleaved:
 * sample (y, x, c) at planes[0][(y * w + x) * numcomps + c]).  Interleaved
 * output needs every component on one grid (subsampled components on
 * different grids: GRKGPU_EUNSUPPORTED; planar output takes them, each plane
 * on its own grid).  Geometry as grkgpu_decompress_ex, the reduced whole
 * image's zero margin included.
 * p = NULL: whole image, all layers.  tile_begin / tile_end = 0, 0xffffffff:
 * every tile; a proper range has grkgpu_decompress_tiles' rules (no reduce /
 * window, the other tiles' samples untouched).
 *
 * layout | GRKGPU_LAYOUT_UPSAMPLE (grk_decompress -u, upsample_image_components,
 * grk_decompress.cpp:891-1040): every subsampled component is replicated to
 * the image grid by the store of the last decode kernel, so a 4:2:0 / 4:2:2
 * stream decodes to full-size planes or to (y, x, c) pixels of numcomps
 * samples (the one-grid rule above no longer applies).  With O = [ox0, ox1) x
 * [oy0, oy1) the image, or the decode window clipped to it, and P_k the plane
 * component k (dx, dy) decodes to without the flag, the sample at (X, Y) in O
 * is P_k[floor(Y / dy) - ceil(oy0 / dy)][floor(X / dx) - ceil(ox0 / dx)], or 0
 * where an index is negative (an origin that is no multiple of dx / dy: the
 * reference's zero lead-in).  Components all subsampled alike are expanded
 * after their inverse MCT.  Every sample format, host or device planes, window
 * and cp_layer; cp_reduce > 0 on a stream with a subsampled component is
 * GRKGPU_EINVAL (the reference refuses -u with -r), a proper tile range stays
 * GRKGPU_EUNSUPPORTED.  img receives O with dx = dy = 1.  On a stream without
 * subsampled components the flag changes nothing. */
enum { GRKGPU_LAYOUT_PLANAR = 0, GRKGPU_LAYOUT_INTERLEAVED = 1 };
#define GRKGPU_LAYOUT_UPSAMPLE 0x100u
typedef struct {
    void *planes[GRKGPU_MAX_COMPS]; /* planar: one per component; interleaved: planes[0] */
    uint32_t sample_fmt;            /* GRKGPU_SAMPLE_* */
    uint32_t layout;                /* GRKGPU_LAYOUT_* | GRKGPU_LAYOUT_UPSAMPLE */
    int32_t on_device;
    uint32_t pad_;
} grkgpu_out_planes;
int grkgpu_decompress_to(grkgpu_ctx *ctx, const uint8_t *cs, size_t len, const grkgpu_dparams *p,
                         uint32_t tile_begin, uint32_t tile_end, grkgpu_image_desc *img,
                         const grkgpu_out_planes *out);
/* grkgpu_decompress_to with the two remaining per-sample steps of
 * grk_decompress between the decode and displayable pixels, done by the store
 * of the last decode kernel on the values it holds in registers -- in the
 * reference's order colour -> precision, on the upsampled samples
 * (precision(colour(upsample(decode))): the reference's sYCC routines
 * replicate the chroma themselves, and replication commutes with a per-sample
 * map).  Let U_k(X, Y) be the GRKGPU_LAYOUT_UPSAMPLE value above (zero where
 * an index is negative, the identity for a component at (1,1)).
 *
 * colour = GRKGPU_COLOUR_SYCC (grk_decompress.cpp:1585-1609 ->
 * color_sycc_to_rgb, bin/common/color.cpp:136-418): exactly 3 components, all
 * unsigned and of one precision P, component 0 at (1,1), components 1 and 2
 * both at (1,1), both at (2,1) or both at (2,2); anything else is
 * GRKGPU_EINVAL.  It implies GRKGPU_LAYOUT_UPSAMPLE.  Per pixel, with
 * off = 2^(P-1), upb = 2^P - 1, y = U_0, cb = U_1 - off, cr = U_2 - off:
 *   R = clamp(y + trunc(1.402 * cr), 0, upb)
 *   G = clamp(y - trunc(0.344 * cb + 0.714 * cr), 0, upb)
 *   B = clamp(y + trunc(1.772 * cb), 0, upb)
 * in IEEE double, every product and the sum rounded on its own (no FMA), the
 * conversion to int32 truncating.  A zero lead-in chroma sample enters as raw
 * 0 (cb = -off), as in the reference.  Equal to sycc444_to_rgb / sycc422_to_rgb
 * at any origin and to sycc420_to_rgb at any origin with even x.  The one
 * deviation: 4:2:0 with an odd x origin, where the reference's loop disagrees
 * with its own 4:2:2 loop and with -u (the second row of each row pair takes
 * cb[0] for the first column, the tail row ignores the offset) -- this keeps
 * the upsample rule.
 *
 * prec = p in 1 .. 16 (grk_decompress -p, grk_decompress.cpp:1690-1716;
 * clip_component / scale_component, bin/jp2/convert.cpp:82-161), applied after
 * the colour step to every component, q its own precision:
 *   clip,  unsigned         min(v, 2^p - 1)
 *   clip,  signed           clamp(v, -2^(p-1), 2^(p-1) - 1)
 *   scale, p == q           v
 *   scale, p < q            v >> (q - p)  (signed: arithmetic)
 *   scale, p > q, unsigned  (v * (2^p - 1)) / (2^q - 1), integer division
 *   scale, p > q, signed    v * 2^(p-q)
 * prec = 0 keeps each component's precision.
 *
 * out->sample_fmt must hold the OUTPUT precision (prec, or the component's own
 * when prec = 0) and signedness of every component, else GRKGPU_EINVAL -- so a
 * 12-bit stream decodes to U8 with prec = 8.  img receives the output
 * precision, and dx = dy = 1 with SYCC.  ops = NULL or all zero:
 * grkgpu_decompress_to, launch for launch.  Unknown colour / prec_mode, prec >
 * 16, reserved != 0 or a format narrower than prec: GRKGPU_EINVAL before any
 * device call.  Window, cp_layer, host or device planes, both layouts and
 * every sample format as grkgpu_decompress_to; cp_reduce > 0 where no
 * component is subsampled (with SYCC or the upsample flag on a subsampled
 * stream: GRKGPU_EINVAL, as there); a proper tile range keeps its rules.
 * Precision alone on a subsampled stream without the upsample flag converts
 * each plane on its own grid.  Samples nothing decoded (the zero margin of a
 * reduced decode at an odd origin, tiles a cut stream never reached) are
 * converted like any other, as the reference's colour step does with them:
 * with SYCC they come out as the conversion of (0, 0, 0).
 *
 * The other per-sample colour steps of grk_decompress (grk_decompress.cpp:
 * 1585-1749: colour -> precision -> upsample -> force-RGB; computed here as
 * forcergb(precision(colour(upsample(decode)))), replication commuting with a
 * per-sample map) sit in the same store.  Neither implies the upsample flag:
 * components all subsampled alike stay on their grid without it.
 *
 * colour = GRKGPU_COLOUR_EYCC (color_esycc_to_rgb, bin/common/color.cpp:936-995):
 * exactly 3 components on one grid, one precision P in 1 .. 16, component 0
 * unsigned; anything else is GRKGPU_EINVAL.  With flip = 2^(P-1),
 * max = 2^P - 1, y = U_0, cb = U_1 - (sgnd_1 ? 0 : flip),
 * cr = U_2 - (sgnd_2 ? 0 : flip):
 *   R = clamp(trunc(((y - 0.0000368 * cb) + 1.40199 * cr) + 0.5), 0, max)
 *   G = clamp(trunc(((1.0003 * y - 0.344125 * cb) - 0.7141128 * cr) + 0.5), 0, max)
 *   B = clamp(trunc(((0.999823 * y + 1.77204 * cb) - 0.000008 * cr) + 0.5), 0, max)
 * in IEEE double, every product, sum and difference rounded on its own, left
 * to right (no FMA), the conversion to int32 truncating.  Deviations from the
 * reference: the three output channels are reported UNSIGNED and the
 * precision step treats them so (the reference leaves sgnd = 1 on a signed
 * chroma component that now holds [0, max], and its -p clip would cut G and B
 * at 2^(p-1) - 1); a signed component 0, on which the reference's "assuming
 * unsigned" loop computes regardless, is refused.
 *
 * colour = GRKGPU_COLOUR_CMYK (color_cmyk_to_rgb, color.cpp:881-933): n >= 4
 * components on one grid, components 0 .. 3 unsigned with precisions q_k in
 * 1 .. 16; anything else is GRKGPU_EINVAL (signed inks, from which the
 * reference makes negative garbage, included).  With
 * s_k = 1.0f / (float)(2^q_k - 1), one correctly rounded float32 division:
 *   C = 1.0f - (float)U_0 * s_0      (likewise M, Y, K)
 *   R = (int32)((255.0f * C) * K),  G = ... M ...,  B = ... Y ...
 * in float32, every operation rounded on its own (no FMA), the conversions
 * truncating.  The output has n - 1 CHANNELS: R, G, B unsigned of precision 8
 * (every result lies in 0 .. 255), then components 4 .. as channels 3 .. with
 * their own precision and sign.
 *
 * GRKGPU_COLOUR_FORCE_RGB, or'ed into colour (grk_decompress --force-rgb,
 * convert_gray_to_rgb, grk_decompress.cpp:805-890), looks at the channels left
 * by the steps above: 1 or 2 -> channel 0 three times (R = G = B, its
 * precision and sign), a second channel following as channel 3 (k_palette_*'s
 * store with a direct map); every component must be at (1,1) and the stream
 * carry no custom MCT, else GRKGPU_EUNSUPPORTED.  3 or more: nothing when this
 * call converted (SYCC / EYCC / CMYK), else GRKGPU_EINVAL ("don't know how to
 * convert to RGB": a raw codestream has no colour space).
 *
 * With any of these, out->sample_fmt has to hold the precision and sign of
 * the OUTPUT CHANNELS (R, G, B: 8 bits after CMYK), planar out->planes[] has
 * one entry per output channel, an interleaved pixel that many samples, and
 * img receives the output channels: count, precision, sign.  Samples nothing
 * decoded are converted like any other: CMYK of zeros is (255, 255, 255) and
 * zero extras, EYCC of zeros the formula at (0, 0, 0).  EYCC or CMYK behind a
 * JP2 palette or channel swap is GRKGPU_EUNSUPPORTED.  Value 2 is
 * GRKGPU_COLOUR_AUTO and 5 GRKGPU_COLOUR_AUTO_RGB, both for
 * grkgpu_jp2_decompress only (GRKGPU_EINVAL elsewhere).  Not taken: ICC and
 * CIELab (they need a colour management library), per-component -p lists. */
enum { GRKGPU_COLOUR_NONE = 0, GRKGPU_COLOUR_SYCC = 1, GRKGPU_COLOUR_EYCC = 3, GRKGPU_COLOUR_CMYK = 4 };
#define GRKGPU_COLOUR_FORCE_RGB 0x100u
enum { GRKGPU_PREC_CLIP = 0, GRKGPU_PREC_SCALE = 1 };
typedef struct {
    uint32_t colour;     /* GRKGPU_COLOUR_* [| GRKGPU_COLOUR_FORCE_RGB] */
    uint32_t prec;       /* 0: keep each component's precision; 1..16: output precision of every component */
    uint32_t prec_mode;  /* GRKGPU_PREC_*; read only when prec != 0 */
    uint32_t reserved;   /* 0 */
} grkgpu_out_ops;
int grkgpu_decompress_convert(grkgpu_ctx *ctx, const uint8_t *cs, size_t len, const grkgpu_dparams *p,
                              uint32_t tile_begin, uint32_t tile_end, grkgpu_image_desc *img,
                              const grkgpu_out_planes *out, const grkgpu_out_ops *ops);
/* grkgpu_decompress_convert that also decodes a stream whose COD carries
 * MCT = 2: the Part-2 array-based multi-component transform grkgpu_set_mct
 * (grk_set_MCT) encodes, which every other decode entry point refuses as the
 * reference's j2k_read_cod does.  The main header's CBD / MCT / MCC / MCO
 * segments give the n x n decoding matrix D (float32, row-major) and the
 * offsets off_j (the offset array's entries cast to int32); with x_k component
 * k's sample after the inverse 9/7 wavelet, per pixel and component j
 *     acc = 0.0f;  for k = 0 .. n-1:  acc = acc + D[j][k] * x_k
 *     out_j = clamp((int32) lrintf(acc) + off_j, min_j, max_j)
 * every product and sum rounded on its own in float32 (no FMA), min_j / max_j
 * those of component j's precision and sign: mct::decode_custom (mct.cpp:
 * 477-511) then dc_level_shift_decode (TileProcessor.cpp:1377-1432), for any
 * n >= 1, with the offsets added.  ops (NULL: none) then run on out_j.
 * Accepted: CBD equal to SIZ; MCT arrays in one segment each (Zmct = Ymct = 0),
 * decorrelation and offset, elements int16 / int32 / float32 / float64; one
 * MCC record of one array-based irreversible collection over all components in
 * order; one MCO stage naming it; every component 9/7 and at (1,1).  Anything
 * else the segments ask for -- and MCT / MCC / MCO in a tile-part header -- is
 * GRKGPU_EUNSUPPORTED; segments of a wrong size, a dangling array index, a
 * non-finite entry or no usable MCO are GRKGPU_ECORRUPT.  Never a silent
 * decode without the transform.  On a stream without MCT = 2 this is
 * grkgpu_decompress_convert, launch for launch. */
int grkgpu_decompress_mct(grkgpu_ctx *ctx, const uint8_t *cs, size_t len, const grkgpu_dparams *p,
                          uint32_t tile_begin, uint32_t tile_end, grkgpu_image_desc *img,
                          const grkgpu_out_planes *out, const grkgpu_out_ops *ops);
/* Decode a batch of codestreams in one launch set: item i is the whole-image
 * decode grkgpu_decompress_to(ctx, cs, len, p, 0, 0xffffffff, &img, &out) and
 * receives that call's samples bit for bit, but the n items share one upload
 * of their codestreams, one Tier-1 launch per code-block style, one inverse
 * DWT launch sequence and one store launch per (sample format, layout) present
 * -- the way a few dozen code-blocks per image fill the device.  Items may
 * differ in everything grkgpu_decompress_to takes: geometry, tile grid,
 * components (1 .. 16; more than four go through per-tile store launches),
 * precision, sign, wavelet, code-block size and style, layers, progression,
 * tile-part markers, sample format, layout and host / device destination.
 * p (NULL: defaults) applies to every item: cp_reduce and cp_layer; a decode
 * area is GRKGPU_EINVAL for the call, as are a NULL ctx or items with n > 0;
 * n = 0 is GRKGPU_OK.
 *
 * Every check that can refuse a stream runs on the host before the first
 * device call.  An item that fails gets its code in `status` -- what the
 * single call would have returned, and GRKGPU_EUNSUPPORTED for a stream with a
 * subsampled component, GRKGPU_LAYOUT_UPSAMPLE in out.layout and a custom-MCT
 * stream, which this call does not take -- and its destination is left
 * untouched; the other items are decoded.  The call returns GRKGPU_OK when
 * every item succeeded, else the first failing item's code with
 * grkgpu_last_error() = "item <i>: <its message>".  A cut stream the single
 * call accepts is accepted, its missing tiles zero.  Merged tables beyond the
 * 32-bit limits of one call (blocks, passes, unstuffed words): the whole call
 * is GRKGPU_EUNSUPPORTED "batch too large for one call" before any device
 * work; the caller splits.  grkgpu_get_stats reports the batch (num_cblks and
 * cs_bytes are sums); the call is one call in progress for the Tier-1 plan,
 * chosen on the merged block count.
 *
 * info (may be NULL): items decoded, code-blocks, job-table store records and
 * n_launches, the call's kernel launches and fills (the DWT plan's device
 * copies included, the H2D / D2H copies not): 64 copies of a stream take the
 * launches of one.
 * grkgpu_batch_plan is the host half alone -- no device call, no ctx, the
 * items' `out` planes not read: status / img of every item and info with
 * n_launches = 0. */
typedef struct {
    const uint8_t *cs;     /* in: one raw codestream */
    size_t len;
    grkgpu_out_planes out; /* in: this item's destination (format, layout, host / device) */
    grkgpu_image_desc img; /* out: geometry, as grkgpu_decompress_to reports it */
    int32_t status;        /* out: GRKGPU_OK or the code this item alone would have returned */
    uint32_t pad_;
} grkgpu_batch_item;
typedef struct { uint32_t n_ok, n_blocks, n_store_jobs, n_launches; } grkgpu_batch_info;
int grkgpu_decompress_batch(grkgpu_ctx *ctx, grkgpu_batch_item *items, uint32_t n, const grkgpu_dparams *p,
                            grkgpu_batch_info *info);
int grkgpu_batch_plan(grkgpu_batch_item *items, uint32_t n, const grkgpu_dparams *p, grkgpu_batch_info *info);
/* grkgpu_decompress_batch with the converting and upsampling last store: item i
 * is grkgpu_decompress_convert(ctx, cs, len, p, 0, 0xffffffff, &img, &out,
 * &ops[i]) and receives that call's samples and img descriptor bit for bit
 * (output channels, precision and sign, dx = dy = 1 where that call reports
 * them).  ops is NULL (no item converts) or has n entries.  Beyond what
 * grkgpu_decompress_batch takes, an item may be a stream with subsampled
 * components -- on their own grids (one plane per component), or with
 * GRKGPU_LAYOUT_UPSAMPLE in out.layout on the image grid -- and may ask for
 * GRKGPU_COLOUR_SYCC (which implies the upsampled output), _EYCC, _CMYK and an
 * output precision of 1 .. 16 bits, clipped or scaled; cp_reduce and cp_layer
 * follow the single call's rules per item (cp_reduce with SYCC or the
 * upsample flag on a subsampled stream is that item's GRKGPU_EINVAL).  The
 * last store is then two table phases in stream order behind the zero fills:
 * the stores on the components' own grids (to the output, or to staging
 * planes behind the output staging), then the upsampling / converting store
 * (grkgpu_convert_jobs_to's kernels), one launch per (phase, thread shape,
 * sample format, layout, op class) present, so 64 copies of a 4:2:0 stream
 * take the launches of one.  Samples nothing decoded (a reduced decode's zero
 * margin, tiles a cut stream never reached) are converted like any other, by
 * jobs with null sources.  Items of more than four components go through the
 * single call's per-tile launches.
 * Refused per item with GRKGPU_EUNSUPPORTED: GRKGPU_COLOUR_FORCE_RGB and a
 * custom-MCT stream; GRKGPU_COLOUR_AUTO / _AUTO_RGB and bad ops are
 * GRKGPU_EINVAL as in the single call; all on the host before the first
 * device call.  The call-level rules, the failing items' untouched
 * destinations and info are grkgpu_decompress_batch's (n_store_jobs counts
 * the records of every table).  With ops == NULL, no subsampled item and no
 * upsample flag the call is grkgpu_decompress_batch, launch for launch.
 * grkgpu_batch_convert_plan is the host half alone. */
int grkgpu_decompress_batch_convert(grkgpu_ctx *ctx, grkgpu_batch_item *items, const grkgpu_out_ops *ops,
                                    uint32_t n, const grkgpu_dparams *p, grkgpu_batch_info *info);
int grkgpu_batch_convert_plan(grkgpu_batch_item *items, const grkgpu_out_ops *ops, uint32_t n,
                              const grkgpu_dparams *p, grkgpu_batch_info *info);
/* Decode straight to normalised float32 / float16 / bfloat16 samples: what a
 * network takes, written once by the store of the last decode kernel instead of
 * an integer image followed by x.to(float) * scale + bias passes over it.
 *
 * grkgpu_decompress_float is grkgpu_decompress_convert with one of the float
 * formats below in out->sample_fmt -- valid in these calls only; every other
 * entry point keeps refusing a sample_fmt above GRKGPU_SAMPLE_I16.  Let v be
 * the int32 value grkgpu_decompress_convert delivers for output channel ch
 * with the same ops and GRKGPU_SAMPLE_I32 (after inverse MCT, DC shift, clamp,
 * upsampling, colour step and precision op).  The sample stored is
 *     f = fadd(fmul((float)v, norm->scale[ch]), norm->bias[ch])
 * in float32: (float)v rounds to nearest even (exact below 2^24), the product
 * and the sum are each rounded on their own (no FMA), nothing is flushed to
 * zero.  F32 stores f; F16 / BF16 store f rounded to nearest even, overflow
 * going to +-inf, float16 subnormals kept.  In numpy:
 *     (v.astype(float32) * float32(s) + float32(b)).astype(float16)
 * Samples nothing decoded (the zero margin of a reduced decode at an odd
 * origin, an upsampled stream's zero lead-in, tiles a cut stream never
 * reached) are normalised like any other: bias[ch] without a colour step, the
 * normalised conversion of zeros with one.
 *
 * ops may be NULL; norm == NULL is scale 1, bias 0.  Everything
 * grkgpu_decompress_convert takes on a raw codestream is taken: both layouts
 * and GRKGPU_LAYOUT_UPSAMPLE, SYCC / EYCC / CMYK and the precision op, window,
 * cp_reduce, cp_layer and a tile range under that call's rules, host or device
 * planes (aligned to the sample size).  A float format holds every precision
 * and sign, so the "format holds the precision" rule does not apply; img is
 * what grkgpu_decompress_convert reports -- the channels' integer precision
 * and sign, from which the caller chooses scale.  GRKGPU_EINVAL before any
 * device call: an integer sample_fmt, a non-finite scale or bias among the
 * output channels (entries beyond them are not read), and everything
 * grkgpu_decompress_convert refuses so.  GRKGPU_EUNSUPPORTED:
 * GRKGPU_COLOUR_FORCE_RGB (it stores through the palette kernels) and a
 * custom-MCT stream.
 *
 * grkgpu_decompress_batch_float is grkgpu_decompress_batch_convert in the same
 * way: item i is grkgpu_decompress_float on that item bit for bit, with
 * norms[i] (norms NULL: scale 1, bias 0 for every item).  Items may differ in
 * float format, layout, ops and norm; an item with an integer format gets
 * GRKGPU_EINVAL in its status and the others decode.  The call-level rules,
 * the untouched destinations of failed items and info are unchanged, and the
 * launch count does not depend on the number of items.
 * grkgpu_batch_float_plan is the host half alone.
 *
 * Out of scope (integer formats only): JP2 files and the palette store
 * (grkgpu_jp2_*), the custom-MCT store (grkgpu_decompress_mct) and force-RGB,
 * the stage calls (grkgpu_*_to, grkgpu_*_jobs_to), grkgpu_decompress_multi,
 * the grk_* API and the plugin, and float input to the encoder. */
enum { GRKGPU_SAMPLE_F32 = 16, GRKGPU_SAMPLE_F16 = 17, GRKGPU_SAMPLE_BF16 = 18 }; /* decode output only */
typedef struct { float scale[GRKGPU_MAX_COMPS], bias[GRKGPU_MAX_COMPS]; } grkgpu_out_norm; /* per output channel */
int grkgpu_decompress_float(grkgpu_ctx *ctx, const uint8_t *cs, size_t len, const grkgpu_dparams *p,
                            uint32_t tile_begin, uint32_t tile_end, grkgpu_image_desc *img,
                            const grkgpu_out_planes *out, const grkgpu_out_ops *ops, const grkgpu_out_norm *norm);
int grkgpu_decompress_batch_float(grkgpu_ctx *ctx, grkgpu_batch_item *items, const grkgpu_out_ops *ops,
                                  const grkgpu_out_norm *norms, uint32_t n, const grkgpu_dparams *p,
                                  grkgpu_batch_info *info);
int grkgpu_batch_float_plan(grkgpu_batch_item *items, const grkgpu_out_ops *ops, const grkgpu_out_norm *norms,
                            uint32_t n, const grkgpu_dparams *p, grkgpu_batch_info *info);
/* Encode a batch of images in one launch set: item i is the whole-image encode
 * grkgpu_compress_ex(ctx, &img, p, &in, 0, 0xffffffff, GRKGPU_PART_ALL, ...)
 * and receives that call's codestream byte for byte, but the n items share
 * one upload of their host samples (staged into one pinned buffer, each plane
 * on a 16-byte boundary; device-resident items are read in place), one DC
 * shift / MCT launch per source format and layout present (a job table,
 * grkgpu_dcshift_mct_fwd_jobs; tiles of more than four components go through
 * per-tile launches), one forward DWT launch sequence per wavelet, one Tier-1
 * launch set per distinct code-block style, one gather launch and one D2H.
 * Items may differ in everything grkgpu_compress_ex takes for a whole image:
 * geometry, image and tile offsets, tile grid, components (1 .. 16),
 * precision, sign, wavelet, resolutions, code-block size and style, precincts,
 * layers with rate control, progression and POC, SOP / EPH, tile-parts and
 * TLM, the cinema profiles, ROI, sample format with its flags, host or device
 * source (in.row0 .. in.ncols as there: the whole image must be held).
 *
 * Every check that can refuse an image before a device is touched runs on the
 * host first (the parameters, the sample-format rules, the 255 tile-part
 * limit).  Not taken by this call, GRKGPU_EUNSUPPORTED for the item: a
 * subsampled component, and a custom MCT (tcp_mct == 2 / grkgpu_set_mct).  An
 * item that fails gets its code in `status` -- what the single call would have
 * returned -- with cs = NULL and len = 0; the other items are encoded.  A
 * failure that shows only after Tier-1 ("code-block numbps exceeds its band's
 * bound", "too many coding passes", "MQ slab overflow", "rate allocation
 * failed") fails that item alone.  The call returns GRKGPU_OK when every item
 * succeeded, else the first failing item's code with grkgpu_last_error() =
 * "item <i>: <its message>".  A NULL ctx, or NULL items with n > 0:
 * GRKGPU_EINVAL; n = 0 is GRKGPU_OK.  Merged tables beyond the 32-bit limits
 * of one call (code-blocks, pass-record slots, gather runs): the whole call is
 * GRKGPU_EUNSUPPORTED "batch too large for one call" before any device work;
 * the caller splits.
 *
 * cs / len point into the context's pinned output buffer, each item's stream
 * on a 16-byte boundary, valid until the next call on ctx.  grkgpu_get_stats
 * reports the batch (num_cblks, cs_bytes and mq_symbols are sums); the call is
 * one call in progress for the Tier-1 plan, chosen on the merged block count
 * of each style group.  info (may be NULL): items encoded, code-blocks,
 * job-table load records and n_launches, the call's kernel launches and fills
 * (the DWT plan's device copies included, the H2D / D2H copies not): 64
 * copies of an image take the launches of one.
 * grkgpu_compress_batch_plan is the host half alone -- no device call, no ctx,
 * the items' planes not read: status of every item and info with
 * n_launches = 0. */
typedef struct {
    grkgpu_image_desc img;   /* in */
    const grkgpu_cparams *p; /* in; NULL: grkgpu_default_cparams */
    grkgpu_planes in;        /* in: this item's samples (format + flags, host / device) */
    const uint8_t *cs;       /* out: this item's codestream, in the context's pinned output buffer */
    size_t len;              /* out */
    int32_t status;          /* out: GRKGPU_OK or the code this item alone would have returned */
    uint32_t pad_;
} grkgpu_cbatch_item;
typedef struct { uint32_t n_ok, n_blocks, n_load_jobs, n_launches; } grkgpu_cbatch_info;
int grkgpu_compress_batch(grkgpu_ctx *ctx, grkgpu_cbatch_item *items, uint32_t n, grkgpu_cbatch_info *info);
int grkgpu_compress_batch_plan(grkgpu_cbatch_item *items, uint32_t n, grkgpu_cbatch_info *info);
/* The custom MCT of a codestream, host only: grkgpu_read_header's img (may be
 * NULL) for a stream with or without MCT = 2, and for the former *n = numcomps,
 * matrix[n * n] and offsets[n] (room for 256 / 16; either may be NULL) as
 * grkgpu_decompress_mct applies them.  *n = 0: no custom MCT. */
int grkgpu_read_mct(const uint8_t *cs, size_t len, grkgpu_image_desc *img, float *matrix, int32_t *offsets,
                    uint32_t *n);
/* ---------------------------------------------------------------------------
 * JP2 files (ISO/IEC 15444-1 Annex I): the box layer of Grok's
 * codestream/jp2.cpp on the host, its palette and channel order in the store
 * of the last decode kernel.
 *
 * Reader: jp2_read_header_procedure and its box handlers restated check for
 * check, so a file is refused (GRKGPU_ECORRUPT) where the reference refuses
 * it: signature box first, ftyp second, jp2h before jp2c, ihdr required and 14
 * bytes, XL lengths, LBox 0 = to the end of the file, unknown boxes skipped,
 * ihdr-family boxes outside jp2h read only after jp2h, a second ihdr / colr
 * ignored, METH > 2 ignored, METH 2 without profile bytes refused, cmap only
 * after pclr and only once, NE 1 .. 1024, NPC >= 1, every rule of
 * jp2_check_color including its single-component cmap repair, a pclr without
 * cmap dropped.  The codestream is the jp2c payload; the geometry is SIZ's and
 * is not compared with ihdr, as in the reference.  res / xml / uuid boxes are
 * checked for the sizes the reference insists on and their contents dropped.
 * The jp2c LBox is trusted (the reference reads on to EOC whatever it says).
 *
 * Decoded by the reference, GRKGPU_EUNSUPPORTED here: a palette of more than
 * GRKGPU_MAX_COMPS columns; a palette column wider than 16 bits or with the
 * sign bit set (the reference stores the raw unsigned entry in a component it
 * then marks signed); a cmap entry of MTYP 1 whose PCOL is not its own index
 * (the reference asserts, and in a release build writes another channel's
 * plane); a cmap over a subsampled component, or a cdef swap on a subsampled
 * image; a jp2c payload of 4 GiB or more; more than GRKGPU_JP2_MAX_CDEF
 * channel definitions.
 * ------------------------------------------------------------------------- */
#define GRKGPU_JP2_MAX_CDEF 64
/* GRK_CLRSPC_* (grok.h), as jp2_decode maps METH / EnumCS: 12 CMYK, 14 CIE
 * (default or custom), 16 sRGB, 17 gray, 18 sYCC, 24 eYCC, METH 2 ICC,
 * anything else unknown */
enum {
    GRKGPU_CS_UNKNOWN = 0, GRKGPU_CS_UNSPECIFIED = 1, GRKGPU_CS_SRGB = 2, GRKGPU_CS_GRAY = 3, GRKGPU_CS_SYCC = 4,
    GRKGPU_CS_EYCC = 5, GRKGPU_CS_CMYK = 6, GRKGPU_CS_DEFAULT_CIE = 7, GRKGPU_CS_CUSTOM_CIE = 8, GRKGPU_CS_ICC = 9
};
typedef struct {
    uint64_t cs_offset, cs_length;   /* the codestream: the jp2c payload inside the file */
    uint32_t ihdr_w, ihdr_h, ihdr_nc, ihdr_bpc; /* as read; informational */
    uint32_t meth, enumcs;           /* of the first colr box with METH 1 or 2 (0, 0: none) */
    uint32_t colour_space;           /* GRKGPU_CS_* */
    uint32_t icc_length;             /* METH 2: the ICC profile, file[icc_offset .. + icc_length) */
    uint64_t icc_offset;
    uint32_t cielab_words;           /* EnumCS 14: 2 or 9 words of cielab[] as jp2_read_colr builds them */
    uint32_t cielab[9];              /* 14, 'DEF\0' or 0 (custom), then rl, ol, ra, oa, rb, ob, il */
    /* palette: present only when it is applied (pclr AND cmap) */
    uint32_t pal_entries, pal_columns;         /* NE, NPC; 0, 0: no palette */
    uint32_t pal_prec[GRKGPU_MAX_COMPS];       /* per column */
    int32_t pal_sgnd[GRKGPU_MAX_COMPS];
    uint32_t cmap_cmp[GRKGPU_MAX_COMPS], cmap_mtyp[GRKGPU_MAX_COMPS], cmap_pcol[GRKGPU_MAX_COMPS]; /* after the repair */
    /* channel definitions as the file gives them */
    uint32_t cdef_n;
    uint16_t cdef_cn[GRKGPU_JP2_MAX_CDEF], cdef_typ[GRKGPU_JP2_MAX_CDEF], cdef_asoc[GRKGPU_JP2_MAX_CDEF];
    /* the output channels after jp2_apply_pclr and jp2_apply_cdef (its swaps,
     * and its rewrite of later cn entries): channel c leaves with chan_prec /
     * chan_sgnd, carries alpha type chan_alpha (the cdef Typ: 0 colour, 1
     * opacity, 2 premultiplied opacity, 65535 unspecified) and takes codestream
     * component chan_comp's sample -- directly (chan_pcol < 0) or as the index
     * into palette column chan_pcol */
    uint32_t numchannels;
    uint32_t chan_prec[GRKGPU_MAX_COMPS];
    int32_t chan_sgnd[GRKGPU_MAX_COMPS];
    uint32_t chan_alpha[GRKGPU_MAX_COMPS];
    uint32_t chan_comp[GRKGPU_MAX_COMPS];
    int32_t chan_pcol[GRKGPU_MAX_COMPS];
    uint32_t mapped;                 /* 1: the channels are not the components in order (the palette store runs) */
    uint32_t reserved;
} grkgpu_jp2_info;
/* Host only (no device needed): info = the fields above, img (may be NULL) =
 * the OUTPUT channels on the image's grid (numcomps = numchannels, their
 * precisions and signs, SIZ's rectangle and subsampling).  A raw codestream is
 * GRKGPU_ECORRUPT (no signature box); a codestream header this decoder does
 * not take keeps grkgpu_read_header's code. */
int grkgpu_jp2_read_info(const uint8_t *file, size_t len, grkgpu_jp2_info *info, grkgpu_image_desc *img);
/* The applied palette's table: pal_entries x pal_columns values, row-major, into
 * entries[cap] (cap >= that product, else GRKGPU_EINVAL); *n = the product, 0
 * for a file without an applied palette.  Host only. */
int grkgpu_jp2_read_palette(const uint8_t *file, size_t len, uint16_t *entries, uint32_t cap, uint32_t *n);
/* grkgpu_decompress_convert on the jp2c payload with the palette and the
 * channel order applied by the store of the last decode kernel
 * (k_palette_planar / k_palette_pixels): an index component is finished as
 * ever (inverse MCT, DC shift, clamp to its range), then k = clamp(v, 0, NE - 1)
 * and channel c receives entries[k * NPC + pcol_c]; a directly used channel
 * receives its component's sample.  out, its sample format (which must hold
 * each OUTPUT channel's precision: the palette sizes, or ops->prec) and ops
 * describe channels; img receives them.  Window, cp_reduce, cp_layer, tile
 * ranges, cut streams, host or device planes, the five formats and both
 * layouts keep grkgpu_decompress_to's rules; samples nothing decoded are
 * mapped like any other (entry 0), as the reference's pass does.
 * ops->colour = GRKGPU_COLOUR_AUTO (valid only here): SYCC when EnumCS is 18
 * (then SYCC's shape rules hold: GRKGPU_EINVAL otherwise), NONE for every other
 * space -- CMYK, eYCC, CIELab and ICC are reported in info and not converted.
 * SYCC together with a palette or a channel swap is GRKGPU_EUNSUPPORTED.  A
 * file without palette or swap takes grkgpu_decompress_convert's launches,
 * launch for launch.  info (may be NULL) as grkgpu_jp2_read_info.
 * ops->colour = GRKGPU_COLOUR_AUTO_RGB (valid only here): SYCC for EnumCS 18,
 * EYCC for 24, CMYK for 12 (each with its shape rules), NONE for every other
 * space.  EYCC or CMYK together with a palette or a channel swap is
 * GRKGPU_EUNSUPPORTED.  GRKGPU_COLOUR_FORCE_RGB may be or'ed into any value:
 * as above, on the file's channels (behind a palette too); 3 or more channels
 * are also left alone when the file says sRGB (EnumCS 16); a file with an ICC
 * profile and the flag is GRKGPU_EUNSUPPORTED (the reference would run its
 * colour management library). */
#define GRKGPU_COLOUR_AUTO 2u
#define GRKGPU_COLOUR_AUTO_RGB 5u
int grkgpu_jp2_decompress(grkgpu_ctx *ctx, const uint8_t *file, size_t len, const grkgpu_dparams *p,
                          uint32_t tile_begin, uint32_t tile_end, grkgpu_image_desc *img,
                          const grkgpu_out_planes *out, const grkgpu_out_ops *ops, grkgpu_jp2_info *info);
/* A batch of JP2 files in one launch set: grkgpu_decompress_batch_convert with
 * the box layer per item.  items[i].cs / len are the FILE (only its jp2c
 * payload is uploaded); item i is grkgpu_jp2_decompress(ctx, file, len, p, 0,
 * 0xffffffff, &img, &out, &ops[i], &infos[i]) and receives that call's samples
 * and img bit for bit.  ops is NULL or has n entries, in which
 * GRKGPU_COLOUR_AUTO, _AUTO_RGB and _FORCE_RGB are valid per item; infos is
 * NULL or has n entries (as grkgpu_jp2_read_info fills them; zeroed for a file
 * whose boxes do not parse).  A file without a palette or a channel swap
 * contributes exactly the records grkgpu_decompress_batch_convert makes for
 * its payload with the resolved ops.  A file with a palette, a channel swap
 * or force-RGB on one or two channels is stored through job tables of the
 * palette store (grkgpu_palette_jobs_to's kernel): the items' tables packed
 * into one merged table that rides behind the codestreams in their one H2D
 * copy, one launch per (sample format, layout shape, table size class, with or
 * without precision ops) present, the fills over samples nothing decoded in
 * launches ahead of the tiles' -- so 64 copies of a palette file take the
 * launches of one.  Items of more than four components or channels keep the
 * single call's per-tile launches.  The boxes are parsed and every check runs
 * on the host before the first device call; a failing item gets the single
 * call's code in `status` (a raw codestream: GRKGPU_ECORRUPT; force-RGB on a
 * file with an ICC profile: GRKGPU_EUNSUPPORTED), its destination is left
 * untouched and the others decode.  The call-level rules (decode area, n = 0,
 * NULL arguments, "batch too large for one call", the return code and
 * "item <i>: ..." message) and info are grkgpu_decompress_batch's;
 * n_store_jobs counts the records of every table.  With no mapped item and no
 * force-RGB the call is grkgpu_decompress_batch_convert on the payloads,
 * launch for launch.  grkgpu_jp2_batch_plan is the host half alone. */
int grkgpu_jp2_decompress_batch(grkgpu_ctx *ctx, grkgpu_batch_item *items, const grkgpu_out_ops *ops, uint32_t n,
                                const grkgpu_dparams *p, grkgpu_batch_info *info, grkgpu_jp2_info *infos);
int grkgpu_jp2_batch_plan(grkgpu_batch_item *items, const grkgpu_out_ops *ops, uint32_t n, const grkgpu_dparams *p,
                          grkgpu_batch_info *info, grkgpu_jp2_info *infos);
/* Writer: jp, ftyp (brand 'jp2 ', MinV 0, CL 'jp2 '), jp2h { ihdr, bpcc only
 * when the depths differ (BPC 255), colr, cdef only for exactly one alpha
 * channel behind the colour channels (jp2_setup_encoder, jp2.cpp:2264-2343) },
 * jp2c -- byte for byte what the reference's encoder writes around the same
 * codestream.  res / xml / uuid boxes and an XL jp2c (images above 2^30 sample
 * bytes, where the reference writes one) are not written: GRKGPU_EUNSUPPORTED. */
typedef struct {
    uint32_t colour_space;            /* GRKGPU_CS_*: sRGB 16, gray 17, sYCC 18, CMYK 12, default CIE 14, ICC -> METH 2, else EnumCS 0 */
    uint32_t icc_len;                 /* GRKGPU_CS_ICC: the profile */
    const uint8_t *icc;
    uint32_t alpha[GRKGPU_MAX_COMPS]; /* grk_image_comp::alpha of each component (0: colour) */
} grkgpu_jp2_wparams;
/* grkgpu_compress_ex of the whole image with those boxes ahead of the
 * codestream: they travel in the header blob the gather kernel places ahead
 * of the packets, jp2c's LBox set from the gather plan's total before the
 * launch, so the file is assembled in device memory and leaves in the one
 * D2H copy (*out: the context's buffer, as grkgpu_compress_ex). */
int grkgpu_jp2_compress(grkgpu_ctx *ctx, const grkgpu_image_desc *img, const grkgpu_cparams *p,
                        const grkgpu_jp2_wparams *wp, const grkgpu_planes *in, const uint8_t **out, size_t *out_len);
/* The boxes alone, up to and including jp2c's 8-byte header with LBox = 8 +
 * cs_len: what grkgpu_jp2_compress puts ahead of a codestream of cs_len bytes.
 * Host only.  buf[cap] receives *n bytes (cap too small: GRKGPU_EINVAL, *n set). */
int grkgpu_jp2_write_boxes(const grkgpu_image_desc *img, const grkgpu_jp2_wparams *wp, uint64_t cs_len, uint8_t *buf,
                           size_t cap, size_t *n);
/* (multi-device decode into host planes: see grkgpu_device_set above) */
int grkgpu_decompress_multi(const grkgpu_device_set *devs, const uint8_t *cs, size_t len, grkgpu_image_desc *img,
                            int32_t *const *planes);

/* The tile-part walk of a decode, host only (no device needed): the
 * reference decoder's walk over the tile-parts (j2k_decode_tiles,
 * j2k.cpp:1136-1224) -- GRKGPU_OK and decoded[t] = 1 for every
 * tile a decode produces (others stay zero in its output), or the error a
 * short or damaged stream makes the whole decode fail with.  *ntiles = the
 * tile count; decoded holds cap entries (may be NULL). */
int grkgpu_walk_tiles(const uint8_t *cs, size_t len, uint8_t *decoded, uint32_t cap, uint32_t *ntiles);

/* The tables the host half of a decode hands the device half, host only (no
 * device needed): main header, tile-part walk, packet headers and the table
 * layout of grkgpu_decompress_ex(cs, len, p), then copies of
 *   blocks[n_blocks]        one code-block each: where its bytes lie in the
 *                           data buffer (the codestream followed by the
 *                           segments gathered from several chunks), where its
 *                           samples go in the coefficient arena (element offset
 *                           of the top-left sample, rows dstride apart), its
 *                           size, band orientation, bit-planes and coding passes
 *   segs[n_segs], seg_first[n_blocks + 1]
 *                           the codeword segments: block i's are
 *                           segs[seg_first[i] .. seg_first[i + 1])
 *   style[n_blocks]         code-block style of each block's tile-component
 *   roi[n_blocks]           its ROI shift; NULL when no component has one
 * and the sizes those offsets must stay inside: data_bytes, coef_elems (int32
 * / float elements of the coefficient arena) and ll_elems (of the LL arena).
 * The tables are in stream order, before the Tier-1 launch plan reorders
 * them.  Fails as the decode would, before anything is allocated; the arrays
 * are the library's, released by grkgpu_dec_tables_free (which zeroes *t). */
typedef struct {
    uint64_t data_off;    /* byte offset of the block's (first) segment in the data buffer */
    uint64_t dst_off;     /* element offset of the block's top-left in the destination arena */
    uint32_t len, numpasses, numbps, w, h, orient, dstride;
    int32_t irreversible;
    float stepsize;       /* decode step size (Quantizer.cpp:65-104, fraction 0.5) */
    uint32_t pad;
} grkgpu_dec_block;       /* (also the record of the stage call grkgpu_t1_decode_blocks) */
typedef struct {
    uint64_t data_off;
    uint32_t len, npasses, pad_[2];
} grkgpu_dec_seg;
typedef struct {
    uint32_t n_blocks, n_segs;
    uint64_t data_bytes, coef_elems, ll_elems;
    grkgpu_dec_block *blocks;
    grkgpu_dec_seg *segs;
    uint32_t *seg_first;
    uint8_t *style;
    uint8_t *roi;
} grkgpu_dec_tables;
int grkgpu_dec_tables_of(const uint8_t *cs, size_t len, const grkgpu_dparams *p, grkgpu_dec_tables *t);
void grkgpu_dec_tables_free(grkgpu_dec_tables *t);

void grkgpu_free(void *p);

/* ---- stage entry points (device pointers, asynchronous on `stream`) ---- */

int grkgpu_dcshift_mct_fwd(int32_t *const *planes, uint32_t numcomps, uint32_t w, uint32_t h,
                           uint32_t stride, const int32_t *shift, int32_t mct, int32_t irreversible,
                           void *stream);
int grkgpu_mct_inv_dcshift(int32_t *const *planes, uint32_t numcomps, uint32_t w, uint32_t h,
                           uint32_t stride, const uint32_t *prec, const int32_t *sgnd, int32_t mct,
                           int32_t irreversible, void *stream);
/* grkgpu_mct_inv_dcshift out of place, to the sample format and layout of dst
 * (the last kernel of grkgpu_decompress_to on its own; in the reference the
 * caller's own narrowing when it writes a PNM or raw file): src[c] = the
 * int32 (9/7: float bit pattern) planes, rows src_stride apart; dst->planes
 * are device pointers (on_device is not read), rows dst_stride samples apart
 * (>= w, interleaved >= w * numcomps), starting at any sample.  The format
 * must hold every component's precision and signedness (GRKGPU_EINVAL). */
int grkgpu_mct_inv_dcshift_to(const int32_t *const *src, uint32_t numcomps, uint32_t w, uint32_t h,
                              uint32_t src_stride, const uint32_t *prec, const int32_t *sgnd, int32_t mct,
                              int32_t irreversible, const grkgpu_out_planes *dst, uint32_t dst_stride,
                              void *stream);
/* grkgpu_mct_inv_dcshift_to for a table of n tiles in one launch (the last
 * kernel of grkgpu_decompress_batch on its own): jobs is a host array whose
 * src / dst are device pointers (src 4-byte aligned, dst sample aligned;
 * interleaved: dst[0]), numcomps 1 .. 4, strides as there, the DC shift and
 * the clamp bounds given per component, wavelet_mask bit k set = component k
 * holds 9/7 float bit patterns (the MCT follows component 0's).  Every job
 * has the sample format and layout given; the bounds must fit the format.
 * Jobs of w = 0 or h = 0 store nothing.  The table is copied to the device
 * and freed after the launch, so the call synchronises `stream`. */
typedef struct {
    const int32_t *src[4];
    void *dst[4];
    uint32_t src_stride, dst_stride, w, h;
    uint32_t numcomps;
    int32_t mct;
    uint32_t wavelet_mask, pad_;
    int32_t shift[4], min[4], max[4];
} grkgpu_store_job;
int grkgpu_mct_inv_dcshift_jobs_to(const grkgpu_store_job *jobs, uint32_t n, uint32_t sample_fmt, uint32_t layout,
                                   void *stream);
/* The last kernel of grkgpu_decompress_mct on its own, as
 * grkgpu_mct_inv_dcshift_to is grkgpu_decompress_to's: src[c] = float planes
 * (the inverse 9/7 wavelet's output), rows src_stride apart; matrix = numcomps
 * x numcomps row-major, offsets = numcomps entries (NULL: zeros); dst as there. */
int grkgpu_mct_inv_custom_to(const float *const *src, uint32_t numcomps, uint32_t w, uint32_t h,
                             uint32_t src_stride, const float *matrix, const int32_t *offsets, const uint32_t *prec,
                             const int32_t *sgnd, const grkgpu_out_planes *dst, uint32_t dst_stride, void *stream);
/* The palette store of grkgpu_jp2_decompress on its own: src[k] = device plane
 * of component k's int32 samples after the inverse wavelet (5/3; no MCT), rows
 * src_stride apart, finished as grkgpu_mct_inv_dcshift_to does (DC shift of an
 * unsigned component, clamp to prec / sgnd); output channel c < numchannels
 * takes component chan_comp[c]'s sample (chan_pcol[c] < 0) or
 * table[clamp(sample, 0, ne - 1) * npc + chan_pcol[c]].  table: ne x npc uint16
 * in DEVICE memory (may be NULL when no channel looks up); dst as
 * grkgpu_mct_inv_dcshift_to, describing channels -- a narrow sample format has
 * to hold chan_prec[c] bits, unsigned for a looked-up channel. */
int grkgpu_palette_to(const int32_t *const *src, uint32_t numcomps, uint32_t w, uint32_t h, uint32_t src_stride,
                      const uint32_t *prec, const int32_t *sgnd, uint32_t numchannels, const uint32_t *chan_comp,
                      const int32_t *chan_pcol, const uint32_t *chan_prec, const uint16_t *table, uint32_t ne,
                      uint32_t npc, const grkgpu_out_planes *dst, uint32_t dst_stride, void *stream);
/* grkgpu_palette_to for a table of n tiles in one launch per table size class
 * (the last kernel of grkgpu_jp2_decompress_batch on its own; the palette
 * mirror of grkgpu_mct_inv_dcshift_jobs_to): jobs is a host array whose src /
 * dst are device pointers.  The first fields are grkgpu_store_job's, dst and
 * dst_stride describing the numchannels (1 .. 4) output channels; channel c
 * takes component chan_comp[c]'s finished sample (chan_pcol[c] < 0, which
 * [min, max] must fit into the format) or entry
 * table[table_off + clamp(sample, 0, ne - 1) * npc + chan_pcol[c]], narrowed
 * to the format.  table: one merged device table of table_entries uint16
 * entries, 4-byte aligned (may be NULL when no job looks up); table_off even,
 * ne 0 .. 1024, npc 0 .. 16, ne = 0 exactly when no channel of the job looks
 * up.  zero != 0: src is not read (may be NULL), every component counts as
 * finished zero samples -- the fill of samples nothing decoded.  Interleaved
 * jobs of 3 / 4 channels store runs on the destination's 16-byte grid, of 2 a
 * pixel per thread; one channel is a plane.  Jobs of w = 0 or h = 0 store
 * nothing.  ops_ and used_ are set by the call.  The job table is copied to the
 * device and freed after the launch, so the call synchronises `stream`. */
typedef struct {
    const int32_t *src[4];
    void *dst[4];
    uint32_t src_stride, dst_stride, w, h;
    uint32_t numcomps;
    int32_t mct;
    uint32_t wavelet_mask, ops_;
    int32_t shift[4], min[4], max[4];
    uint8_t chan_comp[GRKGPU_MAX_COMPS];
    int8_t chan_pcol[GRKGPU_MAX_COMPS];
    uint32_t numchannels, ne, npc, used_;
    int32_t zero;
    uint32_t table_off;
} grkgpu_palette_job;
int grkgpu_palette_jobs_to(const grkgpu_palette_job *jobs, uint32_t n, const uint16_t *table, uint32_t table_entries,
                           uint32_t sample_fmt, uint32_t layout, void *stream);
/* The upsampling store of grkgpu_decompress_to (GRKGPU_LAYOUT_UPSAMPLE) on its
 * own -- the kernels the decode runs, fed finished samples: src[k] = device
 * plane of component k on its own grid, [ceil(x0 / dx[k]), ceil(x1 / dx[k])) x
 * [ceil(y0 / dy[k]), ceil(y1 / dy[k])), samples of dst's format, rows
 * src_stride[k] samples apart, starting at any sample; dx / dy in 1 .. 255.
 * dst (planar or interleaved; on_device is not read, the upsample flag may be
 * set or not) receives the rectangle [x0, x1) x [y0, y1) of the reference
 * grid by grkgpu_decompress_to's rule, rows dst_stride samples apart (>= x1 -
 * x0, interleaved >= (x1 - x0) * numcomps), starting at any sample. */
int grkgpu_upsample_to(const void *const *src, const uint32_t *src_stride, uint32_t numcomps, const uint32_t *dx,
                       const uint32_t *dy, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                       const grkgpu_out_planes *dst, uint32_t dst_stride, void *stream);
/* The converting store of grkgpu_decompress_convert on its own -- the kernels
 * the decode runs, fed finished samples; the counterpart of
 * grkgpu_upsample_to, whose geometry and refusals it keeps.  src[k] = device
 * plane of component k on its own grid, samples of src_fmt (a GRKGPU_SAMPLE_*
 * width that holds every (prec[k], sgnd[k]), else GRKGPU_EINVAL); dst's format
 * must hold the output precision and signedness.  ops as above (NULL: no
 * conversion -- the samples replicated and stored in dst's format).  Int32
 * sources with every component at (1,1) run the inverse-MCT kernels' stores,
 * every other shape the upsampling kernels'.  EYCC and CMYK as there (CMYK:
 * dst describes numcomps - 1 channels, dst_stride interleaved >= (x1 - x0) *
 * (numcomps - 1)).  GRKGPU_COLOUR_FORCE_RGB on 1 or 2 components: int32
 * sources at (1,1) with one row stride (dst: 3 or 4 channels), every other
 * shape GRKGPU_EUNSUPPORTED; on 3 or more as there. */
int grkgpu_convert_to(const void *const *src, const uint32_t *src_stride, uint32_t src_fmt, uint32_t numcomps,
                      const uint32_t *dx, const uint32_t *dy, const uint32_t *prec, const int32_t *sgnd,
                      uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                      const grkgpu_out_planes *dst, uint32_t dst_stride, const grkgpu_out_ops *ops, void *stream);
/* grkgpu_convert_to / grkgpu_upsample_to for a table of n jobs (the last two
 * kernels of grkgpu_decompress_batch_convert on their own; the counterpart of
 * grkgpu_mct_inv_dcshift_jobs_to): jobs is a host array, every job storing
 * the rectangle [x0, x1) x [y0, y1) of the reference grid (x1 <= x0 or
 * y1 <= y0: nothing) in the sample format and layout given, dst[] (device) at
 * the rectangle's first pixel -- one plane per output channel, or dst[0]
 * interleaved -- rows dst_stride samples apart.  numcomps 1 .. 4 components,
 * pixel (X, Y) taking component k's sample at column floor(X / dx), row
 * floor(Y / dy) of its grid:
 *   src     device memory holding the grid from column gx0, row gy0 on, rows
 *           `stride` elements apart; NULL: zeros
 *   kind    GRKGPU_SRC_RAW: an int32 tile buffer (wavelet = 1: 9/7 float bit
 *           patterns), finished on the way by shift and the clamp to
 *           [min, max] as in grkgpu_store_job; GRKGPU_SRC_SAMPLES +
 *           GRKGPU_SAMPLE_*: finished samples of that format
 *   zx0/zy0 columns left of zx0 and rows above zy0 read as zero (the
 *           reference's lead-in: ceil(origin / dx) of the image the rectangle
 *           is cut from); zx0 >= gx0, zy0 >= gy0
 *   min/max the component's range, that of a precision and sign (ops and the
 *           destination format are checked against it)
 * mct != 0 (inverse RCT / ICT by component 0's wavelet, on components 0 .. 2)
 * needs raw sources on one grid: every component at dx = dy = 1 with one
 * stride and origin and no lead-in inside the rectangle; such jobs, with or
 * without an MCT, run the store of grkgpu_mct_inv_dcshift_jobs_to with the
 * ops in it, every other job the upsampling store, as 16-byte runs for three
 * components at (1,1), (2,dy), (2,dy) (dy 1 or 2; U8 / U16 / I32, no eYCC /
 * CMYK) and a thread per pixel otherwise.  ops as in grkgpu_convert_to
 * (GRKGPU_COLOUR_FORCE_RGB: GRKGPU_EUNSUPPORTED); CMYK stores numcomps - 1
 * channels.  One launch per (store, thread shape, op class) present.  The
 * tables are copied to the device and freed after the launches, so the call
 * synchronises `stream`. */
enum { GRKGPU_SRC_RAW = 1, GRKGPU_SRC_SAMPLES = 2 };
typedef struct {
    const void *src;
    uint32_t stride;
    int32_t gx0, gy0, zx0, zy0;
    uint8_t dx, dy, kind, wavelet;
    int32_t shift, min, max;
} grkgpu_convert_comp;
typedef struct {
    grkgpu_convert_comp comp[4];
    void *dst[4];
    uint32_t x0, y0, x1, y1;
    uint32_t dst_stride, numcomps;
    int32_t mct;
    uint32_t pad_;
    grkgpu_out_ops ops;
} grkgpu_convert_job;
int grkgpu_convert_jobs_to(const grkgpu_convert_job *jobs, uint32_t n, uint32_t sample_fmt, uint32_t layout,
                           void *stream);
/* grkgpu_dcshift_mct_fwd out of place, from the sample format and layout of
 * src (the first kernel of grkgpu_compress_ex on its own; the counterpart of
 * grkgpu_mct_inv_dcshift_to): src->planes are device pointers (on_device, row0
 * .. ncols are not read), src->sample_fmt a width with its flags, rows
 * src_stride samples apart (>= w, interleaved >= w * numcomps), starting at
 * any byte; dst[c] = int32 planes, rows dst_stride (>= w) apart.  The values
 * are those grkgpu_dcshift_mct_fwd leaves from the same samples.  A
 * big-endian flag on a width other than 16 bits, or unknown flag bits:
 * GRKGPU_EINVAL. */
int grkgpu_dcshift_mct_fwd_from(const grkgpu_planes *src, uint32_t numcomps, uint32_t w, uint32_t h,
                                uint32_t src_stride, const int32_t *shift, int32_t mct, int32_t irreversible,
                                int32_t *const *dst, uint32_t dst_stride, void *stream);
/* grkgpu_dcshift_mct_fwd_from for a table of n tiles in one launch (the first
 * kernel of grkgpu_compress_batch on its own; the counterpart of
 * grkgpu_mct_inv_dcshift_jobs_to): jobs is a host array whose src / dst are
 * device pointers -- src[k] component k's sample at the tile's origin
 * (interleaved: src[0] its first pixel; planar samples in host byte order
 * sample aligned, else any byte), dst[k] its int32 plane -- numcomps 1 .. 4,
 * src_stride in samples (>= w, interleaved >= w * numcomps), dst_stride >= w,
 * the DC shift given per component.  Every job has the sample format given (a
 * width with its flags, as grkgpu_planes.sample_fmt).  Jobs of w = 0 or h = 0
 * load nothing.  The values are those grkgpu_dcshift_mct_fwd_from leaves job
 * by job.  The table goes through the context's buffers and runs on its
 * stream, which the call synchronises. */
typedef struct {
    const void *src[4];
    int32_t *dst[4];
    uint32_t src_stride, dst_stride, w, h;
    uint32_t numcomps;
    int32_t mct, irreversible;
    uint32_t pad_;
    int32_t shift[4];
} grkgpu_load_job;
int grkgpu_dcshift_mct_fwd_jobs(grkgpu_ctx *ctx, const grkgpu_load_job *jobs, uint32_t n, uint32_t sample_fmt);
/* In-place (Mallat layout) forward / inverse DWT of one tile-component with
 * origin (x0,y0), size (x1-x0) x (y1-y0), row stride x1-x0.  scratch must
 * hold grkgpu_dwt_scratch_bytes(...) device bytes.  For 9/7 inverse the buffer
 * holds float bit patterns. */
size_t grkgpu_dwt_scratch_bytes(uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, uint32_t numres);
int grkgpu_dwt_fwd(int32_t *buf, int32_t *scratch, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                   uint32_t numres, int32_t irreversible, void *stream);
int grkgpu_dwt_inv(int32_t *buf, int32_t *scratch, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                   uint32_t numres, int32_t irreversible, void *stream);

/* Code-block descriptors for the T1 entry points (all device memory). */
typedef struct {
    uint64_t coef_off;    /* element offset of the block's top-left in `coef` */
    uint64_t out_off;     /* byte offset in `out`, a multiple of 4 and >= 4: the
                             block's bytes start there, and the encoder writes
                             zeros to out[out_off - 4 .. out_off - 1] (the MQ
                             coder's pad byte before the block, Grok's
                             bp = start - 1, committed with its dword), so no
                             other block's bytes may lie there.  From out_off
                             on the block needs grkgpu_t1_enc_out_bytes(w, h,
                             cblk_sty) bytes of its own, rounded up to 4: the
                             encoder stores whole dwords, and with TERMALL or
                             BYPASS a block of a few samples writes far more
                             than w*h*4 + 64 bytes */
    uint32_t stride, w, h, orient; /* orient = band number 0:LL 1:HL 2:LH 3:HH */
    int32_t qmfbid, inv_step;      /* qmfbid 1 = 5/3, 0 = 9/7 (13-bit inv step) */
} grkgpu_enc_block;

typedef struct {
    uint32_t numbps, numpasses, len, pad;  /* pad != 0: numbps above the band's bound */
    uint32_t nsym, pad1, pad2, pad3;       /* nsym: MQ symbols coded */
    uint32_t rate[96];    /* cumulative pass rates after Grok's fix-ups */
    int32_t nmsedec[96];  /* per-pass normalised distortion decrease (t1.cpp
                             nmsedec; distortiondec = t1_getwmsedec of it,
                             t1.cpp:912-930); filled when with_distortion */
} grkgpu_enc_result;

/* (grkgpu_dec_block: above, with grkgpu_dec_tables_of) */

/* scratch: >= grkgpu_t1_scratch_bytes_n(nblocks) device bytes, encode and
 * decode -- that is (nblocks rounded up to a multiple of 64) *
 * grkgpu_t1_scratch_bytes(): both keep the rows of 64 blocks interleaved, so
 * n * grkgpu_t1_scratch_bytes() is too small when n % 64 != 0; decode: every
 * segment at most GRKGPU_T1_MAX_SEG bytes (w*h*4 + 64 for a 64x64 block, the
 * encoder's slab bound). */
#define GRKGPU_T1_MAX_SEG (64 * 64 * 4 + 64)
size_t grkgpu_t1_scratch_bytes(void);
size_t grkgpu_t1_scratch_bytes_n(uint32_t nblocks);
/* The most bytes grkgpu_t1_encode_blocks[_sty] writes from a w x h block's
 * out_off on (w, h <= 64, else 0): w*h*4 + 64, plus with TERMALL or BYPASS
 * the bytes of every terminated coding pass -- up to 3 per pass, whatever the
 * block's size -- for the deepest block the encoder produces (26 bit-planes).
 * Lay blocks out at least this far apart (rounded up to 4) plus the 4 bytes
 * before each out_off; a block that overran its neighbour is not detected by
 * the stage call. */
size_t grkgpu_t1_enc_out_bytes(uint32_t w, uint32_t h, uint32_t cblk_sty);
int grkgpu_t1_encode_blocks(const grkgpu_enc_block *blocks, uint32_t nblocks, const int32_t *coef,
                            void *scratch, uint8_t *out, grkgpu_enc_result *results, int with_distortion,
                            void *stream);
/* the same with a code-block style (COD SPcod bits 0..5: BYPASS 1, RESET 2,
 * TERMALL 4, VSC 8, PTERM 16, SEGSYM 32) */
int grkgpu_t1_encode_blocks_sty(const grkgpu_enc_block *blocks, uint32_t nblocks, const int32_t *coef,
                                void *scratch, uint8_t *out, grkgpu_enc_result *results, int with_distortion,
                                uint32_t cblk_sty, void *stream);
int grkgpu_t1_decode_blocks(const grkgpu_dec_block *blocks, uint32_t nblocks, const uint8_t *data,
                            void *scratch, int32_t *dst, void *stream);

#ifdef __cplusplus
}
#endif
#endif
