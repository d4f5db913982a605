// grk_device.h -- device-visible descriptors shared by kernels.hip and codec.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "t1_flat.h"

namespace grkgpu {

constexpr int GRK_MAX_COMPS = 16;
constexpr int GRK_MAX_PASSES = 96;  // 3 * 31 - 2 = 91 passes max for cblksty 0

struct PlanePtrs { int32_t *p[GRK_MAX_COMPS]; };
// Image planes as the caller holds them: int32 (grk_image) or the 8 / 16-bit
// samples of the image file (GRKGPU_SAMPLE_*, include/grk_mi355x.h), widened
// to int32 by the kernel that first reads them (DC shift + MCT, or the fused
// DWT level 0) -- an 8K 12-bit frame crosses PCIe as 2 B/sample.
struct SrcPlanes { const void *p[GRK_MAX_COMPS]; };
enum SampleFmt : int32_t { SMP_I32 = 0, SMP_U8 = 1, SMP_I8 = 2, SMP_U16 = 3, SMP_I16 = 4,
                           // decode output of the float entry points only (GRKGPU_SAMPLE_F32 / _F16 / _BF16):
                           // the finished int32 value v leaves as v * scale + bias (OutOps, below)
                           SMP_F32 = 16, SMP_F16 = 17, SMP_BF16 = 18 };
constexpr bool float_fmt(int32_t fmt) { return fmt >= SMP_F32 && fmt <= SMP_BF16; }
// flags on a source format (GRKGPU_SAMPLE_INTERLEAVED / _BIG_ENDIAN): pixels
// in p[0], sample (y, x, c) at p[0][y * stride + x * ncomp + c]; 16-bit
// samples stored most-significant byte first
constexpr int32_t SMP_INTERLEAVED = 0x100, SMP_BIG_ENDIAN = 0x200;
constexpr uint32_t sample_bytes(int32_t fmt) {
    return (fmt & 0xff) == SMP_I32 || (fmt & 0xff) == SMP_F32 ? 4u : ((fmt & 0xff) <= SMP_I8 ? 1u : 2u);
}
struct ShiftArr { int32_t v[GRK_MAX_COMPS]; };

// One code-block to encode (T1Part1::preEncode + t1_encode_cblk inputs,
// t1/Tier1.cpp:24-96 encodeBlockInfo).
struct EncBlock {
    uint64_t coef_off;  // element offset of the block's top-left in the coefficient arena
    uint64_t out_off;   // byte offset of the block's output in the MQ slab, a multiple of 4 and >= 4: the coder
                        // zeroes out[out_off - 4 .. out_off - 1] (its pad byte, committed with its dword), so no
                        // other block's bytes may lie there; the block may write t1_enc_slab_bytes(w, h, sty,
                        // numbps) bytes, rounded up to 4, from out_off on
    uint32_t stride, w, h, orient;
    int32_t qmfbid, inv_step;
};

struct EncResult {
    uint32_t numbps, numpasses, len, pad;  // pad != 0: numbps above the band's bound
    uint32_t nsym, pad1, pad2, pad3;       // nsym: MQ symbols coded
    uint32_t rate[GRK_MAX_PASSES];         // cumulative, after Grok's fix-ups
    int32_t nmsedec[GRK_MAX_PASSES];       // per-pass distortion sums (launch_t1_dist only)
};
// bytes of an EncResult without the distortion sums (what a D2H needs when
// no rate control runs)
constexpr size_t ENC_RESULT_RATE_BYTES = 32 + 4 * GRK_MAX_PASSES;

// Normalised-MSE decrease tables (t1_generate_luts.cpp:290-318, restated):
// index = the 7 magnitude bits from the coded bit-plane down.
struct NmseLut { int16_t sig[128], sig0[128], ref[128], ref0[128]; };
const NmseLut &nmse_lut();

// One code-block to decode (t1/Tier1.cpp:98-175 decodeBlockInfo).
struct DecBlock {
    uint64_t data_off;  // byte offset of the (single) segment in the data buffer
    uint64_t dst_off;   // element offset of the block's top-left in the tile arena
    uint32_t len, numpasses, numbps, w, h, orient, dstride;
    int32_t irrev;
    float step;
    uint32_t pad;       // unstuffed-stream region offset / 16 bytes (launch_t1_decode)
};

struct GatherItem { uint64_t src, dst; uint32_t len, pad; };  // pad: 0 = header blob, 1 = MQ slab

hipError_t launch_dcshift_mct_fwd(const SrcPlanes &src, int32_t fmt, uint32_t sstride, const PlanePtrs &dst,
                                  uint32_t tw, uint32_t th, uint32_t ncomp, const ShiftArr &shift, int32_t mct,
                                  int32_t irrev, hipStream_t s);
// The same pass from a source format with flags (fmt = SampleFmt |
// SMP_INTERLEAVED | SMP_BIG_ENDIAN; launch_dcshift_mct_fwd forwards a flagged
// format here): src rows sstride samples apart starting at any byte, dst rows
// dstride apart.  Interleaved 3 / 4 components: k_dcshift_mct_fwd_pixels (runs
// of 4 pixels: wide loads, one dwordx4 store per component); else one thread
// per sample position.
hipError_t launch_dcshift_mct_fwd_from(const SrcPlanes &src, int32_t fmt, uint32_t sstride, const PlanePtrs &dst,
                                       uint32_t dstride, uint32_t tw, uint32_t th, uint32_t ncomp,
                                       const ShiftArr &shift, int32_t mct, int32_t irrev, hipStream_t s);
// src rows at sstride elements (a window of a tile buffer), dst rows at dstride;
// irrev: bit k set = component k holds 9/7 (float) samples; MCT follows
// component 0's wavelet
// DC shift + custom MCT (Part 2) of one tile: m.c = the n x n encoding matrix in
// 13-bit fixed point (row-major)
struct MctMatrix { int32_t c[GRK_MAX_COMPS * GRK_MAX_COMPS]; };
hipError_t launch_dcshift_mct_custom(const SrcPlanes &src, int32_t fmt, uint32_t sstride, const PlanePtrs &dst,
                                     uint32_t tw, uint32_t th, uint32_t ncomp, const ShiftArr &shift,
                                     const MctMatrix &m, hipStream_t s);
hipError_t launch_mct_inv_dcshift(const PlanePtrs &src, uint32_t sstride, uint32_t tw, uint32_t th,
                                  const PlanePtrs &dst, uint32_t dstride, uint32_t ncomp, const ShiftArr &shift,
                                  const ShiftArr &mn, const ShiftArr &mx, int32_t mct, int32_t irrev, hipStream_t s);
// The same pass, storing the clamped samples in the caller's format `fmt`
// (SampleFmt; the clamp range must fit it, so the narrowing is exact) and
// layout: planar -- dst.p[c] = plane c, rows dstride samples apart -- or
// interleaved -- sample (y, x, c) at dst.p[0][y * dstride + x * ncomp + c].
// Destinations may start at any sample; int32 planar runs launch_mct_inv_dcshift.
struct DstPlanes { void *p[GRK_MAX_COMPS]; };
hipError_t launch_mct_inv_dcshift_to(const PlanePtrs &src, uint32_t sstride, uint32_t tw, uint32_t th,
                                     const DstPlanes &dst, int32_t fmt, bool interleaved, uint32_t dstride,
                                     uint32_t ncomp, const ShiftArr &shift, const ShiftArr &mn, const ShiftArr &mx,
                                     int32_t mct, int32_t irrev, hipStream_t s);
// launch_mct_inv_dcshift_to / _ops (below) for a table of tiles in one launch
// (the batch decode, grkgpu_mct_inv_dcshift_jobs_to / grkgpu_convert_jobs_to):
// each tile's arguments as a record in device memory (grkgpu_store_job's
// layout; static_assert in codec.cpp), 1 .. 4 components, all jobs of a launch
// in one sample format, layout and op class.  irrev: bit k set = component k
// holds 9/7 samples.  One kernel template, k_store_jobs, runs every class: the
// per-tile kernels' store bodies behind a workgroup-to-job search.
struct StoreJob {
    const int32_t *src[4];  // component k's coefficients at the tile's first stored sample
    void *dst[4];           // planar: plane k there; interleaved: dst[0]
    uint32_t sstride, dstride, w, h;
    uint32_t ncomp;
    int32_t mct;
    uint32_t irrev;
    uint32_t ops;  // op != 0: the job's entry of the OutOps table (not read otherwise)
    int32_t shift[4], mn[4], mx[4];
};
// threads along a row of a job: the lead run and the runs of 16 bytes
// (launch_inv's), or the pixels of a two-component interleaved tile
__host__ __device__ inline uint32_t store_job_row_threads(uint32_t w, uint32_t ncomp, uint32_t sb, bool interleaved) {
    if (interleaved && ncomp == 2) return w;
    const uint32_t n = 16 / sb;
    return (uint32_t)(((uint64_t)w + n - 1) / n + 1);
}
// a job's workgroups of 256 threads (0: nothing to store); more than 2^24 do
// not fit the kernel's 32-bit thread index: such a tile takes the launch of its own
inline uint64_t store_job_wgs(const StoreJob &j, uint32_t sb, bool interleaved) {
    if (!j.w || !j.h) return 0;
    return ((uint64_t)store_job_row_threads(j.w, j.ncomp, sb, interleaved) * j.h + 255) / 256;
}
constexpr uint64_t STORE_JOB_MAX_WGS = (uint64_t)1 << 24;
// first: njobs + 1 first-workgroup numbers (prefix sums of store_job_wgs), nwg = first[njobs].
// op: the jobs' op class (OP_* of kernels.hip: 0 none, 1 precision only, 2 sYCC, 3 eYCC, 4 CMYK); op != 0 takes
// ops, the device table of OutOps (below) uploaded with the jobs -- one per item, a job that converts nothing
// pointing at an all-zero entry.  sYCC / eYCC jobs have three components, CMYK jobs four (three channels
// stored); the row threads are store_job_row_threads' either way.
struct OutOps;
hipError_t launch_store_jobs(const StoreJob *jobs, const uint32_t *first, uint32_t njobs, uint32_t nwg, int32_t fmt,
                             bool interleaved, hipStream_t s, int op = 0, const OutOps *ops = nullptr);
// launch_dcshift_mct_fwd / _from for a table of tiles in one launch (the batch
// encode, grkgpu_dcshift_mct_fwd_jobs): each tile's arguments as a record in
// device memory (grkgpu_load_job's layout; static_assert in codec.cpp), 1 .. 4
// components on one grid, all jobs of a launch in one sample format and mode
// (bit 0 big-endian, bit 1 interleaved).
struct LoadJob {
    const void *src[4];  // planar: component k's sample at the tile's origin; interleaved: src[0] = its first pixel
    int32_t *dst[4];     // component k's tile buffer
    uint32_t sstride, dstride, w, h;  // sstride in samples (interleaved: of every component)
    uint32_t ncomp;
    int32_t mct, irrev;
    uint32_t pad_;
    int32_t shift[4];
};
// threads along a row of a job: the lead run and the runs of 4 pixels of an
// interleaved 3 / 4-component source (launch_fwd_from's), else the samples
__host__ __device__ inline uint32_t load_job_row_threads(uint32_t w, uint32_t ncomp, bool interleaved) {
    if (interleaved && (ncomp == 3 || ncomp == 4)) return (uint32_t)(((uint64_t)w + 3) / 4 + 1);
    return w;
}
// a job's workgroups of 256 threads (0: nothing to load); more than
// STORE_JOB_MAX_WGS do not fit the kernel's 32-bit thread index
inline uint64_t load_job_wgs(const LoadJob &j, bool interleaved) {
    if (!j.w || !j.h) return 0;
    return ((uint64_t)load_job_row_threads(j.w, j.ncomp, interleaved) * j.h + 255) / 256;
}
// first: njobs + 1 first-workgroup numbers (prefix sums of load_job_wgs), nwg = first[njobs]
hipError_t launch_load_jobs(const LoadJob *jobs, const uint32_t *first, uint32_t njobs, uint32_t nwg, int32_t fmt,
                            int mode, hipStream_t s);
// The decoded image with its subsampled components replicated to the image
// grid (GRKGPU_LAYOUT_UPSAMPLE, grk_decompress -u): output pixel (X, Y) of the
// reference grid takes component k's sample at column floor(X / dx), row
// floor(Y / dy) of its grid -- zero left of column zx0 or above row zy0 (the
// output rectangle's origin on that grid, ceil(ox0 / dx): the reference's zero
// lead-in).  src holds the grid from (gx0, gy0) on, rows `stride` elements
// apart.  raw: src is a tile buffer of int32 coefficients (irrev: 9/7 float
// bit patterns), finished on the way by k_mct_inv_dcshift's second loop
// (shift, mn, mx); else finished samples of the destination's type (a staging
// plane).  src = null: zeros (a tile the stream never reached).
struct UpComp {
    const void *src;
    uint32_t stride;
    int32_t gx0, gy0, zx0, zy0;
    uint8_t dx, dy, raw, irrev;
    int32_t shift, mn, mx;
};
struct UpPlan { UpComp c[GRK_MAX_COMPS]; };
// The w x h pixels from (X0, Y0) on the reference grid, dst at the first of
// them (format, layout and dstride as launch_mct_inv_dcshift_to).  Three
// components at (1,1), (2,dy), (2,dy) with dy 1 or 2 in U8 / U16 / I32 run
// k_upsample_420 (16-byte runs, chroma replicated in registers); everything
// else k_upsample_any (a thread per pixel, dx / dy 1 .. 255).
hipError_t launch_upsample_to(const UpPlan &src, uint32_t ncomp, uint32_t X0, uint32_t Y0, uint32_t w, uint32_t h,
                              const DstPlanes &dst, int32_t fmt, bool interleaved, uint32_t dstride, hipStream_t s);
// Output conversions of grkgpu_decompress_convert / grkgpu_convert_to, applied
// by the last kernel to the finished int32 run values right before the store
// (grk_decompress's colour and -p steps, color.cpp:136-418 and
// convert.cpp:82-161): sycc != 0 turns the three components (Y, Cb, Cr;
// unsigned, one precision, off = 2^(P-1), upb = 2^P - 1) into R, G, B; then
// pc[k] maps component k to the output precision --
//   POP_CLIP    clamp(v, a, b)
//   POP_SHR     v >> a (arithmetic)
//   POP_MULDIV  (uint32) v * a / b, the unsigned scale-up (the product fits 32 bits)
//   POP_MUL     v * a, the signed scale-up by a power of two
// Everything here is uniform over a launch.
//
// col (COL_*; never together with sycc) is one of the two other conversions
// of grk_decompress's colour step (color.cpp:881-995), which sit where sycc
// sits:
//   COL_EYCC  color_esycc_to_rgb on the three components: cb = v1 - coff[0],
//             cr = v2 - coff[1] (2^(P-1) for an unsigned chroma component, 0
//             for a signed one), then in IEEE double, every operation rounded
//             on its own, left to right, truncating, clamped to [0, upb]
//               R = (y - 0.0000368 * cb + 1.40199 * cr + 0.5)
//               G = (1.0003 * y - 0.344125 * cb - 0.7141128 * cr + 0.5)
//               B = (0.999823 * y + 1.77204 * cb - 0.000008 * cr + 0.5)
//   COL_CMYK  color_cmyk_to_rgb on components 0 .. 3 of ncomp >= 4: in
//             float32, every operation rounded on its own, truncating,
//               C = 1.0f - (float)v0 * sc[0]   (likewise M, Y, K)
//               R = (int32)(255.0f * C * K), G = ... M ..., B = ... Y ...
//             sc[k] = 1.0f / (float)(2^prec_k - 1), divided on the host.  The
//             ncomp components leave as ncomp - 1 CHANNELS: R, G, B, then
//             components 4 .. as channels 3 ..; pc[], the destination planes,
//             dstride and the run ownership of the stores describe channels.
enum : int32_t { POP_NONE = 0, POP_CLIP = 1, POP_SHR = 2, POP_MULDIV = 3, POP_MUL = 4 };
enum : int32_t { COL_NONE = 0, COL_EYCC = 1, COL_CMYK = 2 };
struct PrecOp { int32_t mode, a, b; };
struct OutOps {
    int32_t sycc, off, upb;
    PrecOp pc[GRK_MAX_COMPS];
    int32_t col, coff[2];
    float sc[4];
    // a float destination (SMP_F32 / _F16 / _BF16) only: channel c's value v -- after everything above --
    // leaves as fadd(fmul((float)v, scale[c]), bias[c]), each rounded on its own in float32 (no FMA), then
    // rounded to nearest even to the destination's format.  Not read by any other format's kernels.
    float scale[GRK_MAX_COMPS], bias[GRK_MAX_COMPS];
};
// launch_mct_inv_dcshift_to / launch_upsample_to with the conversions in their
// stores (the same kernels, instantiated with the ops; int32 planes run
// k_mct_inv_dcshift_planar<int32_t>).  sycc / COL_EYCC need ncomp == 3,
// COL_CMYK ncomp >= 4, all three an unsigned or int32 format.  A finished (not raw) UpComp of launch_upsample_ops carries
// its samples' own format f, which may differ from the destination's, as
// raw = UPCOMP_FIN + f: a staging plane keeps the stream's precision when the
// output is narrower.
constexpr uint8_t UPCOMP_FIN = 2;
hipError_t launch_mct_inv_dcshift_ops(const PlanePtrs &src, uint32_t sstride, uint32_t tw, uint32_t th,
                                      const DstPlanes &dst, int32_t fmt, bool interleaved, uint32_t dstride,
                                      uint32_t ncomp, const ShiftArr &shift, const ShiftArr &mn, const ShiftArr &mx,
                                      int32_t mct, int32_t irrev, const OutOps &ops, hipStream_t s);
hipError_t launch_upsample_ops(const UpPlan &src, uint32_t ncomp, uint32_t X0, uint32_t Y0, uint32_t w, uint32_t h,
                               const DstPlanes &dst, int32_t fmt, bool interleaved, uint32_t dstride,
                               const OutOps &ops, hipStream_t s);
// launch_upsample_ops for a table of jobs in one launch (the batch decode with
// output ops, grkgpu_convert_jobs_to; the ops of every job an entry of
// launch_store_jobs' table, uniform over its workgroups): the rectangle [X0, x1) x [Y0, y1) of the
// reference grid from up to four UpComps (a finished one always carries its
// format, raw = UPCOMP_FIN + f), dst at the rectangle's first pixel.
// grkgpu_convert_job's layout up to its ops (static_assert in codec.cpp).
struct ConvJob {
    UpComp c[4];
    void *dst[4];  // planar: plane k of the output channels; interleaved: dst[0]
    uint32_t X0, Y0, x1, y1;
    uint32_t dstride, ncomp;
    int32_t mct_;  // (grkgpu_convert_job.mct: such a job runs as a StoreJob)
    uint32_t ops;
};
// the two thread shapes, by launch_upsample_ops' rule: the 16-byte runs of
// k_upsample_420 (fast) or k_upsample_any's thread per pixel
__host__ __device__ inline bool conv_job_fast(const UpComp *c, uint32_t ncomp, int32_t fmt, int32_t col) {
    return (fmt == SMP_I32 || fmt == SMP_U8 || fmt == SMP_U16 || float_fmt(fmt)) && !col && ncomp == 3 && c[0].dx == 1 &&
           c[0].dy == 1 && c[1].dx == 2 && c[2].dx == 2 && c[1].dy == c[2].dy && (c[1].dy == 1 || c[1].dy == 2);
}
// threads along a row of a job (sb = bytes of a destination sample) and its workgroups of 256 threads
__host__ __device__ inline uint32_t conv_job_row_threads(uint32_t w, uint32_t sb, bool fast) {
    if (!fast) return w;
    const uint32_t n = 16 / sb;
    return (uint32_t)(((uint64_t)w + n - 1) / n + 1);
}
inline uint64_t conv_job_wgs(const ConvJob &j, uint32_t sb, bool fast) {
    if (j.x1 <= j.X0 || j.y1 <= j.Y0) return 0;
    return ((uint64_t)conv_job_row_threads(j.x1 - j.X0, sb, fast) * (j.y1 - j.Y0) + 255) / 256;
}
// fast: every job has conv_job_fast's shape, sycc = the op class (all jobs with the sYCC conversion or all
// without); else any shape, the colour step read from each job's OutOps
hipError_t launch_conv_jobs(const ConvJob *jobs, const uint32_t *first, uint32_t njobs, uint32_t nwg,
                            const OutOps *ops, int32_t fmt, bool interleaved, bool fast, bool sycc, hipStream_t s);
// Inverse custom MCT (Part 2 array-based; COD MCT = 2) + offsets + clamp of one
// tile, where launch_mct_inv_dcshift_to / _ops run for the other streams: src =
// the components' 9/7 samples (float bit patterns), out_j = clamp(lrintf(sum
// over k ascending of d[j][k] * x_k, float32 without FMA) + off_j).  d holds
// the decoding matrix with its rows GRK_MAX_COMPS apart and zeros beyond
// ncomp (set_mct_inv).  Format, layout, dstride and ops (null: none) as
// launch_mct_inv_dcshift_ops.
struct MctInv { float d[GRK_MAX_COMPS * GRK_MAX_COMPS]; };
inline void set_mct_inv(MctInv &m, const float *matrix, uint32_t n) {  // matrix: n x n, row-major
    m = MctInv{};
    for (uint32_t j = 0; j < n; ++j)
        for (uint32_t k = 0; k < n; ++k) m.d[j * GRK_MAX_COMPS + k] = matrix[j * n + k];
}
hipError_t launch_mct_inv_custom(const PlanePtrs &src, uint32_t sstride, uint32_t tw, uint32_t th,
                                 const DstPlanes &dst, int32_t fmt, bool interleaved, uint32_t dstride,
                                 uint32_t ncomp, const MctInv &m, const ShiftArr &off, const ShiftArr &mn,
                                 const ShiftArr &mx, const OutOps *ops, hipStream_t s);
// The JP2 palette / channel order in the last store (jp2_apply_pclr and the
// swaps of jp2_apply_cdef, jp2.cpp:1301-1407, 1564-1623), where
// launch_mct_inv_dcshift_to / _ops run for a file without either: the ncomp
// components are finished as there (mct, irrev, shift, mn, mx), then output
// channel c < nch takes component comp[c]'s sample (pcol[c] < 0) or
// table[clamp(sample, 0, ne - 1) * npc + pcol[c]].  table: ne x npc uint16
// entries in device memory (null when no channel looks up).  zero: src is not
// read, every component counts as finished zero samples.  dst, fmt, layout and
// dstride describe the nch channels; ops (null: none; no sycc) index channels.
struct PalMap {
    uint8_t comp[GRK_MAX_COMPS];
    int8_t pcol[GRK_MAX_COMPS];
    uint32_t nch, ne, npc;
    uint32_t used;  // bit k: component k feeds a channel (set_pal_used)
    int32_t zero;
};
inline void set_pal_used(PalMap &m) {
    m.used = 0;
    for (uint32_t c = 0; c < m.nch && c < (uint32_t)GRK_MAX_COMPS; ++c) m.used |= 1u << (m.comp[c] & 15);
}
hipError_t launch_palette(const PlanePtrs &src, uint32_t sstride, uint32_t tw, uint32_t th, const DstPlanes &dst,
                          int32_t fmt, bool interleaved, uint32_t dstride, uint32_t ncomp, const ShiftArr &shift,
                          const ShiftArr &mn, const ShiftArr &mx, int32_t mct, int32_t irrev, const PalMap &map,
                          const uint16_t *table, const OutOps *ops, hipStream_t s);
// launch_palette for a table of tiles in one launch (the batch decode of JP2
// files, grkgpu_palette_jobs_to): a StoreJob's arguments -- dst, dstride and
// the ops index describing the map's nch <= 4 channels --, the tile's PalMap
// and where its table starts in the launch's merged table of uint16 entries
// (table_off, even, so that the LDS fill keeps its dword path; not read when
// ne = 0).  map.zero: the sources are null and not read.
// grkgpu_palette_job's layout (static_assert in codec.cpp).
struct PalJob {
    StoreJob s;
    PalMap map;
    uint32_t table_off;
};
// The job kernel's shape: 0 planar (one interleaved channel is a plane), 3 / 4
// interleaved runs on the destination's 16-byte grid, 2 interleaved with a
// thread per pixel
__host__ __device__ inline int pal_job_shape(uint32_t nch, bool interleaved) { return interleaved && nch > 1 ? (int)nch : 0; }
constexpr uint32_t PAL_JOB_ROWS = 8;  // rows a workgroup keeps its table for (PAL_ROWS of kernels.hip)
// threads along a row of a job and its workgroups: bands of PAL_JOB_ROWS rows
// by chunks of 256 row threads
__host__ __device__ inline uint32_t pal_job_row_threads(uint32_t w, uint32_t sb, int shape) {
    if (shape == 2) return w;
    const uint32_t n = 16 / sb;
    return (uint32_t)(((uint64_t)w + n - 1) / n + 1);
}
inline uint64_t pal_job_wgs(const PalJob &j, uint32_t sb, int shape) {
    if (!j.s.w || !j.s.h) return 0;
    return (uint64_t)((pal_job_row_threads(j.s.w, sb, shape) + 255) / 256) * ((j.s.h + PAL_JOB_ROWS - 1) / PAL_JOB_ROWS);
}
// The LDS a launch reserves for its jobs' tables, in three classes, so that a
// 16-entry palette does not take 32 KB because another item's has 700 entries:
// 0 no table (direct maps, force-RGB), 1 up to 4 KB, 2 up to 32 KB (the largest
// table: 1024 x 16 entries).
inline int pal_lds_class(uint32_t ne, uint32_t npc) {
    const uint32_t bytes = ne * npc * 2;
    return !bytes ? 0 : (bytes <= 4096 ? 1 : 2);
}
inline uint32_t pal_lds_bytes(int cls) { return cls == 0 ? 0u : (cls == 1 ? 4096u : 32768u); }
// first: njobs + 1 first-workgroup numbers (prefix sums of pal_job_wgs), nwg = first[njobs].  Every job of a
// launch has the sample format, the shape and the op class (op = 0, or 1 = OP_PREC with the OutOps table ops)
// given, and a table of at most lds_bytes.
hipError_t launch_palette_jobs(const PalJob *jobs, const uint32_t *first, uint32_t njobs, uint32_t nwg, int32_t fmt,
                               int shape, int op, const OutOps *ops, const uint16_t *table, uint32_t lds_bytes,
                               hipStream_t s);
// One DWT level of one tile-component (dwt.hip).  A launch runs one level of
// every job in a table (grid.y = job).
struct DwtJob {
    const int32_t *in;     // fwd: resolution samples;     inv: LL band
    const int32_t *coef;   // inv: HL/LH/HH (Mallat)
    int32_t *out;          // fwd: LL band output;         inv: reconstructed resolution
    int32_t *bands;        // fwd: HL/LH/HH output (Mallat)
    uint32_t in_stride, coef_stride, out_stride, bands_stride;  // elements
    uint32_t in_bytes, coef_bytes, out_bytes, bands_bytes;      // buffer extents
    int32_t rw, rh, casx, casy, snx, sny;
    int32_t tiles_x, ntiles;
    // Forward level 0 with the DC shift + MCT fused into its loads
    // (TileProcessor.cpp:1449-1471, mct.cpp:85-139 / 195-350): the window is
    // read from the image planes instead of `in`.  mct_mode 0: not fused;
    // 1: DC shift of src[0]; 2: RCT output component `comp` of src[0..2];
    // 3: ICT output component `comp`.  Samples in format src_fmt (SampleFmt).
    const void *src[3];         // image planes at the tile origin
    uint32_t src_stride, src_bytes;  // elements; bytes from src[i] to its plane's end (min)
    int32_t shift[3];
    // Interleaved pixels (k_dwt_fwd_mct3 only): src[i] = component i of the
    // tile's first pixel, adjacent columns src_pitch (= 3) samples apart,
    // src_stride the row of pixels in samples.
    int32_t mct_mode, comp, src_vec;  // src_vec: pair loads allowed (base aligned to 2 samples, even stride;
                                      // interleaved: src[0] and the row pitch aligned to 2 samples)
    int32_t src_fmt, src_pitch;       // src_pitch: samples between adjacent columns (planar: 1)
    // the windows a launch runs for this job: columns [win_x0, win_x0 +
    // tiles_x), rows [win_y0, win_y0 + win_ny) of the level's window grid
    // (dwt_job_tiles; all of them unless reg_* restricts the output region:
    // window decode, grk_set_decode_area)
    int32_t win_x0, win_y0, win_ny;
    int32_t reg_x0, reg_y0, reg_x1, reg_y1;  // output region (resolution-relative); reg_x1 = 0: all
    int32_t pad2_;
};
// DWT plan options (grkgpu_dwt_options, set by grkgpu_set_dwt_options; the
// defaults are the measured best -- the parity suite forces the others)
struct DwtOptions {
    int32_t fuse_level0 = -1;                    // -1: 3-component 5/3 tiles; 0 never; 1 always
    int32_t f01_rows = 4;                        // 9/7 levels 0 + 1 fused: 2 / 4 / 6 row windows; 0 = apart
    uint64_t f01_min_samples = (uint64_t)1 << 23;  // fuse a level pair from this many samples
    uint64_t f01_small_min_samples = ~(uint64_t)0;  // ... and, with 2 row windows, smaller pairs from this many
    int32_t inv01 = 2;                               // the two largest inverse levels in one launch (k_dwt_inv01):
                                                     // 2 / 4 stage-A row windows per workgroup; 0 = apart
    uint64_t inv01_min_samples = (uint64_t)1 << 23;  // ... when the larger has this many samples
    int32_t pair_group = 0;  // fused level pairs: workgroups walk groups of this many columns top-down (0: row-major)
    int32_t f64_lift = 0;    // forward 9/7 fused pair: lifting in f64 FMA + floor instead of v_mad_i64_i32
    int32_t t1_dec_sort = 1;   // T1 decode: blocks in decreasing order of expected work (-1: only a lone call)
    int32_t t1_dec_bpw = 0;  // T1 decode: blocks per wavefront (0: by block count)
    int32_t mid_th = 0;      // window rows of a level of 2^21 .. 2^23 samples (0: 8)
    int32_t t1_enc_bpw = 0;  // T1 encode (MQ coder): blocks per wavefront (0: by block count)
    int32_t t1_enc_sort = 0; // T1 encode: MQ coder lanes take the blocks heaviest first (device counting sort)
    int32_t pair_kernel = 1;  // fused forward level pairs: 1 = k_dwt_fwd_pair (streamed strips, 5/3 + 9/7),
                              // 0 = k_dwt_fwd01 (9/7 windows, f01_rows)
    int32_t pair_rows = 0;    // k_dwt_fwd_pair: level-(l+1) rows per segment (even; 0 = by size)
    int32_t pair_waves = 0;   // k_dwt_fwd_pair: level-l waves per workgroup (3 / 4; 0 = by width)
    uint64_t pair_min_samples = (uint64_t)1 << 20;  // k_dwt_fwd_pair: fuse pairs from this many level-l samples
    int32_t t1_lone = 0;      // T1 plan: 0 = by the calls in progress, 1 = always the lone plan, -1 = always the batch plan
};
const DwtOptions &dwt_options();
// level geometry code (window rows) for a level of that many samples whose
// smallest resolution is minw x minh
int dwt_pick_th(int irrev, uint64_t level_samples, int minw, int minh);
constexpr int DWT_FUSED = 1 << 16;       // geometry-code flag: forward level with fused DC shift loads
constexpr int DWT_FUSED_MCT3 = 1 << 17;  // ... with fused DC shift + MCT (jobs in component triples)
constexpr int DWT_FMT_SHIFT = 18;        // bits 18-20: SampleFmt of the fused level's image planes (I32 / U8 / U16)
constexpr int DWT_FUSED_PIXELS = 1 << 21;  // ... read from interleaved pixels (MCT triples only)
// the window grid of a job at `th` window rows: tiles_x, ntiles (whole
// workgroups) and win_* (restricted to reg_* when set)
void dwt_job_tiles(int irrev, int th, DwtJob &j);
hipError_t launch_dwt_jobs(const DwtJob *jobs_dev, uint32_t njobs, uint32_t max_tiles, int th, int irrev,
                           int inverse, hipStream_t s);
// forward 9/7 levels 0 and 1 in one launch (dwt.hip k_dwt_fwd01): workgroups
// per job from dwt01_tiles (level-1 geometry), 0 if unsupported
// (ny: level-0 row windows per workgroup, 2 / 4 / 6)
int dwt01_tiles(int irrev, int ny, int rw1, int rh1, int casx1, int casy1, int *tiles_x);
// the last two inverse levels in one launch (k_dwt_inv01): workgroups per job
// for a larger level of rw_b x rh_b; jobsA / jobsB = the two levels
int dwt_inv01_tiles(int irrev, int rw_b, int rh_b, int casx_b, int casy_b);
hipError_t launch_dwt_inv01(const DwtJob *jobsA, const DwtJob *jobsB, uint32_t njobs, uint32_t max_tiles, int irrev,
                            int na, hipStream_t s);
hipError_t launch_dwt_fwd01(const DwtJob *jobs0, const DwtJob *jobs1, uint32_t njobs, uint32_t max_tiles, int irrev,
                            int ny, hipStream_t s);
// forward levels l and l + 1 streamed down column strips (k_dwt_fwd_pair, 5/3
// and 9/7): level-(l+1) core columns per workgroup with nw0 (3 / 4) level-l
// waves, workgroups per job at s1 level-(l+1) rows per segment
int dwt_pair_cw1(int irrev, int nw0);
int dwt_pair_wgs(int irrev, int nw0, int s1, int rw1, int rh1, int casx1, int casy1);
hipError_t launch_dwt_fwd_pair(const DwtJob *jobs0, const DwtJob *jobs1, uint32_t njobs, uint32_t max_wgs, int irrev,
                               int nw0, int s1, hipStream_t s);
// sym: symbol-stream arena; sym_off[i] = block i's byte offset (n+1 entries,
// capacity = (sym_off[i+1]-sym_off[i]) / sym_slot_bytes(w,h) planes), or null
// for the fixed layout of 32 planes x sym_slot_bytes(64,64) per block.
// cblksty: the CBLKSTY_* mode switches of the codestream (t1_lane.h), 0 = none.
// scratch: t1e_scratch_bytes(n, maxdepth) bytes (t1_lane.h EncScratch), with
// maxdepth >= every block's plane capacity (<= 32)
hipError_t launch_t1_encode(const EncBlock *blocks, uint32_t n, const int32_t *coef, void *scratch,
                            uint8_t *sym, const uint64_t *sym_off, uint32_t maxdepth, uint8_t *out, EncResult *res,
                            hipStream_t s, uint32_t cblksty = 0, uint32_t bpw = 0, uint32_t *order = nullptr);
// device words the MQ coder's work order needs (launch_t1_encode `order`)
uint32_t t1_order_words(uint32_t nblocks);
// Pass records formed on the device when a layer is rate-controlled: the
// host's per-pass loop of the encoder (codec.cpp: rate, length, termination
// t1.cpp:1131-1151, cumulative distortion t1.cpp:1249-1254 with
// t1_getwmsedec :912-930, and the block's slope range, t2.cpp block_slopes)
// moved next to the results it reads, so only records cross PCIe and the
// host's Tier-2 starts at the layer formation.  DevPass has EncPass's layout
// (t2.h; static_assert in codec.cpp); block i's records go to
// out[pass0[i] .. pass0[i + 1]) -- slots sized from the band's bit-plane
// bound -- and its summary to sum[i].
struct DevPass {
    uint32_t rate, len;
    double dd;
    uint16_t slope;
    uint8_t term;
};
struct PassSum {
    uint32_t numbps, numpasses, len, nsym;
    uint32_t bad;  // 1: numbps above the band's bound, 2: more passes than slots, 4: MQ slab overflow
    uint32_t z0;   // EncCblkState::z0
    double smin, smax, s0max, disto;
};
hipError_t launch_pass_records(const EncBlock *blocks, const EncResult *res, const double *wfac, const uint64_t *pass0,
                               uint32_t n, uint32_t cblksty, DevPass *out, PassSum *sum, hipStream_t s);
// Per-pass distortion sums of the blocks k_t1_model coded (same scratch and
// maxdepth): nmsedec[pass] of every block, in the pass order of
// t1_encode_cblk (t1.cpp:1222-1260).
hipError_t launch_t1_dist(const EncBlock *blocks, uint32_t n, uint32_t maxdepth, const int32_t *coef,
                          const void *scratch, EncResult *res, hipStream_t s);
// ubuf: unstuffed-stream arena; block i's region at ubuf + i * fixed_words
// words, or (fixed_words == 0) at blocks[i].pad * 16 bytes
// (t1_unstuff_region_words words each).
// segs / seg_first: the codeword segments of every block (block i's are
// segs[seg_first[i] .. seg_first[i+1]), each with its own unstuffed region at
// ubuf + ub_off * 16 bytes); null: one segment per block at blocks[i].data_off.
// cblksty: CBLKSTY_* mode switches; roi: per-block ROI shift (null: none).
hipError_t launch_t1_decode(const DecBlock *blocks, uint32_t n, const uint8_t *data, T1Scratch *scratch,
                            int32_t *tiles, hipStream_t s, uint32_t *ubuf, uint32_t fixed_words,
                            const DecSeg *segs = nullptr, const uint32_t *seg_first = nullptr, uint32_t cblksty = 0,
                            const uint8_t *roi = nullptr, uint32_t bpw = 0);
// blocks per wavefront (bpw, a power of two <= 64; 0 = the options' value or
// the block-count rule) of the T1 kernels' lane-per-block launches, and the
// rule for a call that has the GPU to itself (lone_bpw): enough wavefronts
// to give every SIMD of the chip one and a half (1,536), not full lanes
uint32_t lone_bpw(uint32_t nblocks);
// 32-bit words of a block's unstuffed-stream region (header + words + carries)
inline uint32_t t1_unstuff_region_words(uint32_t len) { return 4 + unstuff_word_cap(len) + unstuff_carry_cap(len); }
hipError_t launch_gather(const uint8_t *hdr, const uint8_t *slab, const GatherItem *items, uint32_t n, uint8_t *dst,
                         hipStream_t s);

// One product of the forward ICT (mct.cpp:195-350), int_fix_mul(r << 11, c)
// = (2048 r c + 4096) >> 13 with the 64-bit product, for a DC-shifted sample
// r (|r| <= 2^16, precision <= 16 bits): 2048 (r c + 2) / 8192 = (r c + 2) / 4,
// so the same value is floor((r c + 2) / 4) in 32-bit arithmetic (|r c| < 2^30).
__device__ __forceinline__ int32_t ict_term(int32_t r, int32_t c) { return (r * c + 2) >> 2; }

}  // namespace grkgpu
